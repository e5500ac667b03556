#!/usr/bin/env python3
"""What ehyb_svds costs on the audikw_1-like plan (the bench matrix with EVERY entry stored -- cfg.sym_pairs = 0, so that
ehyb_spmv_t runs on it -- and a second plan of A^T in the same numbering, Matrix.transposed_like): a full step of the
bidiagonalisation against a Lanczos step of ehyb_eigsh at the same basis size, and two solves end to end.

Per step.  The step's launches one at a time through the *_step building blocks, which use the grid the solves use at this size.
  svds   the multiply on the plan of A, dots, update, dots, update on j columns of Q, next(left, j); the multiply on the plan of
         A^T, dots, update, dots, update on j + 1 columns of P, next(right, j): twelve launches
  eigsh  the multiply, dots, update, dots, update on j + 1 columns, eigsh's next(j): six launches
HIP events on the tool's stream around the launches; the tail (status, counter) is uploaded afresh before every step, outside the
events.  The bases hold unit random columns and w a random vector: the kernels' work does not depend on the values.  j = 1, 20 and
63, the arms alternating within a round, the smallest of --rounds kept.  The expectation, a count of launches and bytes: a full
step costs about two Lanczos steps.

End to end.  nsv = 4 to tol 1e-8 with the plan of A^T and with ehyb_spmv_t: multiplies, restarts, wall time around the call (best
of --rounds), every triplet's two true residuals recomputed on the CPU.

usage: python tools/svds_time.py [--workload audikw_1-like] [--rounds 3] [--out profiles/svds_time_audikw.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cg_multi_time import hip_events  # noqa: E402

STEPS = (1, 20, 63)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import scipy.sparse as sp

    import bench as B
    import ehyb_spmv_gpu_amd as E
    from ehyb_spmv_gpu_amd import _lib

    hip = hip_events()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    st = E.Stream()
    vp = C.c_void_p

    def timed_us(fn):
        assert hip.hipEventRecord(ev0, st.ptr) == 0
        out = fn()
        assert hip.hipEventRecord(ev1, st.ptr) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return ms.value * 1e3, out

    gen, gargs, _ = B.WORKLOADS[args.workload]
    cfg = E.make_config(partitioner=B.partitioner_for(E, gen), sym_pairs=0)
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    m.reorder(cfg)
    n = m.n
    A = sp.csr_matrix((m.V.copy(), m.J.copy(), m.row_idx.astype(np.int64)), shape=(n, n))      # the permuted numbering, for the CPU checks
    plan = E.Plan(m, cfg)
    mt = m.transposed_like(cfg)
    plan_t = E.Plan(mt, cfg)
    print(f"# {args.workload}: n={n} nnz={m.nnz} sym_pairs={plan.stats['sym_pairs']} spmv_t_supported={plan.spmv_t_supported}", flush=True)
    m.free()
    mt.free()
    lib = _lib.load()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    def ok(rc):
        assert rc == 0, lib.ehyb_last_error()

    # ---------------------------------------------------------------- per step
    L = _lib.GmresSlots()
    ok(lib.ehyb_gmres_layout(C.byref(L)))
    L = L.as_dict()
    cols = L["max_restart"] + 1
    ld = n + (n & 1)
    rng = np.random.default_rng(1)
    dP, dQ = E.DeviceBuffer(ld * cols), E.DeviceBuffer(ld * cols)
    column = np.zeros(ld)
    for d in (dP, dQ):
        for c in range(cols):                                    # one column at a time: no second copy of a basis on the host
            column[:n] = rng.standard_normal(n) / np.sqrt(n)
            ok(lib.ehyb_h2d(vp(d.ptr + 8 * ld * c), column.ctypes.data_as(vp), column.nbytes))
    dw, dz = E.DeviceBuffer(ld), E.DeviceBuffer(ld).upload(np.r_[rng.standard_normal(n), np.zeros(ld - n)])
    slots = np.zeros(L["slots"] * L["slot_doubles"] + L["tail_doubles"])
    tail_at = L["slots"] * L["slot_doubles"]
    ds = E.DeviceBuffer(len(slots))

    def step(arm, j):
        ds.upload(slots)
        s, P_, Q_, w_, z_ = vp(ds.ptr), vp(dP.ptr), vp(dQ.ptr), vp(dw.ptr), vp(dz.ptr)

        def ortho(basis, count):
            for p in (0, 1):
                ok(lib.ehyb_gmres_dots_step(n, ld, basis, w_, count, s, vp(st.ptr)))
                ok(lib.ehyb_gmres_update_step(n, ld, basis, w_, count, s, p, p, vp(st.ptr)))

        def svds():
            plan.spmv(dP.ptr + 8 * ld * j, dw.ptr, stream=st.ptr, walk=j & 1)
            ortho(Q_, j)
            ok(lib.ehyb_svds_next_step(n, ld, Q_, w_, s, 0, j, vp(st.ptr)))
            plan_t.spmv(dQ.ptr + 8 * ld * j, dw.ptr, stream=st.ptr, walk=1 - (j & 1))
            ortho(P_, j + 1)
            ok(lib.ehyb_svds_next_step(n, ld, P_, w_, s, 1, j, vp(st.ptr)))

        def eigsh():
            plan.spmv(dz.ptr, dw.ptr, stream=st.ptr, walk=j & 1)
            ortho(P_, j + 1)
            ok(lib.ehyb_eigsh_next_step(n, ld, P_, w_, None, z_, s, j, vp(st.ptr)))

        us, _ = timed_us(svds if arm == "svds" else eigsh)
        flags = ds.download()[tail_at + L["flags_at"]:tail_at + L["flags_at"] + 1].view(np.int32)
        assert flags[L["flag_status"]] == L["status_running"] and flags[L["flag_iters"]] == (2 if arm == "svds" else 1), (arm, j, flags)
        return us

    best = {}
    for arm in ("svds", "eigsh"):
        step(arm, STEPS[-1])                                     # warm
    for r in range(args.rounds):
        for j in STEPS:
            for arm in (("svds", "eigsh") if (j + r) % 2 == 0 else ("eigsh", "svds")):
                us = step(arm, j)
                best[arm, j] = min(best.get((arm, j), us), us)
    for j in STEPS:
        emit(dict(workload=args.workload, kind="step", j=j, n=n, us_svds_full_step=round(best["svds", j], 1), us_eigsh_step=round(best["eigsh", j], 1),
                  ratio=round(best["svds", j] / best["eigsh", j], 3)))
    for b in (dP, dQ, dw, dz, ds):
        b.free()

    # ---------------------------------------------------------------- end to end
    for name, pt in (("plan_t", plan_t), ("ehyb_spmv_t", None)):
        wall, got = None, None
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            got = plan.svds(4, plan_t=pt, tol=1e-8, stream=st.ptr)
            ms = (time.perf_counter() - t0) * 1e3
            wall = ms if wall is None else min(wall, ms)
        s, U, V, info = got
        right = max(float(np.linalg.norm(A @ V[i] - s[i] * U[i])) for i in range(len(s))) / float(s[0])
        left = max(float(np.linalg.norm(A.T @ U[i] - s[i] * V[i])) for i in range(len(s))) / float(s[0])
        emit(dict(workload=args.workload, kind="solve", transposed=name, nsv=4, tol=1e-8, found=info["found"], nconv=info["nconv"],
                  multiplies=info["multiplies"], restarts=info["restarts"], wall_ms=round(wall, 2), wall_includes="staging the vectors through the host",
                  svals=[float(f"{v:.12g}") for v in s], true_right_residual_over_s0=float(f"{right:.3e}"),
                  true_left_residual_over_s0=float(f"{left:.3e}")))
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()


if __name__ == "__main__":
    main()
