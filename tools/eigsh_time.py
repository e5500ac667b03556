#!/usr/bin/env python3
"""What ehyb_eigsh costs on the audikw_1-like symmetric plan (the bench matrix with symmetric pair storage, made the M-matrix of
tools/pcg_cheb_time.py: off-diagonals negative, diagonal = row sum + shift * mean): a Lanczos step against a two-pass GMRES step at
the same basis size, a restart against the bytes it must move, and two solves end to end.

Per step.  The step's launches one at a time through the *_step building blocks, which use the grid the solves use at this size:
the multiply, dots, update, dots, update on j + 1 columns, then eigsh's next(j) or GMRES's.  HIP events on the tool's stream
around the six launches; the tail (status, counter, planted g~_j = bb = 1 so that neither next stops) is uploaded afresh before
every step, outside the events.  The basis holds unit random columns and w a random vector: the kernels' work does not depend on
the values.  j = 1 .. 63, the arms alternating within a round, the smallest of --rounds kept.

Restart.  eigsh_rotate_kernel (ehyb_eigsh_rotate_step) and the device-to-device copy back of kc columns at (mc, kc) = (20, 13),
(64, 41), (65, 17); the bytes the kernel must move, 8 n (mc ceil(kc / 8) + kc), over its time as a fraction of the read bandwidth
ehyb_measure_read_bw reports; a restart (rotation + copy) as a share of the steady cycle of nev 4 at the default basis
(m = 20, keep = 12: steps j = 12 .. 19 from the per-step figures, restart at (21, 13)).

End to end.  nev = 4 largest to tol 1e-8 with and without the Jacobi scale: multiplies, restarts, wall time around the call (best of
--rounds), every pair's true residual recomputed on the CPU; and Plan.spectrum_bounds of D^-1 A beside 1.1 * ehyb_lambda_max and
that over 30, the defaults of ehyb_pcg_cheb.

usage: python tools/eigsh_time.py [--workload audikw_1-like] [--shift 1e-2] [--sym 1] [--rounds 3] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--shift", type=float, default=1e-2)
    ap.add_argument("--sym", type=int, default=1, help="cfg.sym_pairs of the plan")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import scipy.sparse as sp

    import bench as B
    import ehyb_spmv_gpu_amd as E
    from ehyb_spmv_gpu_amd import _lib

    hip = hip_events()
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
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
    cfg = E.make_config(partitioner=B.partitioner_for(E, gen), sym_pairs=args.sym)
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    I, J, V = m.I, m.J, m.V
    V[I != J] = -np.abs(V[I != J])
    off = np.bincount(I, weights=np.abs(V) * (I != J), minlength=m.n)
    V[I == J] = (off + args.shift * off.mean())[I[I == J]]
    m.reorder(cfg)
    n = m.n
    A = sp.csr_matrix((m.V.copy(), m.J.copy(), m.row_idx.astype(np.int64)), shape=(n, n))      # the permuted numbering, for the CPU checks
    plan = E.Plan(m, cfg)
    print(f"# {args.workload}: n={n} nnz={m.nnz} sym_pairs={plan.stats['sym_pairs']}", flush=True)
    m.free()
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
    dV = E.DeviceBuffer(ld * cols)
    column = np.zeros(ld)
    for c in range(cols):                                        # one column at a time: no second copy of the basis on the host
        column[:n] = rng.standard_normal(n) / np.sqrt(n)
        ok(lib.ehyb_h2d(vp(dV.ptr + 8 * ld * c), column.ctypes.data_as(vp), column.nbytes))
    w_host = rng.standard_normal(n)
    dw, dz = E.DeviceBuffer(ld), E.DeviceBuffer(ld).upload(np.r_[w_host, np.zeros(ld - n)])            # z: the multiply's input
    slots = np.zeros(L["slots"] * L["slot_doubles"] + L["tail_doubles"])
    tail_at = L["slots"] * L["slot_doubles"]
    ds = E.DeviceBuffer(len(slots))

    def step(arm, j):
        tail = slots.copy()
        tail[tail_at + L["gt_at"] + j] = 1.0
        tail[tail_at + L["bb_at"]] = 1.0
        ds.upload(tail)
        s, V_, w_, z_ = vp(ds.ptr), vp(dV.ptr), vp(dw.ptr), vp(dz.ptr)

        def launches():
            plan.spmv(dz.ptr, dw.ptr, stream=st.ptr, walk=j & 1)
            for p in (0, 1):
                ok(lib.ehyb_gmres_dots_step(n, ld, V_, w_, j + 1, s, vp(st.ptr)))
                ok(lib.ehyb_gmres_update_step(n, ld, V_, w_, j + 1, s, p, p, vp(st.ptr)))
            if arm == "eigsh":
                ok(lib.ehyb_eigsh_next_step(n, ld, V_, w_, None, z_, s, j, vp(st.ptr)))
            else:
                ok(lib.ehyb_gmres_next_step(n, ld, V_, w_, None, z_, s, j, 2, 0.0, vp(st.ptr)))

        us, _ = timed_us(launches)
        flags = ds.download()[tail_at + L["flags_at"]:tail_at + L["flags_at"] + 1].view(np.int32)
        assert flags[L["flag_status"]] == L["status_running"] and flags[L["flag_iters"]] == 1, (arm, j, flags)
        return us

    def multiplies():
        for i in range(50):
            plan.spmv(dz.ptr, dw.ptr, stream=st.ptr, walk=i & 1)
        ok(lib.ehyb_stream_sync(vp(st.ptr)))

    multiplies()
    us_multiply = min(timed_us(multiplies)[0] for _ in range(args.rounds)) / 50
    emit(dict(workload=args.workload, kind="multiply", n=n, us=round(us_multiply, 1)))
    js = list(range(1, L["max_restart"]))
    best = {}
    for arm in ("eigsh", "gmres"):
        step(arm, js[-1])                                        # warm
    for r in range(args.rounds):
        for j in js:
            for arm in (("eigsh", "gmres") if (j + r) % 2 == 0 else ("gmres", "eigsh")):
                us = step(arm, j)
                best[arm, j] = min(best.get((arm, j), us), us)
    for j in js:
        emit(dict(workload=args.workload, kind="step", j=j, us_eigsh=round(best["eigsh", j], 1), us_gmres_2pass=round(best["gmres", j], 1),
                  ratio=round(best["eigsh", j] / best["gmres", j], 3)))
    ratios = [best["eigsh", j] / best["gmres", j] for j in js]
    emit(dict(workload=args.workload, kind="step_summary", us_multiply=round(us_multiply, 1), ratio_min=round(min(ratios), 3),
              ratio_median=round(float(np.median(ratios)), 3), ratio_max=round(max(ratios), 3),
              total_us_eigsh=round(sum(best["eigsh", j] for j in js), 1), total_us_gmres_2pass=round(sum(best["gmres", j] for j in js), 1)))

    # ---------------------------------------------------------------- restart
    gbps = C.c_double(0)
    ok(lib.ehyb_measure_read_bw(1 << 30, 10, C.byref(gbps)))
    dV2, dY = E.DeviceBuffer(ld * 64), E.DeviceBuffer(65 * 64)
    restart_us = {}
    for mc, kc in ((20, 13), (64, 41), (65, 17), (21, 13)):
        Y = np.linalg.qr(rng.standard_normal((mc, mc)))[0][:, :kc]
        dY.upload(np.r_[Y.T.ravel(), np.zeros(65 * 64 - mc * kc)])
        rot = lambda: ok(lib.ehyb_eigsh_rotate_step(n, ld, vp(dV.ptr), ld, vp(dV2.ptr), vp(dY.ptr), mc, kc, vp(st.ptr)))         # noqa: E731
        # the copy goes into a third buffer of the same size: V itself stays the rotation's input for the next round
        dV3 = E.DeviceBuffer(ld * kc)
        cpy = lambda: ok(hip.hipMemcpyAsync(vp(dV3.ptr), vp(dV2.ptr), 8 * ld * kc, 3, vp(st.ptr)))                                  # noqa: E731
        rot(), cpy()
        us_rot = min(timed_us(rot)[0] for _ in range(args.rounds + 2))
        us_cpy = min(timed_us(cpy)[0] for _ in range(args.rounds + 2))
        moved = 8 * n * (mc * -(-kc // 8) + kc)
        restart_us[mc, kc] = us_rot + us_cpy
        emit(dict(workload=args.workload, kind="restart", mc=mc, kc=kc, us_rotate=round(us_rot, 1), us_copy=round(us_cpy, 1), MB=round(moved / 1e6, 1),
                  rotate_GBps=round(moved / us_rot / 1e3, 1), read_bw_GBps=round(gbps.value, 1), fraction_of_read_bw=round(moved / us_rot / 1e3 / gbps.value, 3)))
        dV3.free()
    cycle = sum(best["eigsh", j] for j in range(12, 20))
    emit(dict(workload=args.workload, kind="restart_share", nev=4, basis=20, keep=12, us_cycle_steps=round(cycle, 1), us_restart=round(restart_us[21, 13], 1),
              share_of_cycle=round(restart_us[21, 13] / (cycle + restart_us[21, 13]), 3)))
    for b in (dV, dV2, dY, ds):
        b.free()

    # ---------------------------------------------------------------- end to end
    d = A.diagonal()
    for name, scale in (("plain", None), ("jacobi", 1.0 / np.sqrt(d))):
        wall, got = None, None
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            got = plan.eigsh(4, "LA", tol=1e-8, scale=scale, stream=st.ptr)
            ms = (time.perf_counter() - t0) * 1e3
            wall = ms if wall is None else min(wall, ms)
        ev, X, info = got
        op = (lambda x: A @ x) if scale is None else (lambda x: scale * (A @ (scale * x)))
        true = max(float(np.linalg.norm(op(X[i]) - ev[i] * X[i])) for i in range(len(ev))) / float(np.abs(ev).max())
        emit(dict(workload=args.workload, kind="solve", operator=name, nev=4, which="LA", tol=1e-8, found=info["found"], nconv=info["nconv"],
                  multiplies=info["multiplies"], restarts=info["restarts"], wall_ms=round(wall, 2), wall_includes="staging scale and the vectors through the host",
                  evals=[float(f"{v:.12g}") for v in ev], true_residual_over_nrm=float(f"{true:.3e}")))
    t0 = time.perf_counter()
    lo, hi = plan.spectrum_bounds(1.0 / d, stream=st.ptr)
    ms_bounds = (time.perf_counter() - t0) * 1e3
    lam = plan.lambda_max(1.0 / d, stream=st.ptr)
    emit(dict(workload=args.workload, kind="bounds", operator="D^-1 A", lmin=float(f"{lo:.9g}"), lmax=float(f"{hi:.9g}"), wall_ms=round(ms_bounds, 2),
              lambda_max_20_steps=float(f"{lam:.9g}"), cheb_default_lmax=float(f"{1.1 * lam:.9g}"), cheb_default_lmin=float(f"{1.1 * lam / 30:.9g}")))
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()


if __name__ == "__main__":
    main()
