#!/usr/bin/env python3
"""ehyb_pcg_cheb (CG with a Chebyshev polynomial preconditioner) against ehyb_pcg and ehyb_pcg_refine on the bench workload's
SPD system -- the M-matrix of tools/cg_multi_time.py (off-diagonals negative, diagonal = row sum + shift * mean), Jacobi
scaling, a random b -- to a relative residual of 1e-10.  Arms, alternating in one process, `rounds` rounds after one warm-up
solve per arm (every shape, graph and code object of the timed window has run once), the smallest figure per arm kept and the
spread over the rounds beside it:

  pcg               ehyb_pcg on the fp64 plan
  pcg_refine        ehyb_pcg_refine, fp64 plan outside, val_f32 plan inside (inner rtol 1e-5)
  cheb-d fp64       ehyb_pcg_cheb of degree d = 2, 4, 8, the polynomial on the fp64 plan itself
  cheb-d val_f32    the same with the polynomial on the cfg.val_f32 plan of the same reordered matrix
  cheb-4 val_f32 half-keep   both plans built with cfg.ell_keep at half its automatic value: the two plans' pinned slab sets
                    share the Infinity Cache

Per arm: iterations, microseconds per iteration (device time of the whole call between HIP events -- set-up, allocations and
check points included -- over the iterations; for pcg_refine over the inner iterations) and the host's wall time of the whole
call.  lmax is the library's own default (1.1 * ehyb_lambda_max, 20 steps), estimated once per polynomial plan outside the timed
window and passed in; the estimate's own time is reported.  Every answer is checked on the CPU against the fp64 matrix
(reached: ||b - A x|| <= 2e-10 ||b|| and the reported residual <= 1e-10).

usage: python tools/pcg_cheb_time.py [--workload audikw_1-like] [--rounds 3] [--shift 1e-2,1e-4] [--out profiles/pcg_cheb_time_audikw.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cg_multi_time import hip_events  # noqa: E402

TARGET = 1e-10
DEGREES = (2, 4, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shift", default="1e-2,1e-4", help="diagonal = row sum + shift * mean, one line of output per value: the smaller, the harder")
    ap.add_argument("--sym", type=int, default=1, help="1: symmetric pair storage (the bench default for this workload), 0: every entry")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench as B
    import ehyb_spmv_gpu_amd as E

    if E.device_count() < 1:
        raise SystemExit("pcg_cheb_time: no HIP device visible (there is no CPU fallback)")
    lines = [measure(args, B, E, float(shift)) for shift in args.shift.split(",")]
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def measure(args, B, E, shift):
    hip = hip_events()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    st = E.Stream()

    def timed(fn):
        """-> (device ms between the events, host wall ms, fn's result)"""
        t0 = time.perf_counter()
        assert hip.hipEventRecord(ev0, st.ptr) == 0
        out = fn()
        assert hip.hipEventRecord(ev1, st.ptr) == 0 and hip.hipEventSynchronize(ev1) == 0
        wall = (time.perf_counter() - t0) * 1e3
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return ms.value, wall, out

    gen, gargs, _ = B.WORKLOADS[args.workload]
    kw = dict(partitioner=B.partitioner_for(E, gen), sym_pairs=args.sym)
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    I, J, V = m.I, m.J, m.V
    V[I != J] = -np.abs(V[I != J])
    off = np.bincount(I, weights=np.abs(V) * (I != J), minlength=m.n)
    V[I == J] = (off + shift * off.mean())[I[I == J]]          # the M-matrix of tools/cg_multi_time.py
    m.reorder(cfg)
    n = m.n
    A = sp.csr_matrix((m.V.copy(), m.J.copy(), m.row_idx.astype(np.int64)), shape=(n, n))
    A.sort_indices()
    lib = E.host._lib.load()
    plans = {"fp64": E.Plan(m, cfg), "val_f32": E.Plan(m, E.make_config(val_f32=1, **kw))}
    keeps = {}
    for a in ("fp64", "val_f32"):
        s = plans[a].stats
        value = plans[a].device_value_bytes[0]
        auto = lib.ehyb_ell_auto_keep1024(value, s["bytes_format_ell"] - 8 * s["size_block_ell"])
        keeps[a] = dict(automatic_keep1024=auto, half_keep_per_mille=max(1, auto * 1000 // 1024 // 2), resident_bytes=plans[a].resident_bytes)
    plans["fp64 half-keep"] = E.Plan(m, E.make_config(ell_keep=keeps["fp64"]["half_keep_per_mille"], **kw))
    plans["val_f32 half-keep"] = E.Plan(m, E.make_config(val_f32=1, ell_keep=keeps["val_f32"]["half_keep_per_mille"], **kw))
    for a in ("fp64 half-keep", "val_f32 half-keep"):
        keeps[a] = dict(resident_bytes=plans[a].resident_bytes)
    m.free()

    rng = np.random.default_rng(1)
    b = rng.uniform(-1, 1, n)
    nb = np.linalg.norm(b)
    db, dinv, dsol = E.DeviceBuffer(n).upload(b), E.DeviceBuffer(n).upload(1.0 / A.diagonal()), E.DeviceBuffer(n)
    zeros = np.zeros(n)
    vp = C.c_void_p

    # lmax per polynomial plan, outside the timed window
    lmax, estimate_ms = {}, {}
    for a in plans:
        lam = C.c_double(0)
        for _ in range(2):   # (the second one is the timed one)
            ms, _, rc = timed(lambda: lib.ehyb_lambda_max(plans[a].h, vp(dinv.ptr), 20, vp(st.ptr), C.byref(lam)))
            assert rc == 0, lib.ehyb_last_error()
        lmax[a], estimate_ms[a] = 1.1 * lam.value, round(ms, 3)

    def pcg():
        done, rel = C.c_int(0), C.c_double(0)
        rc = lib.ehyb_pcg(plans["fp64"].h, vp(dinv.ptr), vp(db.ptr), vp(dsol.ptr), 100000, TARGET, 10, vp(st.ptr), C.byref(done), C.byref(rel))
        return rc, done.value, done.value, rel.value, {}

    def refine():
        outer, inner, rel = C.c_int(0), C.c_int(0), C.c_double(0)
        rc = lib.ehyb_pcg_refine(plans["fp64"].h, plans["val_f32"].h, vp(dinv.ptr), vp(db.ptr), vp(dsol.ptr), 20, 100000, TARGET, 1e-5,
                                 vp(st.ptr), C.byref(outer), C.byref(inner), C.byref(rel))
        return rc, inner.value, inner.value, rel.value, dict(outer=outer.value)

    def cheb(plan, poly, degree):
        def run():
            done, rel = C.c_int(0), C.c_double(0)
            rc = lib.ehyb_pcg_cheb(plans[plan].h, plans[poly].h, vp(dinv.ptr), vp(db.ptr), vp(dsol.ptr), degree, 0.0, lmax[poly], 100000, TARGET,
                                   2, vp(st.ptr), C.byref(done), C.byref(rel))
            return rc, done.value, done.value, rel.value, dict(degree=degree, multiplies=(1 + degree) * done.value, lmax=lmax[poly])
        return run

    arms = {"pcg": pcg, "pcg_refine": refine}
    for d in DEGREES:
        arms[f"cheb-{d} fp64"] = cheb("fp64", "fp64", d)
        arms[f"cheb-{d} val_f32"] = cheb("fp64", "val_f32", d)
    arms["cheb-4 val_f32 half-keep"] = cheb("fp64 half-keep", "val_f32 half-keep", 4)

    dev_ms, wall_ms, info = {a: [] for a in arms}, {a: [] for a in arms}, {}
    for rnd in range(args.rounds + 1):      # round 0: the warm-up
        for a, fn in arms.items():
            dsol.upload(zeros)
            ms, wall, (rc, iters, per, rel, extra) = timed(fn)
            assert rc == 0, (a, lib.ehyb_last_error())
            true = np.linalg.norm(b - A @ dsol.download()) / nb
            extra["reached"] = bool(rel <= TARGET and true <= 2 * TARGET)        # (recorded, not asserted: a stagnating refinement is a result)
            if rnd:
                dev_ms[a].append(ms)
                wall_ms[a].append(wall)
            info[a] = dict(iterations=iters, rel_residual=float(f"{rel:.3e}"), recomputed=float(f"{true:.3e}"), **extra)

    def spread(v):
        return round((max(v) - min(v)) / min(v), 4)

    line = dict(workload=args.workload, storage="symmetric pairs" if args.sym else "every entry", n=n, nnz=int(A.nnz), rounds=args.rounds,
                target=TARGET, shift=shift, lambda_max_ms=estimate_ms, keep=keeps,
                arms={a: dict(us_per_iteration=round(min(dev_ms[a]) * 1e3 / max(1, info[a]["iterations"]), 1), device_ms=round(min(dev_ms[a]), 3),
                              wall_ms=round(min(wall_ms[a]), 3), spread=spread(wall_ms[a]), **info[a]) for a in arms})
    print(json.dumps(line), flush=True)
    for p in plans.values():
        p.destroy()
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()
    return line


if __name__ == "__main__":
    main()
