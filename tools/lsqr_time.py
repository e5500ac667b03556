#!/usr/bin/env python3
"""Time per iteration of ehyb_lsqr, with a plan of A^T and with ehyb_spmv_t, beside one ehyb_bicgstab iteration in the same run.

The system is that of tools/bicgstab_time.py: the bench workload (audikw_1-like) made unsymmetric with the same pattern -- every
off-diagonal value above the diagonal scaled by (1 + c), every one below by (1 - c), the diagonal set to the row sum of |a_ij|
plus --shift times its mean.  Its transpose is the same construction at -c with the diagonal kept, so the plan of A^T is built from that matrix put on
A's permutation and partitions (Matrix.reorder_like) -- what Matrix.transposed_like gives, without sorting 77 million entries in
Python.  Plain storage.  LSQR has no preconditioner; BiCGSTAB runs Jacobi-preconditioned as in bicgstab_time.py (one more load
per element in two of its vector kernels), so that its figure is the one published there.  atol = btol = 0 and rtol = 0 keep
every solve iterating: the work per iteration does not depend on the residual.

Arms: "lsqr_plan_t" (two ehyb_spmv_walk multiplies per iteration, one per plan), "lsqr_spmv_t" (one ehyb_spmv_walk, one
ehyb_spmv_t), "bicgstab" (two ehyb_spmv_walk on A).  A figure is the difference of two solves (--iters lo,hi) divided by
hi - lo, each timed with HIP events on the tool's stream around a call that ends in a synchronise, so that one-off costs
(workspace, capture, the start) cancel.  Every solve must run all its iterations.  The arms alternate within the process,
--rounds rounds, and the smallest figure per arm is kept.  One JSON line per arm.

usage: python tools/lsqr_time.py [--workload audikw_1-like] [--c 0.3] [--iters 10,60] [--shift 1e-2] [--rounds 3]
                                 [--out profiles/lsqr_time_audikw.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from cg_multi_time import hip_events  # noqa: E402

# launches per iteration: multiplies, vector kernels
LAUNCHES = {"lsqr_plan_t": (2, 3), "lsqr_spmv_t": (2, 3), "bicgstab": (2, 5)}


def unsymmetric_matrix(E, gen, gargs, cfg, c, shift, diag=None):
    """the system of bicgstab_time.unsymmetric_system in the ORIGINAL numbering (not reordered) -> (matrix, its diagonal by row).
    With -c and the diagonal of the matrix at c handed in it is that matrix's transpose."""
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    I, J, V = m.I, m.J, m.V
    V[I < J] *= 1.0 + c
    V[I > J] *= 1.0 - c
    if diag is None:
        off = np.bincount(I, weights=np.abs(V) * (I != J), minlength=m.n)
        diag = off + shift * off.mean()
    V[I == J] = diag[I[I == J]]
    return m, diag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--c", type=float, default=0.3, help="off-diagonals x (1 + c) above, x (1 - c) below the diagonal")
    ap.add_argument("--iters", default="10,60")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shift", type=float, default=1e-2, help="diagonal = row sum of |a_ij| + shift * its mean")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench as B
    import ehyb_spmv_gpu_amd as E

    lo, hi = [int(v) for v in args.iters.split(",")]
    hip = hip_events()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    st = E.Stream()

    def timed_ms(fn):
        assert hip.hipEventRecord(ev0, st.ptr) == 0
        out = fn()                                   # returns after its own stream synchronise
        assert hip.hipEventRecord(ev1, st.ptr) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return ms.value, out

    gen, gargs, _ = B.WORKLOADS[args.workload]
    cfg = E.make_config(partitioner=B.partitioner_for(E, gen), sym_pairs=2)
    m, diag_by_row = unsymmetric_matrix(E, gen, gargs, cfg, args.c, args.shift)
    m.reorder(cfg)
    I, J, V = m.I, m.J, m.V
    diag = np.zeros(m.n)
    diag[I[I == J]] = V[I == J]
    inv = E.DeviceBuffer(m.n).upload(1.0 / diag)
    plan = E.Plan(m, cfg)
    mt = unsymmetric_matrix(E, gen, gargs, cfg, -args.c, args.shift, diag_by_row)[0].reorder_like(m)
    plan_t = E.Plan(mt, cfg)
    n = plan.n
    for name, p in (("A", plan), ("A^T", plan_t)):
        s = p.stats
        print(f"# {args.workload}, c = {args.c}, {name}: n={n} nnz_ell={s['nnz_ell']} nnz_er={s['nnz_er']} sym_pairs={s['sym_pairs']}", flush=True)
    # the plan of A^T is A^T: one multiply of each against the other's transpose through x.(A y) = (A^T x).y
    rng = np.random.default_rng(1)
    xv, yv = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    dxv, dyv, dout = E.DeviceBuffer(n).upload(xv), E.DeviceBuffer(n).upload(yv), E.DeviceBuffer(n)
    plan.spmv(dyv.ptr, dout.ptr)
    lhs = xv @ dout.download()
    plan_t.spmv(dxv.ptr, dout.ptr)
    rhs = dout.download() @ yv
    assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs), 1.0), (lhs, rhs)
    m.free()
    mt.free()
    db = E.DeviceBuffer(n).upload(rng.uniform(-1, 1, n))
    dx = E.DeviceBuffer(n)
    zeros = np.zeros(n)
    lib = E.host._lib.load()

    def run(arm, it):
        """-> the residual figure of the solve; asserts that all `it` iterations ran"""
        if arm == "bicgstab":
            done, rel = C.c_int(0), C.c_double(0)
            rc = lib.ehyb_bicgstab(plan.h, C.c_void_p(inv.ptr), C.c_void_p(db.ptr), C.c_void_p(dx.ptr), it, 0.0, 10, C.c_void_p(st.ptr), C.byref(done), C.byref(rel))
            assert rc == 0 and done.value == it, (arm, rc, done.value, lib.ehyb_last_error())
            return rel.value
        info = E.host._lib.LsqrInfo()
        rc = lib.ehyb_lsqr(plan.h, plan_t.h if arm == "lsqr_plan_t" else None, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), 0.0, 0.0, 0.0, it, 10,
                           C.c_void_p(st.ptr), C.byref(info))
        assert rc == 0 and info.iters == it and info.istop == 7, (arm, rc, info.as_dict(), lib.ehyb_last_error())
        return info.rnorm

    arms = list(LAUNCHES)
    for arm in arms:
        dx.upload(zeros)
        run(arm, lo)                                 # warm
    best, res_hi = {a: None for a in arms}, {}
    for _ in range(args.rounds):
        for arm in arms:
            dx.upload(zeros)
            t_lo, _ = timed_ms(lambda: run(arm, lo))
            dx.upload(zeros)
            t_hi, res = timed_ms(lambda: run(arm, hi))
            per = (t_hi - t_lo) / (hi - lo) * 1e3
            best[arm] = per if best[arm] is None else min(best[arm], per)
            res_hi[arm] = res
    lines = []
    for arm in arms:
        line = dict(workload=args.workload, arm=arm, c=args.c, shift=args.shift, storage="every entry", iters=[lo, hi], rounds=args.rounds,
                    multiplies_per_iter=LAUNCHES[arm][0], vector_kernels_per_iter=LAUNCHES[arm][1], us_per_iter=round(best[arm], 1),
                    ratio_to_bicgstab=round(best[arm] / best["bicgstab"], 3),
                    residual_at_hi=float(f"{res_hi[arm]:.3e}"), residual_is="relative" if arm == "bicgstab" else "rnorm")
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()


if __name__ == "__main__":
    main()
