#!/usr/bin/env python3
"""Time per iteration of ehyb_bicgstab against ehyb_pcg on the bench workload.

The system is the bench workload (audikw_1-like) made unsymmetric with the same pattern: every off-diagonal value above the
diagonal scaled by (1 + c), every one below by (1 - c) (--c, default 0.3), then the diagonal set to the row sum of |a_ij| plus
--shift times its mean -- strictly diagonally dominant, so nonsingular.  The system converges fast (relative residual far below
1e-40 after 60 iterations); rtol = 0 is what keeps both solves iterating, and the work per iteration does not depend on the
residual.  Plain storage.  The baseline is one ehyb_pcg iteration on the same construction at c = 0 (symmetric positive
definite) with the same configuration, so both plans have the same layout.  Both arms are Jacobi-preconditioned unless
--no-jacobi.

A figure is the difference of two solves at rtol = 0 (--iters lo,hi) divided by hi - lo, each solve timed with HIP events on the
tool's stream around a call that ends in a synchronise, so that one-off costs (workspace, capture, the first multiply) cancel.
Both solves must run all hi iterations (no early stop, no breakdown).  The arms alternate within the process, three rounds, and
the smallest figure per arm is kept.  One JSON line per arm.

usage: python tools/bicgstab_time.py [--workload audikw_1-like] [--c 0.3] [--iters 10,60] [--shift 1e-2] [--rounds 3]
                                     [--no-jacobi] [--out FILE]
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


def unsymmetric_system(E, gen, gargs, cfg, c, shift):
    """the workload generated with cfg, off-diagonals x (1 + c) above and x (1 - c) below the diagonal, diagonal = row sum of
    |a_ij| + shift * its mean; reordered.  -> (matrix, diagonal in the permuted numbering)"""
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    I, J, V = m.I, m.J, m.V
    V[I < J] *= 1.0 + c
    V[I > J] *= 1.0 - c
    off = np.bincount(I, weights=np.abs(V) * (I != J), minlength=m.n)
    V[I == J] = (off + shift * off.mean())[I[I == J]]
    m.reorder(cfg)
    I, J, V = m.I, m.J, m.V
    diag = np.zeros(m.n)
    diag[I[I == J]] = V[I == J]
    return m, diag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--c", type=float, default=0.3, help="off-diagonals x (1 + c) above, x (1 - c) below the diagonal")
    ap.add_argument("--iters", default="10,60")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-jacobi", action="store_true")
    ap.add_argument("--shift", type=float, default=1e-2,
                    help="diagonal = row sum of |a_ij| + shift * its mean (the timed solves run at rtol = 0 whatever the residual)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench as B
    import ehyb_spmv_gpu_amd as E

    lo, hi = [int(v) for v in args.iters.split(",")]
    jacobi = not args.no_jacobi
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
    cfg = E.make_config(partitioner=B.partitioner_for(E, gen), sym_pairs=0)
    plans = {}
    for arm, c in (("bicgstab", args.c), ("pcg", 0.0)):
        m, diag = unsymmetric_system(E, gen, gargs, cfg, c, args.shift)
        plan = E.Plan(m, cfg)
        st_ = plan.stats
        print(f"# {args.workload}, c = {c}: n={m.n} nnz={m.nnz} nnz_ell={st_['nnz_ell']} nnz_er={st_['nnz_er']} "
              f"sym_pairs={st_['sym_pairs']}", flush=True)
        plans[arm] = (plan, E.DeviceBuffer(m.n).upload(1.0 / diag) if jacobi else None)
        m.free()
    n = plans["pcg"][0].n
    assert plans["bicgstab"][0].n == n
    db = E.DeviceBuffer(n).upload(np.random.default_rng(1).uniform(-1, 1, n))
    dx = E.DeviceBuffer(n)
    zeros = np.zeros(n)
    lib = E.host._lib.load()

    def run(arm, it):
        plan, inv = plans[arm]
        fn = lib.ehyb_bicgstab if arm == "bicgstab" else lib.ehyb_pcg
        done, rel = C.c_int(0), C.c_double(0)
        rc = fn(plan.h, C.c_void_p(inv.ptr) if inv else None, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), it, 0.0, 10,
                C.c_void_p(st.ptr), C.byref(done), C.byref(rel))
        assert rc == 0, (arm, lib.ehyb_last_error())
        assert done.value == it, (arm, done.value, it)       # no early stop shortened the run
        return rel.value

    for arm in plans:
        dx.upload(zeros)
        run(arm, lo)                                 # warm
    best, rel_hi = {a: None for a in plans}, {}
    for _ in range(args.rounds):
        for arm in plans:
            dx.upload(zeros)
            t_lo, _ = timed_ms(lambda: run(arm, lo))
            dx.upload(zeros)
            t_hi, rel = timed_ms(lambda: run(arm, hi))
            per = (t_hi - t_lo) / (hi - lo) * 1e3
            best[arm] = per if best[arm] is None else min(best[arm], per)
            rel_hi[arm] = rel
    lines = []
    for arm in plans:
        line = dict(workload=args.workload, arm=arm, c=args.c if arm == "bicgstab" else 0.0, shift=args.shift, jacobi=jacobi,
                    storage="every entry", iters=[lo, hi], rounds=args.rounds, us_per_iter=round(best[arm], 1),
                    ratio_to_pcg=round(best[arm] / best["pcg"], 3), rel_residual_at_hi=float(f"{rel_hi[arm]:.3e}"))
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
