#!/usr/bin/env python3
"""Time per iteration of ehyb_minres against ehyb_bicgstab and ehyb_pcg on ONE plan of a symmetric indefinite bench workload.

The system is the workload itself (kkt3d-110: [H A^T; A 0]), a random right-hand side, and for every arm the same positive
diagonal 1 / |a_ii| (1 where a_ii = 0) unless --no-jacobi.  MINRES is the method for it; BiCGSTAB is the solver a caller had
before; CG is not a method on an indefinite matrix and is here for the cost of its iteration only.  rtol = 0 keeps every solve
iterating: the work per iteration does not depend on the residual.  One plan per storage -- every entry stored, and symmetric
pairs -- shared by the three solvers, at k = 1 .. --kmax right-hand sides (the *_multi entry points from k = 2).

A figure is the difference of two solves at rtol = 0 (--iters lo,hi) divided by hi - lo, each solve timed with HIP events on the
tool's stream around a call that ends in a synchronise, so that one-off costs (workspace, capture, the first multiply) cancel.
An arm whose solve does not run all its iterations (a breakdown, a non-finite residual that freezes a CG column) gets no figure
and says why.  The arms alternate within the process, --rounds rounds, and the smallest figure per arm is kept.  One JSON line
per (storage, k, arm).

usage: python tools/minres_time.py [--workload kkt3d-110] [--iters 10,60] [--rounds 3] [--kmax 4] [--no-jacobi] [--out FILE]
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

ARMS = {"minres": ("ehyb_minres", "ehyb_minres_multi"), "bicgstab": ("ehyb_bicgstab", "ehyb_bicgstab_multi"),
        "pcg": ("ehyb_pcg", "ehyb_pcg_multi")}
# launches per iteration and column group: multiplies, vector kernels
LAUNCHES = {"minres": (1, 3), "bicgstab": (2, 5), "pcg": (1, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="kkt3d-110")
    ap.add_argument("--iters", default="10,60")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kmax", type=int, default=4)
    ap.add_argument("--no-jacobi", action="store_true")
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
    lib = E.host._lib.load()

    def timed_ms(fn):
        assert hip.hipEventRecord(ev0, st.ptr) == 0
        out = fn()                                   # returns after its own stream synchronise
        assert hip.hipEventRecord(ev1, st.ptr) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return ms.value, out

    gen, gargs, _ = B.WORKLOADS[args.workload]
    assert gen in B.SYMMETRIC_GENERATORS, "MINRES needs a symmetric matrix"
    lines = []
    for sym, storage in ((0, "every entry"), (1, "symmetric pairs")):
        cfg = E.make_config(partitioner=B.partitioner_for(E, gen), sym_pairs=sym)
        m = E.Matrix.generate(gen, *gargs, cfg=cfg)
        m.reorder(cfg)
        I, J, V = m.I, m.J, m.V
        diag = np.zeros(m.n)
        diag[I[I == J]] = V[I == J]
        n = m.n
        plan = E.Plan(m, cfg)
        m.free()
        s = plan.stats
        print(f"# {args.workload}, {storage}: n={n} nnz_ell={s['nnz_ell']} nnz_er={s['nnz_er']} sym_pairs={s['sym_pairs']} "
              f"zero diagonal entries={int((diag == 0).sum())}", flush=True)
        inv = E.DeviceBuffer(n).upload(E.minres_inv_diag(diag)) if jacobi else None
        rng = np.random.default_rng(1)
        for k in range(1, args.kmax + 1):
            db = E.DeviceBuffer(k * n).upload(rng.uniform(-1, 1, k * n))
            dx = E.DeviceBuffer(k * n)
            zeros = np.zeros(k * n)

            def run(arm, it):
                """-> None if all `it` iterations ran in every column, else why not"""
                done, rel = (C.c_int * k)(), (C.c_double * k)()
                one, multi = ARMS[arm]
                head = (plan.h, C.c_void_p(inv.ptr) if inv else None)
                if k == 1:
                    rc = getattr(lib, one)(*head, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), it, 0.0, 10, C.c_void_p(st.ptr), done, rel)
                else:
                    rc = getattr(lib, multi)(*head, C.c_void_p(db.ptr), n, C.c_void_p(dx.ptr), n, k, it, 0.0, 10, C.c_void_p(st.ptr), done, rel)
                if rc != 0:
                    return lib.ehyb_last_error().decode()
                if list(done) != [it] * k:
                    return f"stopped after {list(done)} of {it} iterations, relative residuals {list(rel)}"
                return None

            best, why = {a: None for a in ARMS}, {a: None for a in ARMS}
            for arm in ARMS:
                dx.upload(zeros)
                why[arm] = run(arm, lo)              # warm
            for _ in range(args.rounds):
                for arm in ARMS:
                    if why[arm]:
                        continue
                    dx.upload(zeros)
                    t_lo, w_lo = timed_ms(lambda: run(arm, lo))
                    dx.upload(zeros)
                    t_hi, w_hi = timed_ms(lambda: run(arm, hi))
                    if w_lo or w_hi:
                        why[arm] = w_lo or w_hi
                        continue
                    per = (t_hi - t_lo) / (hi - lo) * 1e3
                    best[arm] = per if best[arm] is None else min(best[arm], per)
            for arm in ARMS:
                ok = best[arm] is not None and not why[arm]
                line = dict(workload=args.workload, storage=storage, k=k, arm=arm, jacobi=jacobi, iters=[lo, hi], rounds=args.rounds,
                            multiplies_per_iter=LAUNCHES[arm][0], vector_kernels_per_iter=LAUNCHES[arm][1],
                            us_per_iter=round(best[arm], 1) if ok else None,
                            ratio_to_bicgstab=round(best[arm] / best["bicgstab"], 3) if ok and best["bicgstab"] and not why["bicgstab"] else None)
                if why[arm]:
                    line["no_figure_because"] = why[arm][:300]
                print(json.dumps(line), flush=True)
                lines.append(line)
        plan.destroy()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()


if __name__ == "__main__":
    main()
