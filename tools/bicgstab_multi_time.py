#!/usr/bin/env python3
"""Time per iteration of k BiCGSTAB solves that share both multiplies (ehyb_bicgstab_multi) against one ehyb_bicgstab.

The system is that of tools/bicgstab_time.py: the bench workload (audikw_1-like) made unsymmetric on the same pattern (--c,
--shift), every entry stored, Jacobi unless --no-jacobi.  For k = 1..4 the k-column solve runs on a plan built with
lds_doubles = 20480 // k (one pass over the matrix serves k columns); the one-vector solve runs on the default plan.  Every
plan is built from a matrix generated and reordered with its own configuration, whose partitions are sized for its window
(as tools/cg_multi_time.py).

A figure is the difference of two solves at rtol = 0 (--iters lo,hi) divided by hi - lo, each solve timed with HIP events on the
tool's stream around a call that ends in a synchronise, so that one-off costs (workspace, capture, the first multiply) cancel.
Every column of both solves must run all hi iterations (no early stop, no breakdown).  The arms alternate within the process,
three rounds, and the smallest figure per arm is kept.  One JSON line per k.

usage: python tools/bicgstab_multi_time.py [--workload audikw_1-like] [--c 0.3] [--iters 10,60] [--shift 1e-2] [--rounds 3]
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

from bicgstab_time import unsymmetric_system  # noqa: E402
from cg_multi_time import LDS_MAX, hip_events  # noqa: E402


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

    def build(k):
        """the plan of the one-vector solve (k = None: the default window) or of a k-column one -> (plan, 1/diag on the device)"""
        kw = {} if k is None else {"lds_doubles": LDS_MAX // k}
        cfg = E.make_config(partitioner=B.partitioner_for(E, gen), sym_pairs=0, **kw)
        m, diag = unsymmetric_system(E, gen, gargs, cfg, args.c, args.shift)
        plan = E.Plan(m, cfg)
        if k is not None:
            assert plan.spmm_max_k >= k, (k, plan.spmm_max_k)
        print(f"# {args.workload}, c = {args.c}, {'default plan' if k is None else f'plan for k = {k}'}: n={m.n} nnz={m.nnz} "
              f"nnz_ell={plan.stats['nnz_ell']} nnz_er={plan.stats['nnz_er']} sym_pairs={plan.stats['sym_pairs']}", flush=True)
        inv = E.DeviceBuffer(m.n).upload(1.0 / diag) if jacobi else None
        m.free()
        return plan, inv

    single, inv1 = build(None)
    plans = {k: build(k) for k in (1, 2, 3, 4)}
    n = single.n
    Bm = np.random.default_rng(1).uniform(-1, 1, (4, n))
    db, dx = E.DeviceBuffer(4 * n).upload(Bm.ravel()), E.DeviceBuffer(4 * n)
    zeros = np.zeros(4 * n)
    lib = single.lib

    # both arms call the library on the tool's stream with device buffers uploaded before the first event
    def run_single(it):
        done, rel = C.c_int(0), C.c_double(0)
        rc = lib.ehyb_bicgstab(single.h, C.c_void_p(inv1.ptr) if inv1 else None, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), it, 0.0, 10,
                               C.c_void_p(st.ptr), C.byref(done), C.byref(rel))
        assert rc == 0, lib.ehyb_last_error()
        assert done.value == it, (done.value, it)            # no early stop shortened the run
        return [rel.value]

    def run_multi(k, it):
        done, rel = (C.c_int * k)(), (C.c_double * k)()
        plan, inv = plans[k]
        rc = lib.ehyb_bicgstab_multi(plan.h, C.c_void_p(inv.ptr) if inv else None, C.c_void_p(db.ptr), n, C.c_void_p(dx.ptr), n, k,
                                     it, 0.0, 10, C.c_void_p(st.ptr), done, rel)
        assert rc == 0, (k, lib.ehyb_last_error())
        assert list(done) == [it] * k, (k, list(done), it)
        return list(rel)

    arms = {"single": run_single}
    for k in plans:
        arms[f"k{k}"] = (lambda kk: (lambda it: run_multi(kk, it)))(k)
    for fn in arms.values():
        dx.upload(zeros)
        fn(lo)                                       # warm
    best, rel_hi = {a: None for a in arms}, {}
    for _ in range(args.rounds):
        for a, fn in arms.items():
            dx.upload(zeros)
            t_lo, _ = timed_ms(lambda: fn(lo))
            dx.upload(zeros)
            t_hi, rel = timed_ms(lambda: fn(hi))
            per = (t_hi - t_lo) / (hi - lo) * 1e3
            best[a] = per if best[a] is None else min(best[a], per)
            rel_hi[a] = rel
    lines = []
    for k in plans:
        multi = best[f"k{k}"]
        line = dict(workload=args.workload, c=args.c, shift=args.shift, jacobi=jacobi, storage="every entry", k=k,
                    lds_doubles=LDS_MAX // k, iters=[lo, hi], rounds=args.rounds, multi_us_per_iter=round(multi, 1),
                    multi_us_per_system=round(multi / k, 1), single_us_per_iter=round(best["single"], 1),
                    ratio_per_system=round(multi / k / best["single"], 3), speedup_per_system=round(best["single"] * k / multi, 3),
                    rel_residual_at_hi=[float(f"{r:.3e}") for r in rel_hi[f"k{k}"]])
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
