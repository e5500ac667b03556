#!/usr/bin/env python3
"""Time per iteration of k CG solves that share every multiply (ehyb_cg_multi) against k one-vector solves (ehyb_pcg), on the
bench workload made positive definite as in tools/cg_time.py -- the diagonal replaced by the row sum of |a_ij| plus a shift --
but with every off-diagonal value made negative and a small shift (--shift), so that the system is an M-matrix with the slowly
converging smooth modes of a mesh Laplacian.  tools/cg_time.py's system (off-diagonal signs as generated, shift 1) converges to
1e-6 in ten iterations and to the underflow in a hundred, so its per-iteration figures were taken on a converged system.

For each storage (symmetric pairs, every entry stored) and k = 1..4 the k-column solve runs on a plan built with
lds_doubles = 20480 // k (one pass over the matrix serves k columns); the one-vector solve runs on the default plan.  Every plan
is built from a matrix reordered with its own configuration, whose partitions are sized for its window.  A figure is
the difference of two solves at rtol = 0 (--iters lo,hi) divided by hi - lo, each solve timed with HIP events on its stream
around a call that ends in a synchronise, so that one-off costs (workspace, capture, the first multiply) cancel.  The relative
residual after hi iterations must still be above 1e-8 in every column, or the system converged inside the run.  The arms
alternate within the process, three rounds, and the smallest figure per arm is kept.  One JSON line per (storage, k).

usage: python tools/cg_multi_time.py [--workload audikw_1-like] [--iters 10,60] [--shift 1e-2] [--rounds 3] [--jacobi] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LDS_MAX = 20480


def hip_events():
    hip = C.CDLL("libamdhip64.so")
    for f in ("hipEventCreate", "hipEventRecord", "hipEventSynchronize", "hipEventElapsedTime", "hipEventDestroy"):
        getattr(hip, f).restype = C.c_int
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    return hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--iters", default="10,60")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--jacobi", action="store_true")
    ap.add_argument("--shift", type=float, default=1e-2,
                    help="diagonal = row sum of |a_ij| + shift * its mean: small enough that --iters does not converge")
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
    lines = []
    for sym in (1, 0):
        storage = "symmetric pairs" if sym else "every entry"

        def build(k):
            """the plan of the one-vector solve (k = None: the default window) or of a k-column one (lds_doubles = 20480 // k):
            the matrix is generated and reordered with the plan's own configuration, as tools/spmm_time.py does -- the
            partitions are sized for the window -- and -> (plan, 1/diag on the device or None)"""
            kw = {} if k is None else {"lds_doubles": LDS_MAX // k}
            cfg = E.make_config(partitioner=B.partitioner_for(E, gen), sym_pairs=sym, **kw)
            m = E.Matrix.generate(gen, *gargs, cfg=cfg)
            I, J, V = m.I, m.J, m.V
            V[I != J] = -np.abs(V[I != J])
            off = np.bincount(I, weights=np.abs(V) * (I != J), minlength=m.n)
            V[I == J] = (off + args.shift * off.mean())[I[I == J]]      # strictly diagonally dominant, still symmetric
            m.reorder(cfg)
            I, J, V = m.I, m.J, m.V
            diag = np.zeros(m.n)
            diag[I[I == J]] = V[I == J]
            plan = E.Plan(m, cfg)
            if k is not None:
                assert plan.spmm_max_k >= k, (k, plan.spmm_max_k)
            print(f"# {args.workload}, {storage}, {'default plan' if k is None else f'plan for k = {k}'}: n={m.n} nnz={m.nnz} "
                  f"sym_pairs={plan.stats['sym_pairs']} nnz_er={plan.stats['nnz_er']}", flush=True)
            inv = E.DeviceBuffer(m.n).upload(1.0 / diag) if args.jacobi else None
            m.free()
            return plan, inv

        single, inv1 = build(None)
        plans = {k: build(k) for k in (1, 2, 3, 4)}
        n = single.n
        rng = np.random.default_rng(1)
        Bm = rng.uniform(-1, 1, (4, n))             # (not ones: with these row sums a constant vector is an eigenvector)
        db, dx = E.DeviceBuffer(4 * n).upload(Bm.ravel()), E.DeviceBuffer(4 * n)
        zeros = np.zeros(4 * n)
        lib = single.lib

        # both arms call the library on the tool's stream with device buffers uploaded before the first event
        def run_single(it):
            done, rel = C.c_int(0), C.c_double(0)
            assert lib.ehyb_pcg(single.h, C.c_void_p(inv1.ptr) if inv1 else None, C.c_void_p(db.ptr + 8 * n), C.c_void_p(dx.ptr),
                                it, 0.0, 10, C.c_void_p(st.ptr), C.byref(done), C.byref(rel)) == 0
            assert done.value == it
            return np.array([rel.value])

        def run_multi(k, it):
            done, rel = (C.c_int * k)(), (C.c_double * k)()
            plan, inv = plans[k]
            assert lib.ehyb_pcg_multi(plan.h, C.c_void_p(inv.ptr) if inv else None, C.c_void_p(db.ptr), n, C.c_void_p(dx.ptr), n, k,
                                      it, 0.0, 10, C.c_void_p(st.ptr), done, rel) == 0
            assert list(done) == [it] * k
            return np.array(list(rel))

        arms = {"single": lambda it: run_single(it)}
        for k in plans:
            arms[f"k{k}"] = (lambda kk: (lambda it: run_multi(kk, it)))(k)
        for fn in arms.values():
            dx.upload(zeros)
            fn(lo)                                   # warm
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
        for a, rel in rel_hi.items():
            assert (rel > 1e-8).all(), f"{storage} {a}: converged inside the run (relative residual {rel}); use fewer --iters"
        for k in plans:
            multi = best[f"k{k}"]
            line = dict(workload=args.workload, storage=storage, k=k, lds_doubles=LDS_MAX // k, jacobi=bool(args.jacobi),
                        iters=[lo, hi], rounds=args.rounds, multi_us_per_iter=round(multi, 1),
                        multi_us_per_system=round(multi / k, 1), single_us_per_iter=round(best["single"], 1),
                        speedup_per_system=round(best["single"] * k / multi, 3),
                        rel_residual_at_hi=[float(f"{r:.3e}") for r in rel_hi[f"k{k}"]])
            print(json.dumps(line), flush=True)
            lines.append(line)
        del single, inv1, plans, db, dx
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()


if __name__ == "__main__":
    main()
