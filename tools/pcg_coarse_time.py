#!/usr/bin/env python3
"""ehyb_pcg_coarse (two-level PCG with an aggregate coarse space) against ehyb_pcg and ehyb_pcg_cheb of degree 4 on the bench
workload's SPD system -- the M-matrix of tools/pcg_cheb_time.py (off-diagonals negative, diagonal = row sum + shift * mean),
Jacobi scaling, a random b -- to a relative residual of 1e-10.  Arms, alternating in one process, `rounds` rounds after one
warm-up solve per arm, the smallest figure per arm kept and the spread over the rounds beside it:

  pcg               ehyb_pcg
  coarse            ehyb_pcg_coarse, the default map (--agg-rows 0, --dof 3: one constant per component and aggregate)
  cheb-4            ehyb_pcg_cheb of degree 4, the polynomial on the plan itself, lmax = 1.1 * ehyb_lambda_max (estimated outside
                    the timed window)
  coarse-vec        with --vectors modes:N: ehyb_pcg_coarse with a coarse space from vectors (ehyb_coarse_create_host_vecs) -- the
                    dof per-component constants and the N lowest modes of the matrix from Plan.lobpcg (preconditioned with the
                    `coarse` arm's object, on a plan of its own with every entry stored; its wall time is recorded, outside every
                    timed window), on the default aggregates of Coarse.from_vectors

Per arm: iterations, microseconds per iteration (device time of the whole call between HIP events -- set-up, allocations and
check points included -- over the iterations) and the host's wall time of the whole call.  The host set-up of the coarse space
is timed apart: the map, and E with its factorisation and inverse (one call).  With --vectors the two weighted kernels are
launched alone as well and set against their byte counts (restrict: ROWS, r and W, (12 + 8 nv) n bytes; prolong: agg, W, r,
inv_diag and z, (28 + 8 nv) n bytes).  Every answer is checked on the CPU
(reached: ||b - A x|| <= 2e-10 ||b|| and the reported residual <= 1e-10).

usage: python tools/pcg_coarse_time.py [--workload audikw_1-like] [--rounds 3] [--shift 1e-2,1e-4] [--out profiles/pcg_coarse_time_audikw.jsonl]
       python tools/pcg_coarse_time.py --vectors modes:3 --out profiles/pcg_coarse_vec_time_audikw.jsonl
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shift", default="1e-2,1e-4", help="diagonal = row sum + shift * mean, one line of output per value: the smaller, the harder")
    ap.add_argument("--sym", type=int, default=1, help="1: symmetric pair storage (the bench default for this workload), 0: every entry")
    ap.add_argument("--agg-rows", type=int, default=0)
    ap.add_argument("--dof", type=int, default=3)
    ap.add_argument("--vectors", default=None, help="modes:N -- a further arm with the dof constants and the N lowest modes as a vector coarse space")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench as B
    import ehyb_spmv_gpu_amd as E

    if E.device_count() < 1:
        raise SystemExit("pcg_coarse_time: no HIP device visible (there is no CPU fallback)")
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
    plan = E.Plan(m, cfg)

    # the coarse space: host set-up timed call by call, then the upload
    cmap, nc = np.empty(n, dtype=np.int32), C.c_int(0)
    t0 = time.perf_counter()
    rc = lib.ehyb_coarse_map(C.byref(m.c), args.agg_rows, args.dof, cmap.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nc))
    t1 = time.perf_counter()
    assert rc == 0, lib.ehyb_last_error()
    co = E.Coarse(m, map=cmap, upload=False)
    t2 = time.perf_counter()
    co.upload()
    t3 = time.perf_counter()
    rows = np.bincount(cmap, minlength=nc.value)
    setup = dict(nc=nc.value, agg_rows=args.agg_rows, dof=args.dof, partitions=len(m.part_boundary) - 1, rows_per_unknown_min=int(rows.min()),
                 rows_per_unknown_max=int(rows.max()), einv_bytes=8 * nc.value ** 2, host_threads=E.host_threads(),
                 map_ms=round((t1 - t0) * 1e3, 2), e_factor_inverse_ms=round((t2 - t1) * 1e3, 2), upload_ms=round((t3 - t2) * 1e3, 2))
    covec, vectors = None, None
    if args.vectors:
        kind, _, count = args.vectors.partition(":")
        assert kind == "modes" and 0 <= int(count) <= 8 - args.dof, "--vectors modes:N with dof + N <= 8"
        covec, vectors = vector_object(args, B, E, m, plan, co, A, int(count))
    m.free()

    rng = np.random.default_rng(1)
    b = rng.uniform(-1, 1, n)
    nb = np.linalg.norm(b)
    db, dinv, dsol = E.DeviceBuffer(n).upload(b), E.DeviceBuffer(n).upload(1.0 / A.diagonal()), E.DeviceBuffer(n)
    zeros = np.zeros(n)
    vp = C.c_void_p

    lam = C.c_double(0)
    assert lib.ehyb_lambda_max(plan.h, vp(dinv.ptr), 20, vp(st.ptr), C.byref(lam)) == 0, lib.ehyb_last_error()
    lmax = 1.1 * lam.value

    def pcg():
        done, rel = C.c_int(0), C.c_double(0)
        rc = lib.ehyb_pcg(plan.h, vp(dinv.ptr), vp(db.ptr), vp(dsol.ptr), 100000, TARGET, 10, vp(st.ptr), C.byref(done), C.byref(rel))
        return rc, done.value, rel.value

    def coarse():
        done, rel = C.c_int(0), C.c_double(0)
        rc = lib.ehyb_pcg_coarse(plan.h, co.h, vp(dinv.ptr), vp(db.ptr), vp(dsol.ptr), 100000, TARGET, 10, vp(st.ptr), C.byref(done), C.byref(rel))
        return rc, done.value, rel.value

    def cheb():
        done, rel = C.c_int(0), C.c_double(0)
        rc = lib.ehyb_pcg_cheb(plan.h, plan.h, vp(dinv.ptr), vp(db.ptr), vp(dsol.ptr), 4, 0.0, lmax, 100000, TARGET, 10, vp(st.ptr),
                               C.byref(done), C.byref(rel))
        return rc, done.value, rel.value

    def coarse_vec():
        done, rel = C.c_int(0), C.c_double(0)
        rc = lib.ehyb_pcg_coarse(plan.h, covec.h, vp(dinv.ptr), vp(db.ptr), vp(dsol.ptr), 100000, TARGET, 10, vp(st.ptr), C.byref(done), C.byref(rel))
        return rc, done.value, rel.value

    arms = {"pcg": pcg, "coarse": coarse, "cheb-4": cheb}
    if covec is not None:
        arms["coarse-vec"] = coarse_vec
    dev_ms, wall_ms, info = {a: [] for a in arms}, {a: [] for a in arms}, {}
    for rnd in range(args.rounds + 1):      # round 0: the warm-up
        for a, fn in arms.items():
            dsol.upload(zeros)
            ms, wall, (rc, iters, rel) = timed(fn)
            assert rc == 0, (a, lib.ehyb_last_error())
            true = np.linalg.norm(b - A @ dsol.download()) / nb
            if rnd:
                dev_ms[a].append(ms)
                wall_ms[a].append(wall)
            info[a] = dict(iterations=iters, rel_residual=float(f"{rel:.3e}"), recomputed=float(f"{true:.3e}"),
                           reached=bool(rel <= TARGET and true <= 2 * TARGET))

    # the three kernels and the multiply alone: 200 launches each, back to back between the events (K = 1, the step calls' grids)
    dt, dc, dz, ds = E.DeviceBuffer(nc.value), E.DeviceBuffer(nc.value), E.DeviceBuffer(n), E.DeviceBuffer(5 * 1024)

    def alone(call, reps=200):
        def burst(count):
            for _ in range(count):
                assert call() in (0, None), lib.ehyb_last_error()
        burst(10)
        return round(min(timed(lambda: burst(reps))[0] for _ in range(3)) * 1e3 / reps, 2)

    kernels = dict(
        restrict_us=alone(lambda: lib.ehyb_coarse_restrict_step(co.h, vp(db.ptr), vp(dt.ptr), vp(st.ptr))),
        solve_us=alone(lambda: lib.ehyb_coarse_solve_step(co.h, vp(dt.ptr), vp(dc.ptr), vp(st.ptr))),
        prolong_us=alone(lambda: lib.ehyb_coarse_prolong_step(co.h, vp(db.ptr), vp(dinv.ptr), vp(dc.ptr), vp(dz.ptr), vp(ds.ptr), 0, vp(st.ptr))),
        multiply_us=alone(lambda: plan.spmv(db.ptr, dz.ptr, stream=st.ptr)))

    if covec is not None:
        dtv, dcv, nv = E.DeviceBuffer(covec.nc), E.DeviceBuffer(covec.nc).upload(np.zeros(covec.nc)), covec.nv
        r_us = alone(lambda: lib.ehyb_coarse_restrict_step(covec.h, vp(db.ptr), vp(dtv.ptr), vp(st.ptr)))
        p_us = alone(lambda: lib.ehyb_coarse_prolong_step(covec.h, vp(db.ptr), vp(dinv.ptr), vp(dcv.ptr), vp(dz.ptr), vp(ds.ptr), 0, vp(st.ptr)))
        r_bytes, p_bytes = (12 + 8 * nv) * n, (28 + 8 * nv) * n
        vectors["kernels_alone"] = dict(restrict_vec_us=r_us, restrict_vec_bytes=r_bytes, restrict_vec_GBps=round(r_bytes / r_us / 1e3, 1),
                                        prolong_vec_us=p_us, prolong_vec_bytes=p_bytes, prolong_vec_GBps=round(p_bytes / p_us / 1e3, 1),
                                        solve_us=alone(lambda: lib.ehyb_coarse_solve_step(covec.h, vp(dtv.ptr), vp(dcv.ptr), vp(st.ptr))))
        vectors["not_measured"] = "the multiply's time inside the coarse-vec solve; the split of the per-iteration difference"

    def spread(v):
        return round((max(v) - min(v)) / min(v), 4)

    line = dict(kernels_alone=kernels,workload=args.workload, storage="symmetric pairs" if args.sym else "every entry", n=n, nnz=int(A.nnz), rounds=args.rounds,
                target=TARGET, shift=shift, coarse=setup, lmax=lmax, **({"vectors": vectors} if vectors else {}),
                arms={a: dict(us_per_iteration=round(min(dev_ms[a]) * 1e3 / max(1, info[a]["iterations"]), 1), device_ms=round(min(dev_ms[a]), 3),
                              wall_ms=round(min(wall_ms[a]), 3), spread=spread(wall_ms[a]), **info[a]) for a in arms})
    print(json.dumps(line), flush=True)
    if covec is not None:
        line["vectors"]["us_per_iteration_over_coarse"] = round(line["arms"]["coarse-vec"]["us_per_iteration"] - line["arms"]["coarse"]["us_per_iteration"], 1)
        covec.destroy()
    co.destroy()
    plan.destroy()
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()
    return line


def vector_object(args, B, E, m, plan, co, A, modes):
    """-> (the uploaded vector object, what was done): B = the dof per-component constants (old index mod dof) and the `modes`
    lowest eigenvectors of A, from Plan.lobpcg on a plan with every entry stored, preconditioned with the plain object"""
    n, dof = m.n, args.dof
    comp = np.empty(n, dtype=np.int64)
    comp[m.reorder_list] = np.arange(n) % dof                  # reorder_list[old] = new
    vecs = [(comp == c).astype(np.float64) for c in range(dof)]
    info = dict(kind=args.vectors, constants=dof, modes=modes)
    if modes:
        mode_plan = E.Plan(m, E.make_config(partitioner=B.partitioner_for(E, B.WORKLOADS[args.workload][0]), sym_pairs=0, lds_doubles=20480 // 4))
        t0 = time.perf_counter()
        evals, X, out = mode_plan.lobpcg(modes, coarse=co, inv_diag=1.0 / A.diagonal(), tol=1e-6, max_iter=500)
        info.update(lobpcg_wall_ms=round((time.perf_counter() - t0) * 1e3, 1), lobpcg_iters=out["iters"], lobpcg_nconv=out["nconv"],
                    lobpcg_tol=1e-6, evals=[float(f"{v:.6e}") for v in evals])
        mode_plan.destroy()
        vecs += list(X)
    t0 = time.perf_counter()
    covec = E.Coarse.from_vectors(m, np.stack(vecs), upload=False)
    t1 = time.perf_counter()
    covec.upload()
    t2 = time.perf_counter()
    kept = np.diff(covec.array("off"))
    rows = np.bincount(covec.array("map"), minlength=covec.nagg)
    info.update(nv=covec.nv, nagg=covec.nagg, nc=covec.nc, kept_min=int(kept.min()), kept_max=int(kept.max()), rows_per_aggregate_min=int(rows.min()),
                rows_per_aggregate_max=int(rows.max()), w_bytes=8 * n * covec.nv, einv_bytes=8 * covec.nc ** 2,
                map_bases_e_factor_inverse_ms=round((t1 - t0) * 1e3, 2), upload_ms=round((t2 - t1) * 1e3, 2))
    return covec, info


if __name__ == "__main__":
    main()
