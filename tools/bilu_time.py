#!/usr/bin/env python3
"""ehyb_gmres_bilu and ehyb_bicgstab_bilu (GMRES and BiCGSTAB right-preconditioned with block ILU(0) solved in LDS) against
ehyb_gmres and ehyb_bicgstab with Jacobi on the bench workload made unsymmetric -- the system of tools/gmres_time.py: off-diagonals
x 1.3 above and x 0.7 below the diagonal, diagonal = row sum of |a_ij| + shift * mean, plain storage, a random b -- to a relative
residual of 1e-10.  Arms, alternating in one process, `rounds` rounds after one warm-up solve per arm, the smallest figure per arm
kept and the spread over the rounds beside it:

  gmres-jacobi, bicgstab-jacobi        ehyb_gmres(30) and ehyb_bicgstab with 1 / diag: the baselines, timed in the same run
  gmres-ORDER-ROWS, bicgstab-ORDER-ROWS  the *_bilu solvers, order in {stored, colour} x block_rows in {0, 256}

Per arm: iterations, microseconds per iteration (device time of the whole call between HIP events -- set-up, allocations and
check points included -- over the iterations), the device time to solution and the host's wall time.  Per BILU object: the host
set-up and the upload in seconds, blocks, the longest block, the workgroup size, levels, shifted and fallback blocks, the entries
of L and U, the bytes of the two streams, and the apply alone -- 200 launches back to back between HIP events -- beside the
multiply alone.  Every answer's true residual is recomputed on the CPU (reached: ||b - A x|| <= 2e-10 ||b|| and the reported
residual <= 1e-10).

usage: python tools/bilu_time.py [--workload audikw_1-like] [--rounds 3] [--shift 1.0] [--out profiles/bilu_time_audikw.jsonl]
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
NOT_MEASURED = ("the cost of a workgroup barrier by itself, the apply kernel's occupancy and stall reasons (no counters were collected), "
                "restart lengths other than 30, systems that are not diagonally dominant at this size")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shift", default="1.0", help="diagonal = row sum + shift * mean, one line of output per value: the smaller, the harder")
    ap.add_argument("--block-rows", default="0,256")
    ap.add_argument("--orders", default="stored,colour")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench as B
    import ehyb_spmv_gpu_amd as E

    if E.device_count() < 1:
        raise SystemExit("bilu_time: no HIP device visible (there is no CPU fallback)")
    lines = []
    for shift in args.shift.split(","):
        lines.append(measure(args, B, E, float(shift)))
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
    kw = dict(partitioner=B.partitioner_for(E, gen), sym_pairs=0)
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    I, J, V = m.I, m.J, m.V
    V[I < J] *= 1.3
    V[I > J] *= 0.7
    off = np.bincount(I, weights=np.abs(V) * (I != J), minlength=m.n)
    V[I == J] = (off + shift * off.mean())[I[I == J]]
    m.reorder(cfg)
    n = m.n
    A = sp.csr_matrix((m.V.copy(), m.J.copy(), m.row_idx.astype(np.int64)), shape=(n, n))
    lib = E.host._lib.load()
    print(f"shift {shift}: matrix of {n} rows reordered", file=sys.stderr, flush=True)
    plan = E.Plan(m, cfg)
    partitions = int(len(m.part_boundary) - 1)

    factors, setup = {}, {}
    for order in args.orders.split(","):
        for rows in (int(r) for r in args.block_rows.split(",")):
            name = f"{order}-{rows}"
            t0 = time.perf_counter()
            f = E.Bilu(m, block_rows=rows, order=order, upload=False)
            t1 = time.perf_counter()
            f.upload()
            t2 = time.perf_counter()
            nbytes, entries, threads = f.stream_info
            bp, lf, lb = f.array("block_ptr"), f.array("level_f"), f.array("level_b")
            per_block = np.maximum.reduceat(lf, bp[:-1]) + np.maximum.reduceat(lb, bp[:-1]) + 2        # forward + backward, per block
            factors[name] = f
            setup[name] = dict(create_host_s=round(t1 - t0, 3), upload_s=round(t2 - t1, 3), blocks=f.blocks, longest_block=int(np.diff(bp).max()),
                               threads=threads, max_k=f.max_k, most_levels=f.levels, mean_levels_per_block=round(float(per_block.mean()), 1),
                               shifted_blocks=f.shifted_blocks, fallback_blocks=f.fallback_blocks, nnz_l=int(len(f.array("l_cols"))),
                               nnz_u=int(len(f.array("u_cols"))), stream_entries=int(entries), stream_bytes=int(nbytes))
            print(f"shift {shift}: bilu {name} {setup[name]}", file=sys.stderr, flush=True)
    m.free()

    rng = np.random.default_rng(1)
    b = rng.uniform(-1, 1, n)
    nb = np.linalg.norm(b)
    db, dinv, dsol = E.DeviceBuffer(n).upload(b), E.DeviceBuffer(n).upload(1.0 / A.diagonal()), E.DeviceBuffer(n)
    zeros = np.zeros(n)
    vp = C.c_void_p

    def gmres(second, is_factor):
        def run():
            done, rel = C.c_int(0), C.c_double(0)
            fn = lib.ehyb_gmres_bilu if is_factor else lib.ehyb_gmres
            rc = fn(plan.h, second, vp(db.ptr), vp(dsol.ptr), 30, 2, 100000, TARGET, vp(st.ptr), C.byref(done), C.byref(rel))
            return rc, done.value, rel.value
        return run

    def bicgstab(second, is_factor):
        def run():
            done, rel = C.c_int(0), C.c_double(0)
            fn = lib.ehyb_bicgstab_bilu if is_factor else lib.ehyb_bicgstab
            rc = fn(plan.h, second, vp(db.ptr), vp(dsol.ptr), 100000, TARGET, 10, vp(st.ptr), C.byref(done), C.byref(rel))
            return rc, done.value, rel.value
        return run

    arms = {"gmres-jacobi": gmres(vp(dinv.ptr), False), "bicgstab-jacobi": bicgstab(vp(dinv.ptr), False)}
    for name, f in factors.items():
        arms[f"gmres-{name}"] = gmres(f.h, True)
        arms[f"bicgstab-{name}"] = bicgstab(f.h, True)
    dev_ms, wall_ms, info = {a: [] for a in arms}, {a: [] for a in arms}, {}
    for rnd in range(args.rounds + 1):      # round 0: the warm-up
        for a, fn in arms.items():
            dsol.upload(zeros)
            ms, wall, (rc, iters, rel) = timed(fn)
            assert rc == 0, (a, lib.ehyb_last_error())
            if rnd in (0, args.rounds):
                true = np.linalg.norm(b - A @ dsol.download()) / nb
                info[a] = dict(iterations=iters, rel_residual=float(f"{rel:.3e}"), recomputed=float(f"{true:.3e}"),
                               reached=bool(rel <= TARGET and true <= 2 * TARGET))
            print(f"shift {shift}: round {rnd} {a} {iters} iterations {ms:.2f} ms", file=sys.stderr, flush=True)
            if rnd:
                dev_ms[a].append(ms)
                wall_ms[a].append(wall)

    # the apply and the multiply alone: 200 launches each, back to back between the events
    dz = E.DeviceBuffer(n)

    def alone(call, reps=200):
        def burst(count):
            for _ in range(count):
                assert call() in (0, None), lib.ehyb_last_error()
        burst(10)
        return round(min(timed(lambda: burst(reps))[0] for _ in range(3)) * 1e3 / reps, 2)

    kernels = dict(multiply_us=alone(lambda: plan.spmv(db.ptr, dz.ptr, stream=st.ptr)))
    for name, f in factors.items():
        us = alone(lambda f=f: lib.ehyb_bilu_apply(f.h, vp(db.ptr), n, vp(dz.ptr), n, 1, vp(st.ptr)))
        setup[name]["apply_us"] = us
        setup[name]["us_per_level"] = round(us / setup[name]["mean_levels_per_block"], 3)

    def spread(v):
        return round((max(v) - min(v)) / min(v), 4)

    line = dict(workload=args.workload, storage="every entry", n=n, nnz=int(A.nnz), partitions=partitions, rounds=args.rounds, target=TARGET,
                shift=shift, restart=30, host_threads=E.host_threads(), kernels_alone=kernels, bilu=setup,
                arms={a: dict(us_per_iteration=round(min(dev_ms[a]) * 1e3 / max(1, info[a]["iterations"]), 1), device_ms=round(min(dev_ms[a]), 3),
                              wall_ms=round(min(wall_ms[a]), 3), spread=spread(wall_ms[a]), **info[a]) for a in arms},
                not_measured=NOT_MEASURED)
    print(json.dumps(line), flush=True)
    for f in factors.values():
        f.destroy()
    plan.destroy()
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()
    return line


if __name__ == "__main__":
    main()
