#!/usr/bin/env python3
"""ehyb_pcg_fsai (CG with a factorised sparse approximate inverse) against ehyb_pcg and ehyb_pcg_coarse on the bench workload's
SPD system -- the M-matrix of tools/pcg_coarse_time.py (off-diagonals negative, diagonal = row sum + shift * mean), a random b
-- to a relative residual of 1e-10.  Arms, alternating in one process, `rounds` rounds after one warm-up solve per arm, the
smallest figure per arm kept and the spread over the rounds beside it:

  pcg               ehyb_pcg with Jacobi scaling: the baseline, timed in the same run
  coarse            ehyb_pcg_coarse, the default map (--dof 3)
  fsai              ehyb_pcg_fsai, G and G^T on plans of their own, fp64 values
  fsai-f32          the same with cfg.val_f32 = 1 for G's plans
  fsai-spmv_t       one plan of G, G^T through ehyb_spmv_t

Per arm: iterations, microseconds per iteration (device time of the whole call between HIP events -- set-up, allocations and
check points included -- over the iterations), the device time to solution and the host's wall time of the whole call.  For the
preconditioner: the host set-up (pattern, values and plans: ehyb_fsai_create_host), the upload, the numeric phase repeated on
the device (ehyb_fsai_set_values on device arrays), and the bytes a multiply with G's plans moves against A's.  Every answer is
checked on the CPU (reached: ||b - A x|| <= 2e-10 ||b|| and the reported residual <= 1e-10).

usage: python tools/pcg_fsai_time.py [--workload audikw_1-like] [--rounds 3] [--shift 1e-2,1e-4] [--out profiles/pcg_fsai_time_audikw.jsonl]
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
    ap.add_argument("--sym", type=int, default=1, help="1: symmetric pair storage for A (the bench default for this workload), 0: every entry")
    ap.add_argument("--row-cap", type=int, default=0)
    ap.add_argument("--dof", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench as B
    import ehyb_spmv_gpu_amd as E

    if E.device_count() < 1:
        raise SystemExit("pcg_fsai_time: no HIP device visible (there is no CPU fallback)")
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
    a_stats = plan.stats

    co = E.Coarse(m, dof=args.dof)

    # the three FSAI objects: host set-up and upload timed apart
    def build(transpose, **over):
        t0 = time.perf_counter()
        f = E.Fsai(m, row_cap=args.row_cap, cfg=E.make_config(**{**kw, **over}), transpose=transpose, upload=False)
        t1 = time.perf_counter()
        f.upload()
        t2 = time.perf_counter()
        plans = [p for p in f.plans if p is not None]
        stats = [p.stats for p in plans]
        info = dict(create_host_ms=round((t1 - t0) * 1e3, 1), upload_ms=round((t2 - t1) * 1e3, 1), plans=len(plans),
                    nnz_g=int(stats[0]["nnz"]), bytes_format=[int(s["bytes_format"]) for s in stats],
                    value_bytes=[int(sum(p.device_value_bytes)) for p in plans], capped_rows=f.capped_rows, fallback_rows=f.fallback_rows,
                    max_row=int(np.diff(f.array("row_ptr")).max()))
        return f, info

    fsais, setup = {}, {}
    for name, transpose, over in (("fsai", "plan", {}), ("fsai-f32", "plan", dict(val_f32=1)), ("fsai-spmv_t", "spmv_t", {})):
        fsais[name], setup[name] = build(transpose, **over)

    # the numeric phase on the device, values already there: the factor kernel, its counters' read-back, the fills of the plans
    dV = E.DeviceBuffer(len(m.V)).upload(m.V)
    for name, f in fsais.items():
        f.set_values((dV.ptr, len(m.V)), stream=st.ptr)
        runs = [timed(lambda: f.set_values((dV.ptr, len(m.V)), stream=st.ptr)) for _ in range(3)]
        setup[name]["refactor_device_ms"] = round(min(r[0] for r in runs), 3)
        setup[name]["refactor_wall_ms"] = round(min(r[1] for r in runs), 3)
        setup[name]["fallback_rows_device"] = f.fallback_rows
    dV.free()
    m.free()

    rng = np.random.default_rng(1)
    b = rng.uniform(-1, 1, n)
    nb = np.linalg.norm(b)
    db, dinv, dsol = E.DeviceBuffer(n).upload(b), E.DeviceBuffer(n).upload(1.0 / A.diagonal()), E.DeviceBuffer(n)
    zeros = np.zeros(n)
    vp = C.c_void_p

    def pcg():
        done, rel = C.c_int(0), C.c_double(0)
        rc = lib.ehyb_pcg(plan.h, vp(dinv.ptr), vp(db.ptr), vp(dsol.ptr), 100000, TARGET, 10, vp(st.ptr), C.byref(done), C.byref(rel))
        return rc, done.value, rel.value

    def coarse():
        done, rel = C.c_int(0), C.c_double(0)
        rc = lib.ehyb_pcg_coarse(plan.h, co.h, vp(dinv.ptr), vp(db.ptr), vp(dsol.ptr), 100000, TARGET, 10, vp(st.ptr), C.byref(done), C.byref(rel))
        return rc, done.value, rel.value

    def fsai(f):
        def run():
            done, rel = C.c_int(0), C.c_double(0)
            rc = lib.ehyb_pcg_fsai(plan.h, f.h, vp(db.ptr), vp(dsol.ptr), 100000, TARGET, 10, vp(st.ptr), C.byref(done), C.byref(rel))
            return rc, done.value, rel.value
        return run

    arms = {"pcg": pcg, "coarse": coarse, **{name: fsai(f) for name, f in fsais.items()}}
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

    # the apply and the multiply alone: 200 launches each, back to back between the events
    dz = E.DeviceBuffer(n)

    def alone(call, reps=200):
        def burst(count):
            for _ in range(count):
                assert call() in (0, None), lib.ehyb_last_error()
        burst(10)
        return round(min(timed(lambda: burst(reps))[0] for _ in range(3)) * 1e3 / reps, 2)

    kernels = dict(multiply_us=alone(lambda: plan.spmv(db.ptr, dz.ptr, stream=st.ptr)),
                   **{f"apply_{name}_us": alone(lambda f=f: lib.ehyb_fsai_apply(f.h, vp(db.ptr), vp(dz.ptr), vp(st.ptr))) for name, f in fsais.items()})

    def spread(v):
        return round((max(v) - min(v)) / min(v), 4)

    line = dict(workload=args.workload, storage="symmetric pairs" if args.sym else "every entry", n=n, nnz=int(A.nnz), rounds=args.rounds,
                target=TARGET, shift=shift, host_threads=E.host_threads(), kernels_alone=kernels,
                a_plan=dict(bytes_format=int(a_stats["bytes_format"]), value_bytes=int(sum(plan.device_value_bytes))), fsai=setup,
                arms={a: dict(us_per_iteration=round(min(dev_ms[a]) * 1e3 / max(1, info[a]["iterations"]), 1), device_ms=round(min(dev_ms[a]), 3),
                              wall_ms=round(min(wall_ms[a]), 3), spread=spread(wall_ms[a]), **info[a]) for a in arms})
    print(json.dumps(line), flush=True)
    for f in fsais.values():
        f.destroy()
    co.destroy()
    plan.destroy()
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()
    return line


if __name__ == "__main__":
    main()
