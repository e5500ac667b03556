#!/usr/bin/env python3
"""Time per step of ehyb_gmres as a function of the step's index j, the multiply alone, and time to solution against
ehyb_bicgstab, on the unsymmetric audikw_1-like system of tools/bicgstab_time.py (same construction, same plan, plain storage,
Jacobi).

Per step.  One solve of max_iter = J < restart steps is one partial cycle: w = A x, start, J steps, the back substitution.  The
tool times such solves for rising J (--steps) at rtol = 0 with HIP events on its stream around the call (which ends in a
synchronise); the difference of two neighbouring J divided by their distance is the cost of a step at the j between them, and
one-off costs (workspace, the cycle start, solve_x's fixed part) cancel.  J stays below restart, so every timed solve is plain
launches: a full cycle would add the one-off capture of its graph to one side of a difference.  Every solve must run all its
J steps.  ortho_passes 1 and 2, --rounds rounds, the smallest figure kept.  Beside each figure the bytes the step's vector kernels move -- per pass
(j + 2) 8n read by dots and (j + 3) 8n by update, 3 * 8n by next -- and the rate that the time left after the multiply implies.

To solution.  ehyb_gmres(restart 30, both pass counts) and ehyb_bicgstab on the same plan to rtol 1e-10 from x = 0, arms
alternating, wall clock around the call, the smallest of --rounds kept; every answer's true residual is recomputed on the CPU.

usage: python tools/gmres_time.py [--workload audikw_1-like] [--c 0.3] [--shift 1e-2] [--restart 30] [--steps 1,2,4,8,12,16,20,24,29]
                                  [--rounds 3] [--out FILE]
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

from bicgstab_time import unsymmetric_system  # noqa: E402
from cg_multi_time import hip_events  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--c", type=float, default=0.3)
    ap.add_argument("--shift", type=float, default=1e-2)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--steps", default="1,2,4,8,12,16,20,24,29")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import scipy.sparse as sp

    import bench as B
    import ehyb_spmv_gpu_amd as E

    steps = [int(v) for v in args.steps.split(",")]
    assert steps == sorted(set(steps)) and 1 <= steps[0] and steps[-1] < args.restart <= 64
    hip = hip_events()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    st = E.Stream()

    def timed_us(fn):
        assert hip.hipEventRecord(ev0, st.ptr) == 0
        out = fn()
        assert hip.hipEventRecord(ev1, st.ptr) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return ms.value * 1e3, out

    gen, gargs, _ = B.WORKLOADS[args.workload]
    cfg = E.make_config(partitioner=B.partitioner_for(E, gen), sym_pairs=0)
    m, diag = unsymmetric_system(E, gen, gargs, cfg, args.c, args.shift)
    n = m.n
    A = sp.csr_matrix((m.V.copy(), (m.I.copy(), m.J.copy())), shape=(n, n))        # the permuted numbering, for the CPU checks
    plan = E.Plan(m, cfg)
    print(f"# {args.workload}, c = {args.c}: n={n} nnz={m.nnz} nnz_ell={plan.stats['nnz_ell']} nnz_er={plan.stats['nnz_er']}", flush=True)
    m.free()
    b = np.random.default_rng(1).uniform(-1, 1, n)
    inv = E.DeviceBuffer(n).upload(1.0 / diag)
    db, dx, dy = E.DeviceBuffer(n).upload(b), E.DeviceBuffer(n), E.DeviceBuffer(n)
    zeros = np.zeros(n)
    lib = E.host._lib.load()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    def gmres(passes, max_iter, rtol):
        done, rel = C.c_int(0), C.c_double(0)
        rc = lib.ehyb_gmres(plan.h, C.c_void_p(inv.ptr), C.c_void_p(db.ptr), C.c_void_p(dx.ptr), args.restart, passes, max_iter, rtol,
                            C.c_void_p(st.ptr), C.byref(done), C.byref(rel))
        assert rc == 0, lib.ehyb_last_error()
        return done.value, rel.value

    def bicgstab(max_iter, rtol):
        done, rel = C.c_int(0), C.c_double(0)
        rc = lib.ehyb_bicgstab(plan.h, C.c_void_p(inv.ptr), C.c_void_p(db.ptr), C.c_void_p(dx.ptr), max_iter, rtol, 10, C.c_void_p(st.ptr),
                               C.byref(done), C.byref(rel))
        assert rc == 0, lib.ehyb_last_error()
        return done.value, rel.value

    # the multiply alone: 50 multiplies, walks alternating, between two events
    def multiplies():
        for i in range(50):
            plan.spmv(db.ptr, dy.ptr, stream=st.ptr, walk=i & 1)
        assert lib.ehyb_stream_sync(C.c_void_p(st.ptr)) == 0

    multiplies()
    us_multiply = min(timed_us(multiplies)[0] for _ in range(args.rounds)) / 50
    emit(dict(workload=args.workload, kind="multiply", n=n, us=round(us_multiply, 1)))

    # per step
    best = {(p, J): None for p in (1, 2) for J in steps}
    for p in (1, 2):
        dx.upload(zeros)
        gmres(p, steps[-1], 0.0)                    # warm
    for _ in range(args.rounds):
        for p in (1, 2):
            for J in steps:
                dx.upload(zeros)
                us, (done, _) = timed_us(lambda: gmres(p, J, 0.0))
                assert done == J, (p, J, done)
                best[p, J] = us if best[p, J] is None else min(best[p, J], us)
    for p in (1, 2):
        for lo, hi in zip(steps[:-1], steps[1:]):
            per = (best[p, hi] - best[p, lo]) / (hi - lo)
            j_mid = (lo + hi - 1) / 2                # steps lo .. hi-1 (0-based) are the ones added
            vec_bytes = (p * (2 * j_mid + 5) + 3) * 8 * n
            emit(dict(workload=args.workload, kind="step", ortho_passes=p, restart=args.restart, steps=[lo, hi], j_mid=j_mid,
                      us_per_step=round(per, 1), us_multiply=round(us_multiply, 1), vector_MB=round(vec_bytes / 1e6, 1),
                      vector_GBps=round(vec_bytes / max(per - us_multiply, 1e-9) / 1e3, 1)))

    # to solution
    arms = {"gmres-2": lambda: gmres(2, 5000, 1e-10), "gmres-1": lambda: gmres(1, 5000, 1e-10), "bicgstab": lambda: bicgstab(5000, 1e-10)}
    wall, result = {a: None for a in arms}, {}
    for _ in range(args.rounds):
        for arm, fn in arms.items():
            dx.upload(zeros)
            t0 = time.perf_counter()
            done, rel = fn()
            ms = (time.perf_counter() - t0) * 1e3
            wall[arm] = ms if wall[arm] is None else min(wall[arm], ms)
            x = dx.download()
            true_rel = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
            assert rel <= 1e-10 and true_rel <= 1e-9, (arm, done, rel, true_rel)
            result[arm] = (done, rel, true_rel)
    for arm in arms:
        done, rel, true_rel = result[arm]
        mults = done * 2 if arm == "bicgstab" else done + -(-done // args.restart)
        emit(dict(workload=args.workload, kind="solve", arm=arm, rtol=1e-10, iterations=done, multiplies=mults, wall_ms=round(wall[arm], 2),
                  ratio_to_bicgstab=round(wall[arm] / wall["bicgstab"], 3), rel_residual=float(f"{rel:.3e}"), true_rel_residual=float(f"{true_rel:.3e}")))
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()


if __name__ == "__main__":
    main()
