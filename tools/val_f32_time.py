#!/usr/bin/env python3
"""cfg.val_f32 (the device holds the value streams in fp32) against the fp64 plan of the same reordered matrix, on the bench
workload in both storages (symmetric pairs, every entry stored).  Three figures per storage, the arms alternating in one process,
three rounds, the smallest figure per arm kept and the spread over the rounds beside it:

  multiply   a captured graph of 20 multiplies (ehyb_spmv_graph_create) replayed between HIP events, microseconds per multiply,
             with ehyb_plan_device_value_bytes and the bytes of the whole window launch beside each arm.  After the loop every
             arm's y is compared on the CPU with the product of the values its plan holds (fp64, or rounded through float32):
             within 1e-12 * sum |a_ij x_j| per row.
  pcg        ehyb_pcg per iteration on both plans, on the M-matrix system of tools/cg_multi_time.py (off-diagonals negative,
             diagonal = row sum + shift * mean), Jacobi, rtol = 0: a 60- minus a 10-iteration solve.  After the loop the
             residual each solve reports is checked against b - A x computed on the CPU with its plan's values.
  solve      wall time to a relative residual of 1e-10: ehyb_pcg on the fp64 plan against ehyb_pcg_refine (fp64 plan outside,
             val_f32 plan inside, inner rtol 1e-5); the answer of each is checked on the CPU against the fp64 matrix.

usage: python tools/val_f32_time.py [--workload audikw_1-like] [--rounds 3] [--shift 1e-2] [--out profiles/val_f32_time_audikw.jsonl]
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

LOOP = 20


def f32(v):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return v.astype(np.float32).astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shift", type=float, default=1e-2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench as B
    import ehyb_spmv_gpu_amd as E

    hip = hip_events()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    st = E.Stream()

    def timed_ms(fn):
        assert hip.hipEventRecord(ev0, st.ptr) == 0
        out = fn()
        assert hip.hipEventRecord(ev1, st.ptr) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev0, ev1) == 0
        return ms.value, out

    gen, gargs, _ = B.WORKLOADS[args.workload]
    lines = []
    for sym in (1, 0):
        storage = "symmetric pairs" if sym else "every entry"
        kw = dict(partitioner=B.partitioner_for(E, gen), sym_pairs=sym)
        cfgs = {"fp64": E.make_config(**kw), "val_f32": E.make_config(val_f32=1, **kw)}
        m = E.Matrix.generate(gen, *gargs, cfg=cfgs["fp64"])
        I, J, V = m.I, m.J, m.V
        V[I != J] = -np.abs(V[I != J])
        off = np.bincount(I, weights=np.abs(V) * (I != J), minlength=m.n)
        V[I == J] = (off + args.shift * off.mean())[I[I == J]]          # the M-matrix of tools/cg_multi_time.py
        m.reorder(cfgs["fp64"])
        n = m.n
        A = {"fp64": sp.csr_matrix((m.V.copy(), m.J.copy(), m.row_idx.astype(np.int64)), shape=(n, n))}
        A["fp64"].sort_indices()                                         # (now: scipy sorts in place later, under arrays another matrix shares)
        A["val_f32"] = sp.csr_matrix((f32(A["fp64"].data), A["fp64"].indices.copy(), A["fp64"].indptr.copy()), shape=(n, n))
        absA = abs(A["fp64"])
        plans = {a: E.Plan(m, cfgs[a]) for a in cfgs}
        m.free()
        lib = plans["fp64"].lib
        rng = np.random.default_rng(1)
        x, b = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
        nb = np.linalg.norm(b)
        dx, dy, db = E.DeviceBuffer(n).upload(x), {a: E.DeviceBuffer(n) for a in plans}, E.DeviceBuffer(n).upload(b)
        dinv = E.DeviceBuffer(n).upload(1.0 / A["fp64"].diagonal())
        dsol = E.DeviceBuffer(n)
        zeros = np.zeros(n)

        def stats_of(arm):
            p = plans[arm]
            s = p.stats
            ell, er = p.device_value_bytes
            launch = s["bytes_format_ell"] - 8 * (s["size_block_ell"] + s["er_inline"]) + ell
            return dict(value_bytes_ell=ell, value_bytes_er=er, window_launch_bytes=launch, resident_bytes=p.resident_bytes)

        def spread(v):
            return round((max(v) - min(v)) / min(v), 4)

        # ---- multiply
        graphs = {a: plans[a].graph(dx.ptr, dy[a].ptr, LOOP) for a in plans}
        for a in plans:
            for _ in range(3):
                graphs[a].launch(st.ptr)
        st.sync()
        mult = {a: [] for a in plans}
        for _ in range(args.rounds):
            for a in plans:
                ms, _ = timed_ms(lambda: [graphs[a].launch(st.ptr) for _ in range(5)])
                mult[a].append(ms * 1e3 / (5 * LOOP))
        scale = absA @ np.abs(x)
        for a in plans:
            err = np.max(np.abs(dy[a].download() - A[a] @ x) / scale)
            assert err <= 1e-12, (storage, a, err)
            graphs[a].destroy()
        # ---- pcg per iteration
        lo, hi = 10, 60

        def pcg(arm, it, rtol=0.0):
            done, rel = C.c_int(0), C.c_double(0)
            dsol.upload(zeros)
            t0 = time.perf_counter()
            ms, _ = timed_ms(lambda: lib.ehyb_pcg(plans[arm].h, C.c_void_p(dinv.ptr), C.c_void_p(db.ptr), C.c_void_p(dsol.ptr), it, rtol, 10,
                                                   C.c_void_p(st.ptr), C.byref(done), C.byref(rel)))
            return ms, (time.perf_counter() - t0) * 1e3, done.value, rel.value

        for a in plans:
            pcg(a, lo)
        per_it, rel_hi = {a: [] for a in plans}, {}
        for _ in range(args.rounds):
            for a in plans:
                t_lo = pcg(a, lo)[0]
                t_hi, _, done, rel = pcg(a, hi)
                assert done == hi
                per_it[a].append((t_hi - t_lo) / (hi - lo) * 1e3)
                rel_hi[a] = rel
        for a in plans:
            true = np.linalg.norm(b - A[a] @ dsol.download()) / nb if a == "val_f32" else None     # (dsol holds the last arm's x)
            assert rel_hi[a] > 1e-8, (storage, a, "converged inside the run", rel_hi[a])
            assert true is None or abs(true - rel_hi[a]) <= 1e-2 * rel_hi[a], (storage, a, true, rel_hi[a])
        # ---- time to 1e-10
        target = 1e-10

        def refine():
            outer, inner, rel = C.c_int(0), C.c_int(0), C.c_double(0)
            dsol.upload(zeros)
            t0 = time.perf_counter()
            ms, rc = timed_ms(lambda: lib.ehyb_pcg_refine(plans["fp64"].h, plans["val_f32"].h, C.c_void_p(dinv.ptr), C.c_void_p(db.ptr),
                                                          C.c_void_p(dsol.ptr), 20, 100000, target, 1e-5, C.c_void_p(st.ptr), C.byref(outer),
                                                          C.byref(inner), C.byref(rel)))
            assert rc == 0, lib.ehyb_last_error()
            return ms, (time.perf_counter() - t0) * 1e3, outer.value, inner.value, rel.value

        solve = {"pcg fp64": [], "pcg_refine": []}
        info = {}
        for _ in range(args.rounds):
            ms, wall, done, rel = pcg("fp64", 100000, target)
            true = np.linalg.norm(b - A["fp64"] @ dsol.download()) / nb
            assert rel <= target and true <= 2 * target, (storage, "pcg", rel, true)
            solve["pcg fp64"].append(wall)
            info["pcg fp64"] = dict(iterations=done, rel_residual=float(f"{rel:.3e}"), recomputed=float(f"{true:.3e}"))
            ms, wall, outer, inner, rel = refine()
            true = np.linalg.norm(b - A["fp64"] @ dsol.download()) / nb
            assert rel <= target and true <= 2 * target, (storage, "pcg_refine", rel, true)
            solve["pcg_refine"].append(wall)
            info["pcg_refine"] = dict(outer=outer, inner_iterations=inner, rel_residual=float(f"{rel:.3e}"), recomputed=float(f"{true:.3e}"))
        line = dict(workload=args.workload, storage=storage, n=n, nnz=int(A["fp64"].nnz), rounds=args.rounds, loop=LOOP,
                    multiply_us={a: round(min(mult[a]), 2) for a in plans}, multiply_spread={a: spread(mult[a]) for a in plans},
                    multiply_speedup=round(min(mult["fp64"]) / min(mult["val_f32"]), 3), bytes={a: stats_of(a) for a in plans},
                    pcg_us_per_iter={a: round(min(per_it[a]), 1) for a in plans}, pcg_spread={a: spread(per_it[a]) for a in plans},
                    pcg_rel_residual_at_hi={a: float(f"{rel_hi[a]:.3e}") for a in plans}, solve_target=target,
                    solve_wall_ms={a: round(min(v), 2) for a, v in solve.items()}, solve_spread={a: spread(v) for a, v in solve.items()},
                    solve_info=info)
        print(json.dumps(line), flush=True)
        lines.append(line)
        for p in plans.values():
            p.destroy()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hip.hipEventDestroy(ev0)
    hip.hipEventDestroy(ev1)
    st.destroy()


if __name__ == "__main__":
    main()
