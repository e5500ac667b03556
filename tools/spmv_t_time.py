#!/usr/bin/env python3
"""What y = A^T x on the plan A already has costs (ehyb_spmv_t), against the only way there was before: transpose
on the host, reorder and build a second plan, multiply with that.  Per workload three arms are timed on ONE device in ONE
process, alternating, each --repeats times, so that the spread of an arm is known before two are compared:
  t  ehyb_spmv_t on the plan of A                                  (the feature)
  a  ehyb_spmv   on the same plan        (what the forward multiply of the same layout takes: the price of the atomics)
  b  ehyb_spmv   on a plan built from the host-transposed matrix   (the yardstick: the same product, by the old way)
Every arm is a hipGraph of GRAPH_MULTIPLIES multiplies replayed after a warm-up and timed with HIP events over >= --steps
multiplies.  Beside the times: the device bytes of one plan against two (stats.bytes_format of each), what the second plan's
pre-step took on the host, and a check of arm t against the CPU product A^T x and of arm b's plan against the same vector.

Workloads: the bench matrix (audikw_1-like) with every entry stored and UNSYMMETRIC values (upper entries x 1.3, lower x 0.7,
as tools/gmres_time.py), and one workload whose residual is in CSR segments (rmat-22, built with cfg.er_mode = 1: the transposed
row-segment kernel, global atomics on hub columns).  One JSON line per workload.

usage: python tools/spmv_t_time.py [--workloads audikw_1-like,rmat-22] [--steps 200] [--warmup 40] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from spmm_time import hip_api, ok  # noqa: E402

GRAPH_MULTIPLIES = 20


def time_loop(hip, launch, stream, steps, warmup):
    """ms per multiply: a graph of GRAPH_MULTIPLIES calls of launch(i) on `stream`, replayed after `warmup` multiplies and timed
    with HIP events over >= `steps` multiplies"""
    graph, exe = C.c_void_p(), C.c_void_p()
    ok(hip.hipStreamBeginCapture(stream, 1), "hipStreamBeginCapture")
    try:
        for i in range(GRAPH_MULTIPLIES):
            launch(i)
    finally:
        ok(hip.hipStreamEndCapture(stream, C.byref(graph)), "hipStreamEndCapture")
    ok(hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0), "hipGraphInstantiate")
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")
    try:
        for _ in range(max(1, -(-warmup // GRAPH_MULTIPLIES))):
            ok(hip.hipGraphLaunch(exe, stream), "hipGraphLaunch")
        ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
        reps = max(1, -(-steps // GRAPH_MULTIPLIES))
        ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        for _ in range(reps):
            ok(hip.hipGraphLaunch(exe, stream), "hipGraphLaunch")
        ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float(0)
        ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return ms.value / (reps * GRAPH_MULTIPLIES)
    finally:
        hip.hipEventDestroy(ev0)
        hip.hipEventDestroy(ev1)
        hip.hipGraphExecDestroy(exe)
        hip.hipGraphDestroy(graph)


def unsymmetric(m):
    """upper entries x 1.3, lower x 0.7, in place: a pattern that stays, values that are no longer symmetric"""
    I, J, V = m.I, m.J, m.V
    V[I < J] *= 1.3
    V[I > J] *= 0.7


def run(args, name, hip, stream):
    import numpy as np
    import scipy.sparse as sp

    import bench as B
    import ehyb_spmv_gpu_amd as E
    from oracle import oracle as O

    gen, gargs, _ = B.WORKLOADS[name]
    kw = dict(partitioner=B.partitioner_for(E, gen), sym_pairs=0)
    if gen == "rmat":
        kw.update(er_mode=1, fuse_er=2)         # the residual in CSR segments, its own launch
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    unsymmetric(m)
    n, nnz = m.n, m.nnz
    A = sp.csr_matrix((m.V.copy(), m.J.copy(), m.row_idx.astype(np.int64)), shape=(n, n))
    x = E.x_glibc(n)
    yt_ref = O.spmv_coo(n, m.J, m.I, m.V, x)                 # A^T x: the COO product with rows and columns swapped
    yt_scale = O.abs_rowsum(n, m.J, m.I, m.V, x)
    t0 = time.time()
    m.reorder(cfg)
    plan = E.Plan(m, cfg)
    pre_a = time.time() - t0
    perm = m.reorder_list.copy()
    m.free()
    if not plan.spmv_t_supported:
        raise SystemExit(f"spmv_t_time: {name}: {plan.spmv_t_refusal[1]}")
    # arm b: the host transposes, then the whole pre-step again
    t0 = time.time()
    At = A.T.tocsr()
    At.sort_indices()
    t_transpose = time.time() - t0
    t0 = time.time()
    mt = E.Matrix.from_csr(At.indptr, At.indices, At.data, cfg)
    mt.reorder(cfg)
    plan_b = E.Plan(mt, cfg)
    pre_b = time.time() - t0
    perm_b = mt.reorder_list.copy()
    mt.free()
    del A, At

    xd, yd = E.DeviceBuffer(n).upload(E.vector_reorder(x, perm)), E.DeviceBuffer(n)
    xb, yb = E.DeviceBuffer(n).upload(E.vector_reorder(x, perm_b)), E.DeviceBuffer(n)
    arms = {
        "t_spmv_t_same_plan": lambda i: plan.spmv_t(xd.ptr, yd.ptr, stream=stream),
        "a_spmv_same_plan": lambda i: plan.spmv(xd.ptr, yd.ptr, stream=stream, walk=i & 1),
        "b_spmv_transposed_plan": lambda i: plan_b.spmv(xb.ptr, yb.ptr, stream=stream, walk=i & 1),
    }
    us = {a: [] for a in arms}
    for r in range(args.repeats):
        for a, launch in arms.items():
            us[a].append(round(time_loop(hip, launch, stream, args.steps, args.warmup if r == 0 else GRAPH_MULTIPLIES) * 1e3, 2))
    # parity after the loops: arm t last wrote yd through the forward arm -- multiply once more each
    plan.spmv_t(xd.ptr, yd.ptr, stream=stream)
    plan_b.spmv(xb.ptr, yb.ptr, stream=stream)
    ok(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    bad_t, worst_t = O.check_strict(E.vector_recover(yd.download(), perm), yt_ref, yt_scale)
    bad_b, worst_b = O.check_strict(E.vector_recover(yb.download(), perm_b), yt_ref, yt_scale)
    med = {a: statistics.median(v) for a, v in us.items()}
    st, stb = plan.stats, plan_b.stats
    out = {"tool": "spmv_t_time", "workload": name, "storage": "every entry stored, unsymmetric values", "rows": n, "nnz": nnz,
           "config": kw, "graph_multiplies": GRAPH_MULTIPLIES, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "launched_t": sorted(plan.launched_t()),
           "us_per_multiply": {a: {"runs": v, "median": round(med[a], 2), "spread": round(max(v) - min(v), 2)} for a, v in us.items()},
           "spmv_t_over_b": round(med["t_spmv_t_same_plan"] / med["b_spmv_transposed_plan"], 3),
           "spmv_t_over_a": round(med["t_spmv_t_same_plan"] / med["a_spmv_same_plan"], 3),
           "gflops_spmv_t": round(2.0 * nnz / (med["t_spmv_t_same_plan"] * 1e-6) / 1e9, 1),
           "device_bytes": {"one_plan": st["bytes_format"], "two_plans": st["bytes_format"] + stb["bytes_format"]},
           "host_s": {"pre_step_plan_of_A": round(pre_a, 1), "transpose": round(t_transpose, 1), "pre_step_second_plan": round(pre_b, 1)},
           "stats": {key: st[key] for key in ("n_parts", "n_items", "halo_cols", "nnz_ell", "nnz_er", "er_inline", "er_segments", "lds_bytes")},
           "parity": {"t_rows_over_1e-12": int(bad_t), "t_worst_rel": worst_t, "b_rows_over_1e-12": int(bad_b), "b_worst_rel": worst_b}}
    print(json.dumps(out), flush=True)
    plan.destroy(), plan_b.destroy()
    for d in (xd, yd, xb, yb):
        d.free()
    if bad_t or bad_b:
        raise SystemExit(f"spmv_t_time: {name}: {bad_t} (spmv_t) / {bad_b} (transposed plan) rows differ from the CPU product A^T x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="audikw_1-like,rmat-22")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import ehyb_spmv_gpu_amd as E

    if E.device_count() < 1:
        raise SystemExit("spmv_t_time: no HIP device visible (nothing here runs on the CPU)")
    hip = hip_api()
    stream = E.Stream()
    for name in args.workloads.split(","):
        run(args, name, hip, stream.ptr)


if __name__ == "__main__":
    main()
