#!/usr/bin/env python3
"""What several vectors per pass over the matrix buy (ehyb_spmm): for every k of --k, a plan built for k vectors
(cfg.lds_doubles = 20480 // k; for k = 1 the default plan, the one bench.py times) multiplies k columns in a graph-replayed loop
-- once with the walk alternating from multiply to multiply (what a solver's loop gets, bench.py's `value`), once with every
multiply walking first to last (bench.py's first-to-last arm).  One JSON line per plan: us per multiply and per vector, GFLOP/s
per vector, the speed-up per vector over the default plan's single multiply in the same loop mode, plan stats, and a check of
every column against the CPU oracle after the loop.

A power-law workload (--workload rmat-22 / rmat-24: the residual in panel form, no window) gets wide through its panels instead:
the plan for k has cfg.er_panel_cols = 16384 // k, and three arms are timed for every k > 1, alternating in one process and each
--repeats times, so that the spread of an arm is known before two are compared:
  1  k single multiplies of the DEFAULT plan (16,384-column panels): what a caller without the wide pass has;
  2  k single multiplies of the k-plan (narrow panels, passes of width 1);
  3  one ehyb_spmm(k) on the k-plan: both panel passes k wide.
One JSON line per k: us per vector of every arm and repeat, median and spread, stats.er_partials of both plans, parity.

usage: python tools/spmm_time.py [--workload audikw_1-like|rmat-22|rmat-24] [--sym 0|1] [--k 1,2,4] [--steps 200] [--warmup 20] [--repeats 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRAPH_MULTIPLIES = 20     # multiplies captured per graph (even: an alternating run ends where it can begin again)


def hip_api():
    hip = C.CDLL("libamdhip64.so")
    sig = {
        "hipStreamBeginCapture": [C.c_void_p, C.c_int], "hipStreamEndCapture": [C.c_void_p, C.POINTER(C.c_void_p)],
        "hipGraphInstantiate": [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
        "hipGraphLaunch": [C.c_void_p, C.c_void_p], "hipGraphExecDestroy": [C.c_void_p], "hipGraphDestroy": [C.c_void_p],
        "hipStreamSynchronize": [C.c_void_p], "hipEventCreate": [C.POINTER(C.c_void_p)], "hipEventDestroy": [C.c_void_p],
        "hipEventRecord": [C.c_void_p, C.c_void_p], "hipEventSynchronize": [C.c_void_p],
        "hipEventElapsedTime": [C.POINTER(C.c_float), C.c_void_p, C.c_void_p],
    }
    for name, args in sig.items():
        f = getattr(hip, name)
        f.restype = C.c_int
        f.argtypes = args
    return hip


def ok(rc, what):
    if rc != 0:
        raise SystemExit(f"spmm_time: {what} failed ({rc})")


def time_loop(hip, plan, stream, xd, yd, k, walk_of, steps, warmup, singles=False):
    """ms per multiply of a graph of GRAPH_MULTIPLIES ehyb_spmm calls (walk_of(i): the walk of call i) replayed after `warmup`
    multiplies, timed with HIP events over >= `steps` multiplies.  singles: every multiply as k calls of one column each."""
    graph, exe = C.c_void_p(), C.c_void_p()
    ok(hip.hipStreamBeginCapture(stream, 1), "hipStreamBeginCapture")   # hipStreamCaptureModeThreadLocal
    try:
        for i in range(GRAPH_MULTIPLIES):
            if singles:
                for j in range(k):
                    plan.spmm(xd + 8 * j * plan.n, yd + 8 * j * plan.n, 1, stream=stream, walk=walk_of(i))
            else:
                plan.spmm(xd, yd, k, stream=stream, walk=walk_of(i))
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


def panel_arms(args, ks, hip, stream, gen, gargs, xs, y_refs, scales, n, nnz):
    """The three arms of a panel-form workload (module docstring), the walk alternating from multiply to multiply."""
    import statistics

    import numpy as np

    import bench as B
    import ehyb_spmv_gpu_amd as E
    from oracle import oracle as O

    def build(**kw):
        cfg = E.make_config(partitioner=B.partitioner_for(E, gen), **kw)
        m = E.Matrix.generate(gen, *gargs, cfg=cfg)
        m.reorder(cfg)
        plan = E.Plan(m, cfg)
        return plan, m.reorder_list.copy(), cfg, m

    def parity(yd, k, perm):
        Y = yd.download()[:k * n].reshape(k, n)      # (the default plan's buffer holds the columns of the widest k)
        checks = [O.check_strict(E.vector_recover(Y[j], perm), y_refs[j], scales[j]) for j in range(k)]
        return {"rows_over_1e-12": int(sum(b for b, _ in checks)), "worst_rel": max(w for _, w in checks)}

    d_plan, d_perm, _, d_m = build()
    if d_plan.stats["er_partials"] == 0 or d_plan.stats["lds_bytes"] != 0:
        raise SystemExit("spmm_time: the three panel arms are for a plan whose residual is in panel form and that has no window")
    kcols = max(ks)
    Xd = np.stack([E.vector_reorder(x, d_perm) for x in xs[:kcols]])
    dxd, dyd = E.DeviceBuffer(kcols * n).upload(Xd.ravel()), E.DeviceBuffer(kcols * n)
    bad = 0
    for k in ks:
        if k < 2:
            continue
        plan, perm, cfg, m = build(er_panel_cols=16384 // k)
        X = np.stack([E.vector_reorder(x, perm) for x in xs[:k]])
        xd, yd = E.DeviceBuffer(k * n).upload(X.ravel()), E.DeviceBuffer(k * n)
        arms = {"1_k_singles_default_plan": (d_plan, dxd, dyd, True, d_perm), "2_k_singles_k_plan": (plan, xd, yd, True, perm),
                "3_one_spmm_k_on_k_plan": (plan, xd, yd, False, perm)}
        us_v = {a: [] for a in arms}
        par = {}
        for r in range(args.repeats):
            for a, (pl, x_, y_, singles, pm) in arms.items():
                ms = time_loop(hip, pl, stream.ptr, x_.ptr, y_.ptr, k, lambda i: i & 1, args.steps, args.warmup if r == 0 else GRAPH_MULTIPLIES, singles)
                us_v[a].append(round(ms * 1e3 / k, 2))
                if r == 0:
                    par[a] = parity(y_, k, pm)
        out = {"tool": "spmm_time", "mode": "panel arms", "workload": args.workload, "k": k, "k_max": plan.spmm_max_k, "er_panel_cols": cfg.er_panel_cols,
               "rows": n, "nnz": nnz, "graph_multiplies": GRAPH_MULTIPLIES, "steps": args.steps, "repeats": args.repeats,
               "er_partials": {"default_plan": d_plan.stats["er_partials"], "k_plan": plan.stats["er_partials"]},
               "us_per_vector": {a: {"runs": v, "median": round(statistics.median(v), 2), "spread": round(max(v) - min(v), 2)} for a, v in us_v.items()},
               "parity": par}
        med = {a: statistics.median(v) for a, v in us_v.items()}
        out["speedup_arm3_vs_arm2"] = round(med["2_k_singles_k_plan"] / med["3_one_spmm_k_on_k_plan"], 3)
        out["speedup_arm3_vs_arm1"] = round(med["1_k_singles_default_plan"] / med["3_one_spmm_k_on_k_plan"], 3)
        print(json.dumps(out), flush=True)
        bad += sum(p_["rows_over_1e-12"] for p_ in par.values())
        plan.destroy()
        xd.free(), yd.free()
        m.free()
    d_plan.destroy()
    dxd.free(), dyd.free()
    d_m.free()
    if bad:
        raise SystemExit(f"spmm_time: {bad} rows differ from the CPU product")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--sym", type=int, default=1)
    ap.add_argument("--k", default="1,2,4")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3, help="panel-form workloads: how often every arm is timed")
    ap.add_argument("--no-tune", action="store_true", help="skip ehyb_plan_tune (bench.py tunes every plan it times)")
    args = ap.parse_args()
    import numpy as np

    import bench as B
    import ehyb_spmv_gpu_amd as E
    from oracle import oracle as O

    ks = sorted({int(v) for v in args.k.split(",")})
    if not ks or ks[0] < 1:
        raise SystemExit("--k: a list of positive widths")
    if E.device_count() < 1:
        raise SystemExit("spmm_time: no HIP device visible (nothing here runs on the CPU)")
    gen, gargs, _ = B.WORKLOADS[args.workload]
    sym = bool(args.sym) and B.symmetric_storage_pays(gen, gargs)
    kmax_cols = max(ks)
    hip = hip_api()
    stream = E.Stream()

    # the columns (original numbering) and their CPU products, once
    m0 = E.Matrix.generate(gen, *gargs, cfg=E.make_config())
    n, nnz = m0.n, m0.nnz
    rng = np.random.default_rng(2024)
    xs = [E.x_glibc(n)] + [rng.uniform(-1.0, 1.0, n) for _ in range(kmax_cols - 1)]
    y_refs = [O.spmv_coo(n, m0.I, m0.J, m0.V, x) for x in xs]
    scales = [O.abs_rowsum(n, m0.I, m0.J, m0.V, x) for x in xs]
    m0.free()
    if gen == "rmat":
        return panel_arms(args, ks, hip, stream, gen, gargs, xs, y_refs, scales, n, nnz)

    plans = [("default", 1, {})] + [(f"lds_doubles={20480 // k}", k, {"lds_doubles": 20480 // k}) for k in ks if k > 1]
    base = {}
    for label, k, kw in plans:
        cfg = E.make_config(partitioner=B.partitioner_for(E, gen), **({"sym_pairs": 1} if sym else {}), **kw)
        t0 = time.time()
        m = E.Matrix.generate(gen, *gargs, cfg=cfg)
        m.reorder(cfg)
        plan = E.Plan(m, cfg)
        t_pre = time.time() - t0
        perm = m.reorder_list.copy()
        st = plan.stats
        X = np.stack([E.vector_reorder(x, perm) for x in xs[:k]])
        xd, yd = E.DeviceBuffer(k * n).upload(X.ravel()), E.DeviceBuffer(k * n)
        span = None
        if not args.no_tune:
            s0, s1 = plan.tune(xd.ptr, yd.ptr)        # as bench.py does; a no-op for plans with more than one round of workgroups
            span = [round(s0, 2), round(s1, 2)]
        out = {"tool": "spmm_time", "workload": args.workload, "storage": "symmetric pairs" if st["sym_pairs"] else "every entry stored",
               "plan": label, "lds_doubles": cfg.lds_doubles, "k": k, "k_max": plan.spmm_max_k, "rows": n, "nnz": nnz,
               "graph_multiplies": GRAPH_MULTIPLIES, "steps": args.steps, "warmup": args.warmup, "tune_span_us": span,
               "stats": {key: st[key] for key in ("n_parts", "n_items", "halo_cols", "bytes_format", "bytes_format_ell", "sym_pairs",
                                                  "nnz_er", "lds_bytes")},
               "pre_step_s": round(t_pre, 1)}
        for mode, walk_of in (("alternating", lambda i: i & 1), ("first_to_last", lambda i: 0)):
            ms = time_loop(hip, plan, stream.ptr, xd.ptr, yd.ptr, k, walk_of, args.steps, args.warmup)
            us, us_v = ms * 1e3, ms * 1e3 / k
            if label == "default":
                base[mode] = us
            out[mode] = {"us_per_multiply": round(us, 2), "us_per_vector": round(us_v, 2),
                         "gflops_per_vector": round(2.0 * nnz / (us_v * 1e-6) / 1e9, 1),
                         "speedup_per_vector_vs_default_single": round(base[mode] / us_v, 3) if mode in base else None,
                         "k_single_default_multiplies_us": round(k * base[mode], 2) if mode in base else None}
            # after the loop: every column against the CPU product
            Y = yd.download().reshape(k, n)
            checks = [O.check_strict(E.vector_recover(Y[j], perm), y_refs[j], scales[j]) for j in range(k)]
            out[mode]["parity"] = {"rows_over_1e-12": int(sum(b for b, _ in checks)), "worst_rel": max(w for _, w in checks)}
        print(json.dumps(out), flush=True)
        bad = out["alternating"]["parity"]["rows_over_1e-12"] + out["first_to_last"]["parity"]["rows_over_1e-12"]
        plan.destroy()
        xd.free(), yd.free()
        m.free()
        if bad:
            raise SystemExit(f"spmm_time: {label} k={k}: {bad} rows differ from the CPU product")


if __name__ == "__main__":
    main()
