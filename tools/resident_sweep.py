#!/usr/bin/env python3
"""How much of the window kernel's value stream should stay in the Infinity Cache (cfg.ell_nt = 4 / 5, cfg.ell_keep).

One process, one matrix and permutation; one plan per arm: cfg.ell_nt = 1 (every slab with the non-temporal hint: share 0), 3 (plain
loads for the end of an alternating walk), 4 (a fixed set spread over every partition) and 5 (a fixed set at the start of every
partition) with cfg.ell_keep from --keeps, each pinned arm both with its own default walk (first to last) and alternating.  The
arms run interleaved, --rounds times, each time an event-timed loop of --steps multiplies after --warmup (Plan.bench: the loop
between two HIP events on the launch stream).  Per arm, one JSON line: us per multiply of every round, ehyb_plan_resident_bytes,
and `cold_us`: the time of ONE multiply issued right after a 512 MiB fill of another buffer -- the caller who multiplies once after
other work, who finds the pinned slabs as plain-load misses.

usage: python tools/resident_sweep.py [--workload audikw_1-like] [--sym -1|0|1] [--keeps 100,200,...] [--steps 256] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="audikw_1-like")
    ap.add_argument("--sym", type=int, default=-1, help="1 = symmetric pair storage, 0 = every entry stored, -1 = as bench.py chooses for the workload")
    ap.add_argument("--keeps", default="100,200,300,400,450,500,550,600,700", help="cfg.ell_keep of the pinned arms, per mille; 0 = automatic")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cold-reps", type=int, default=5)
    args = ap.parse_args()
    if args.steps < 200:
        raise SystemExit("resident_sweep: loops of at least 200 multiplies")

    import numpy as np
    import torch

    import bench as B
    import ehyb_spmv_gpu_amd as E

    if E.device_count() < 1:
        raise SystemExit("resident_sweep: no HIP device visible (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    gen, gargs, _ = B.WORKLOADS[args.workload]
    if args.sym < 0:
        args.sym = 1 if B.symmetric_storage_pays(gen, gargs) else 0
    kw = dict(partitioner=B.partitioner_for(E, gen), **(dict(sym_pairs=1) if args.sym else {}))
    cfg0 = E.make_config(**kw)
    m = E.Matrix.generate(gen, *gargs, cfg=cfg0)
    x = E.x_glibc(m.n)
    m.reorder(cfg0)
    perm = m.reorder_list.copy()
    x_d = torch.from_numpy(E.vector_reorder(x, perm)).to(dev)
    y_d = torch.zeros(m.n, dtype=torch.float64, device=dev)
    fill = torch.empty(512 << 17, dtype=torch.float64, device=dev)   # 512 MiB
    stream = torch.cuda.current_stream().cuda_stream
    xp, yp = x_d.data_ptr(), y_d.data_ptr()

    keeps = [int(k) for k in args.keeps.split(",") if k != ""]
    arms = [("nt1", dict(ell_nt=1)), ("nt3", dict(ell_nt=3)), ("nt3-first-to-last", dict(ell_nt=3, ell_alternate=2))]
    for k in keeps:
        arms.append((f"spread-{k}", dict(ell_nt=4, ell_keep=k)))
        arms.append((f"block-{k}", dict(ell_nt=5, ell_keep=k)))
        arms.append((f"spread-{k}-alternating", dict(ell_nt=4, ell_keep=k, ell_alternate=1)))
    plans, y_first = [], None
    for name, akw in arms:
        plan = E.Plan(m, E.make_config(**kw, **akw))
        plan.tune(xp, yp)
        plan.spmv(xp, yp, stream)
        torch.cuda.synchronize()
        y = y_d.cpu().numpy()
        if y_first is None:
            y_first = y
        worst = float(np.max(np.abs(y - y_first) / np.maximum(np.abs(y_first), 1e-300)))
        plans.append(dict(arm=name, cfg=akw, plan=plan, us=[], cold=[], worst_rel_to_first_arm=worst))
    st = plans[0]["plan"].stats
    value = 8 * st["size_block_ell"]
    print(json.dumps({"workload": args.workload, "sym": args.sym, "n": m.n, "nnz": m.nnz, "bytes_format_ell": st["bytes_format_ell"],
                      "value_stream_bytes": value, "plain_bytes": st["bytes_format_ell"] - value,
                      "automatic_keep1024": E.host._lib.load().ehyb_ell_auto_keep1024(value, st["bytes_format_ell"] - value),
                      "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}), flush=True)
    for rnd in range(args.rounds):
        for p in (plans if rnd % 2 == 0 else plans[::-1]):
            r = p["plan"].bench(xp, yp, stream, warmup=args.warmup, iters=args.steps, per_kernel=False)
            p["us"].append(round(r["ms_total"] / args.steps * 1e3, 2))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(args.cold_reps):
        for p in plans:
            for _ in range(4):
                p["plan"].spmv(xp, yp, stream)     # the plan's steady state first: what it pins is in the cache
            fill.fill_(float(rep))
            e0.record()
            p["plan"].spmv(xp, yp, stream)
            e1.record()
            torch.cuda.synchronize()
            p["cold"].append(round(e0.elapsed_time(e1) * 1e3, 2))
    for p in plans:
        print(json.dumps({"arm": p["arm"], **p["cfg"], "us": p["us"], "us_median": statistics.median(p["us"]),
                          "resident_bytes": p["plan"].resident_bytes, "cold_us": p["cold"], "cold_us_median": statistics.median(p["cold"]),
                          "worst_rel_to_first_arm": p["worst_rel_to_first_arm"]}), flush=True)
        p["plan"].destroy()


if __name__ == "__main__":
    main()
