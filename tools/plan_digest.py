"""Digests of host-built plans, to hold a change of the layout builder against the commit before it: for a fixed list of
host-only builds (no GPU) one JSON line per case with a SHA-256 of the permutation, of every plan array and of the statistics,
and a few facts that show which branch of the builder the case reached (partitions given up, inline residual, panel form,
relative slabs, split rows).  Every case is built twice in one process and the two builds must agree: a slot of an array that
the builder leaves unwritten shows up as a difference once the allocator hands back used pages.
    python tools/plan_digest.py [--threads 8] [--only NAME[,NAME]] [--skip-full] > digest.jsonl
Run it on both commits with the same --threads; the outputs must be identical."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEM_S = ("fem3d", (24000, 3, 20, 20, 13500, 1, 3))
FEM_M = ("fem3d", (120000, 3, 35, 35, 13500, 1, 1))
RMAT_S = ("rmat", (13, 1 << 16, 1))
AUDIKW = ("fem3d", (943695, 3, 68, 68, 13500, 1, 1))

# (name, (generator, arguments), configuration, shape: None = the whole reordered matrix; "rows" = the second of two top-level blocks;
#  "segs" = that with column segments; "unordered" = the matrix as generated, without a partition list)
CASES = [
    ("fem120k-plain", FEM_M, dict(), None),
    ("fem120k-sym-vmap", FEM_M, dict(sym_pairs=1, value_map=1), None),
    ("graded-sym", ("fem3d_graded", (120000, 3, 35, 35, 100000, 705000, 1, 1)), dict(sym_pairs=1), None),
    ("mesh3d-sym", ("mesh3d", (60000, 3, 12, 1500, 3)), dict(sym_pairs=1), None),
    ("stencil2d-plain", ("stencil2d", (300, 300, 9, 0, 3)), dict(partitioner=1, direct=2), None),
    ("banded-plain", ("banded", (1 << 16, 32, 1024)), dict(direct=2), None),
    ("kkt3d-csr-residual", ("kkt3d", (56,)), dict(partitioner=1, lds_doubles=1024), None),
    ("rmat16-defaults", ("rmat", (16, 1 << 19, 1)), dict(direct=2), None),
    ("rmat16-lists-dense-count", ("rmat", (16, 1 << 19, 1)), dict(col_map=2, partitioner=4, direct=2), None),
    ("rmat17-panel", ("rmat", (17, 1 << 20, 1)), dict(er_mode=2), None),
    ("rmat15-some-windows-given-up", ("rmat", (15, 1 << 19, 5)), dict(er_mode=2, lds_doubles=1024, er_panel_cols=1024), None),
    ("rmat18-all-windows-given-up", ("rmat", (18, 1 << 21, 1)), dict(partitioner=1, er_mode=2, lds_doubles=4096), None),
    ("rmat18-prune-pct", ("rmat", (18, 1 << 21, 1)), dict(er_mode=2, prune_pct=60), None),
    ("rmat19-window-sample", ("rmat", (19, 1 << 22, 1)), dict(), None),
    ("fem-no-partition-list", FEM_S, dict(lds_doubles=2048), "unordered"),
    ("fem-window-reference", FEM_S, dict(window_mode=1, lds_doubles=2048), None),
    ("rmat-window-reference", RMAT_S, dict(window_mode=1, lds_doubles=2048), None),
    ("fem-fuse-er-1", FEM_S, dict(fuse_er=1, lds_doubles=1024, cap_split=2), None),
    ("fem-fuse-er-2", FEM_S, dict(fuse_er=2, lds_doubles=1024, cap_split=2), None),
    ("fem-fuse-er-auto", FEM_S, dict(lds_doubles=4096), None),
    ("fem-direct", FEM_S, dict(direct=1), None),
    ("rmat-direct-vmap", RMAT_S, dict(direct=1, value_map=1), None),
    ("fem-sym-lists", FEM_S, dict(col_map=2, sym_pairs=1, value_map=1, lds_doubles=4096), None),
    ("rmat-lists", RMAT_S, dict(col_map=2, lds_doubles=2048), None),
    ("fem-no-sharing", FEM_S, dict(col_sharing=2, lds_doubles=2048), None),
    ("rmat-no-hub-rule", RMAT_S, dict(hub_rule=2, lds_doubles=2048), None),
    ("fem-lds-64", FEM_S, dict(lds_doubles=64), None),
    ("fem-sym-lds-1024", FEM_S, dict(lds_doubles=1024, sym_pairs=1), None),
    ("rmat-lds-1024", RMAT_S, dict(lds_doubles=1024), None),
    ("rmat-split-rows", RMAT_S, dict(er_seg_len=16, lds_doubles=512), None),
    ("fem-plain-vmap", FEM_S, dict(value_map=1, lds_doubles=2048), None),
    ("rmat-panel-vmap", ("rmat", (14, 1 << 17, 1)), dict(value_map=1, lds_doubles=512, er_mode=2, fuse_er=2, er_panel_cols=512, er_block_rows=300), None),
    ("fem-block-row-range", ("fem3d_block", (24000, 3, 16, 16, 13500, 1, 3, 1, 2)), dict(n_top=2, lds_doubles=512), "rows"),
    ("rmat-block-col-segs", ("rmat_block", (15, 1 << 18, 4, 1, 2)), dict(n_top=2, er_mode=2, fuse_er=2, er_panel_cols=1024, direct=2), "segs"),
    ("audikw_1-like", AUDIKW, dict(sym_pairs=1, value_map=1), None),
    ("audikw_1-plain", AUDIKW, dict(value_map=1), None),
]
FULL_SIZE = ("audikw_1-like", "audikw_1-plain")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def build(E, name, gen, cfg_kw, shape, threads):
    from ehyb_spmv_gpu_amd.host import ARRAYS
    cfg = E.make_config(host_threads=threads, **cfg_kw)
    m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
    if shape == "unordered":
        m.c.nParts = 0
    else:
        m.reorder(cfg)
    kw = {}
    if shape in ("rows", "segs"):
        # the second top-level block of the two (its windows may hold its own columns only: the others are remote)
        r0, r1 = (int(m.part_boundary[p]) for p in m.block_first[1:3])
        kw["rows"] = (r0, r1)
    if shape == "segs":
        kw["col_segs"] = np.array([0, r0 & ~1, r0 & ~1, m.n], dtype=np.int32)
    plan = E.Plan(m, cfg, upload=False, **kw)
    arrays = {a: plan.array(a) for a in sorted(ARRAYS)}
    st = plan.stats
    meta3 = arrays["slab_meta"].reshape(-1, 4)[:, 3]
    facts = {
        "rows": m.n, "entries": m.nnz, "parts": st["n_parts"], "windowless_parts": int((arrays["win_len"] == 0).sum()),
        "halo_cols": st["halo_cols"], "relative_slabs": int(((meta3 & 0x80) != 0).sum()), "shared_column_slabs": int(((meta3 & 0x3F) + 1 < 64).sum()),
        "nnz_er": st["nnz_er"], "er_inline": st["er_inline"], "er_partials": st["er_partials"], "er_segments": st["er_segments"],
        "split_rows": int((arrays["er_seg_row"] < 0).sum()), "sym_pairs": st["sym_pairs"], "items": st["n_items"], "segs": len(arrays["segs"]) // 8,
    }
    out = {"case": name, "facts": facts, "perm": sha(m.reorder_list), "stats": hashlib.sha256(json.dumps(st, sort_keys=True).encode()).hexdigest()[:24],
           "arrays": {a: sha(v) for a, v in arrays.items()}}
    plan.destroy()
    m.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-full", action="store_true", help="leave out the full-size cases (a few GB, tens of seconds)")
    a = ap.parse_args()
    import ehyb_spmv_gpu_amd as E
    only = [s for s in a.only.split(",") if s]
    bad = 0
    for name, gen, cfg_kw, shape in CASES:
        if (only and name not in only) or (a.skip_full and name in FULL_SIZE):
            continue
        first = build(E, name, gen, cfg_kw, shape, a.threads)
        again = build(E, name, gen, cfg_kw, shape, a.threads)
        if first != again:
            bad += 1
            diff = [k for k in first["arrays"] if first["arrays"][k] != again["arrays"][k]]
            sys.stderr.write(f"{name}: two builds in one process differ ({diff or 'permutation / statistics'})\n")
        print(json.dumps(first, sort_keys=True), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
