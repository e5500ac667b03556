"""Damaged plan-cache files, for tests that never touch a GPU (test_plan_check.py): small plans of every form, a parser of the
file format of csrc/plan_io.cpp that can replace one element of one array, targeted and seeded random mutations, and an
independent STRICT WALK of a file's arrays -- the addressing of the kernels (ell_device.h, ell_t_device.h, panel_device.h, the
residual kernels) and of the host routines that read a loaded plan, as oracle.walk_plan interprets the arrays, with every index
checked against the array it indexes before it is used (numpy's negative indexing would hide an underflow).

The contract the tests hold ehyb_plan_load to: a file is refused (code 6), or it loads and the strict walk of the same bytes
finds nothing out of bounds.  A mutant that stays in bounds may compute another product: values and in-range columns cannot be
told from another matrix without a checksum."""
import ctypes as C

import numpy as np

from util import Case, fem_plus_rmat

LDS_MAX = 20480
MAGIC, END = b"EHYBPLN9", b"EHYBEND4"
# the configuration words a file holds (ehyb_internal.h Config up to ell_nt), all int32
CFG_WORDS = ("lds_doubles part_rows threads window_mode items_per_cu partitioner er_seg_len host_threads verbose seed n_top er_threads ell_variant "
             "col_sharing fuse_er cap_split hub_rule sym_pairs part_boundary_cap er_mode er_panel_cols er_block_rows direct ell_prune value_map prune_pct "
             "er_units1 er_units2 graph_compress balance req_margin sym_slack_permille xcd_map graphs er_sums er_panel_threads er_queue symbolic cg_fused_dot "
             "ell_alternate row_split col_map er_nt ell_nt").split()
SCALARS = np.dtype([("n_cols", "<i4"), ("row_begin", "<i4"), ("row_end", "<i4"), ("n_parts", "<i4"), ("lds_doubles", "<i4"), ("inline_er", "<i4"),
                    ("er_bins", "<i4", 8), ("sym", "<i4"), ("yacc_doubles", "<i4"), ("er_panel", "<i4"), ("pb_panel_cols", "<i4"), ("pb_rows_max", "<i4"),
                    ("direct", "<i4"), ("pb_partials", "<i8"), ("pb_bytes", "<i8"), ("pb_assign", "<i4"), ("val_f32", "<i4")])
assert SCALARS.itemsize == 104
# every array in file order (each_array), behind the permutation
ARRAYS = [("perm", "<i4"), ("part_boundary", "<i4"), ("win_len", "<i4"), ("halo_ptr", "<i4"), ("halo_cols", "<i4"), ("slab_pair_ptr", "<u4"), ("slab_row", "<i4"),
          ("slab_part", "<i4"), ("ell_val", "<f8"), ("ell_col", "<u4"), ("slab_col_ptr", "<u4"), ("lane_group", "u1"), ("slab_meta", "<u4"), ("items", "<i4"),
          ("segs", "<i4"), ("er_seg_ptr", "<i8"), ("er_seg_row", "<i4"), ("er_col", "<i4"), ("er_val", "<f8"), ("er_blocks", "<i4"), ("slab_lrow", "<u2"),
          ("pb_val", "<f8"), ("pb_col", "<u2"), ("pb_dst", "<u4"), ("pb_units1", "<i4"), ("pb_row", "<u2"), ("pb_units2", "<i4"), ("col_seg_first", "<i4"),
          ("pb_seg_item", "<i4"), ("pb_items1", "<i4")]
# the arrays whose elements are indices into something (everything but the value streams)
INDEX_ARRAYS = [name for name, dt in ARRAYS if dt != "<f8"]


class PlanFile:
    """A plan file taken apart: .cfg (int32 words), .scalars (one SCALARS record), .a[name] (copies of the arrays), and where
    every array's count and elements sit in the bytes."""

    def __init__(self, data):
        from ehyb_spmv_gpu_amd import _lib

        self.data = bytes(data)
        assert self.data[:8] == MAGIC and self.data[-8:] == END
        off = 16
        self.cfg_off = off
        self.cfg = np.frombuffer(self.data, "<i4", len(CFG_WORDS), off).copy()
        off += 4 * len(CFG_WORDS)
        self.scalars_off = off
        self.scalars = np.frombuffer(self.data, SCALARS, 1, off)[0].copy()
        off += SCALARS.itemsize + C.sizeof(_lib.Stats)
        self.a, self.where = {}, {}
        for name, dt in ARRAYS:
            count = int(np.frombuffer(self.data, "<u8", 1, off)[0])
            self.where[name] = (off, off + 8, np.dtype(dt), count)
            self.a[name] = np.frombuffer(self.data, dt, count, off + 8).copy()
            off += 8 + count * np.dtype(dt).itemsize
        assert off + 8 == len(self.data)

    def with_element(self, name, index, value):
        """the file's bytes with element `index` of array `name` replaced (value: any integer, wrapped to the element's width)"""
        _, first, dt, count = self.where[name]
        assert 0 <= index < count
        out = bytearray(self.data)
        width = dt.itemsize
        out[first + index * width:first + (index + 1) * width] = (int(value) % (1 << (8 * width))).to_bytes(width, "little")
        return bytes(out)

    def with_cfg(self, word, value):
        out = bytearray(self.data)
        at = self.cfg_off + 4 * CFG_WORDS.index(word)
        out[at:at + 4] = (int(value) % (1 << 32)).to_bytes(4, "little")
        return bytes(out)

    def truncations(self):
        """the file cut at every array boundary (in front of each count, and in front of the end mark)"""
        return [self.data[:self.where[name][0]] for name, _ in ARRAYS] + [self.data[:-8]]


# ---------------------------------------------------------------------------------------------- the small plans, one per form
def _fem(n=2400, seed=11):
    return "fem3d", (n, 3, 8, 8, 20000, 1, seed)


FORMS = {
    # name: (generator, arguments, configuration, what the plan must show)
    "window-halo": (*_fem(), dict(lds_doubles=512, fuse_er=2, cap_split=2, direct=2), lambda st, f: st["halo_cols"] > 0 and st["nnz_ell"] > 0 and not f.scalars["sym"]),
    "sym-pairs": (*_fem(), dict(lds_doubles=1024, sym_pairs=1, fuse_er=2), lambda st, f: st["sym_pairs"] > 0 and f.scalars["sym"] == 1),
    "inline-residual": (*_fem(), dict(lds_doubles=512, fuse_er=1, direct=2), lambda st, f: st["er_inline"] > 0 and f.scalars["inline_er"] == 1),
    "csr-split-rows": ("rmat", (11, 1 << 14, 1), dict(window_mode=1, lds_doubles=256, er_seg_len=16, er_mode=1, fuse_er=2, direct=2),
                       lambda st, f: st["er_segments"] > 0 and (f.a["er_seg_row"] < 0).any() and st["er_partials"] == 0),
    "panel": ("rmat", (11, 1 << 14, 2), dict(er_mode=2, fuse_er=2, lds_doubles=256, er_panel_cols=256, er_block_rows=100, ell_prune=2, direct=2),
              lambda st, f: st["er_partials"] > 0 and st["nnz_ell"] > 0 and not f.scalars["pb_assign"] and len(f.a["pb_units1"]) > 8),
    "panel-assign": (None, None, dict(partitioner=1, er_mode=2, lds_doubles=1024, er_panel_cols=256, er_block_rows=100, direct=2),
                     lambda st, f: f.scalars["pb_assign"] == 1 and st["nnz_ell"] > 0 and (f.a["pb_units2"].reshape(-1, 4)[:, 3] < 0).any()),
    "direct": (*_fem(1500, 3), dict(direct=1), lambda st, f: f.scalars["direct"] == 1 and st["er_segments"] == st["n_rows"]),
    "val-f32": (*_fem(), dict(lds_doubles=512, fuse_er=2, cap_split=2, direct=2, val_f32=1), lambda st, f: f.scalars["val_f32"] == 1 and st["nnz_er"] > 0),
    "column-segments": ("rmat", (11, 1 << 14, 4), dict(er_mode=2, fuse_er=2, er_panel_cols=256, direct=2, partitioner=4),
                        lambda st, f: len(f.a["col_seg_first"]) == 5 and len(f.a["pb_seg_item"]) == 5 and st["er_partials"] > 0),
    "relative-columns": ("banded", (1 << 11, 16, 256), dict(lds_doubles=512, partitioner=1, direct=2),
                         lambda st, f: (f.a["slab_meta"].reshape(-1, 4)[:, 3] & 0x80).any()),
}


def build_form(E, O, name):
    """-> (Case, plan built with upload=False and the defaults a loaded plan has, col_segs or None)"""
    kind, args, kw, shows = FORMS[name]
    cfg = E.make_config(**kw)
    if name == "panel-assign":
        c = Case(E, O, None, None, cfg, matrix=fem_plus_rmat(E, cfg, fem_rows=2400, rmat_scale=11, rmat_edges=1 << 15))
    else:
        c = Case(E, O, kind, args, cfg)
    col_segs = None
    if name == "column-segments":
        n = c.n
        col_segs = np.array([0, (n // 3) & ~1, (n // 3) & ~1, (2 * n // 3) & ~1, n], dtype=np.int32)   # four segments, one of them empty
    return c, E.Plan(c.m, cfg, upload=False, col_segs=col_segs), col_segs


def saved_form(E, O, name, path):
    """the form's plan saved to `path` with its permutation -> (Case, plan, PlanFile); asserts that the plan IS of the form"""
    c, plan, _ = build_form(E, O, name)
    plan.save(path, c.perm, key=c.m.key())
    f = PlanFile(path.read_bytes())
    assert FORMS[name][3](plan.stats, f), (name, plan.stats)
    assert c.n <= 6000, "a few thousand rows at most"
    return c, plan, f


# ---------------------------------------------------------------------------------------------- mutations
def _bound(f, name, index):
    """one past the largest value element `index` of `name` may hold: the bound the loader has to know"""
    s, a = f.scalars, f.a
    nslab, nseg, nsegs = len(a["slab_row"]), len(a["er_seg_row"]), len(a["segs"]) // 8
    if name in ("halo_cols", "er_col", "perm"):
        return int(s["n_cols"])
    if name in ("part_boundary", "slab_row"):
        return int(s["row_end"]) + (name == "part_boundary")
    if name == "er_seg_row":
        return int(s["row_end"])
    if name == "win_len":
        return int(s["n_cols"]) + 1
    if name == "halo_ptr":
        return len(a["halo_cols"]) + 1
    if name == "slab_pair_ptr":
        return len(a["ell_val"]) // 128 + 1
    if name == "slab_col_ptr":
        return len(a["ell_col"]) + 1
    if name == "slab_part":
        return int(s["n_parts"])
    if name == "lane_group":
        return 64
    if name == "slab_lrow":
        return int(s["yacc_doubles"])
    if name == "er_seg_ptr":
        return len(a["er_col"]) + 1
    if name == "er_blocks":
        return (nseg + 1, nseg + 1, 65, 1)[index % 4]
    if name == "items":
        return (nsegs + 1, nsegs + 1, nslab + 1, nslab + 1, nseg + 1, nseg + 1, nseg + 1, nseg + 1)[index % 8]
    if name == "segs":
        return (int(s["n_parts"]), nslab + 1, nslab + 1, len(a["halo_cols"]) + 1, int(s["row_end"]) + 1, int(s["row_end"]) + 1, int(s["n_cols"]) + 1,
                len(a["halo_cols"]) + 1)[index % 8]
    if name == "slab_meta":
        return (len(a["ell_val"]) // 128 + 1, len(a["ell_col"]) + 1, int(s["row_end"]), 1 << 32)[index % 4]
    if name == "ell_col":
        return 1 << 32
    if name == "pb_col":
        return int(s["pb_panel_cols"])
    if name == "pb_dst":
        return int(s["pb_partials"])
    if name == "pb_row":
        return int(s["pb_rows_max"])
    if name == "pb_units1":
        return (int(s["n_cols"]), int(s["pb_panel_cols"]) + 1, len(a["pb_val"]) + 1, len(a["pb_val"]) + 1)[index % 4]
    if name == "pb_units2":
        return (int(s["pb_partials"]) + 1, int(s["pb_partials"]) + 1, int(s["row_end"]), int(s["pb_rows_max"]) + 1)[index % 4]
    if name == "pb_items1":
        return len(a["pb_units1"]) // 4 + 1
    if name == "pb_seg_item":
        return len(a["pb_items1"]) // 2 + 1
    if name == "col_seg_first":
        return int(s["n_cols"]) + 1
    raise KeyError(name)


PREFIX = ("part_boundary", "halo_ptr", "slab_pair_ptr", "slab_col_ptr", "er_seg_ptr", "col_seg_first", "pb_seg_item")


def _live_ell_col(f):
    """index of a column word some lane with a row reads, of a slab with pairs (the words of a slab without rows in them are dead)"""
    meta = f.a["slab_meta"].reshape(-1, 4)
    for s in range(len(meta)):
        if meta[s, 3] >> 16:
            return int(meta[s, 1]) + int(f.a["lane_group"][s * 64] & 0x3F)
    return None


def targeted(f):
    """-> [(label, array name, bytes)]: the mutations every one of which the loader must refuse.  Per index array of the form: an
    element at -1 / all ones, one past its bound, a prefix array made to descend, a record that disagrees with its duplicate;
    a permutation with a repeated entry; the launch-selecting configuration words at values no kernel is built for."""
    out = []
    a = f.a
    for name in INDEX_ARRAYS:
        n = len(a[name])
        if n == 0:
            continue
        i = n // 2
        if name == "ell_col":
            i = _live_ell_col(f)
            if i is None:
                continue
        if name == "slab_lrow":
            i = int(np.flatnonzero(a[name] != 0xFFFF)[0])
        relative = name == "ell_col" and bool(a["slab_meta"][4 * (int(np.searchsorted(a["slab_col_ptr"], i, side="right")) - 1) + 3] & 0x80)
        if name == "lane_group" and f.scalars["sym"]:
            # (bits 6-7 are the lane's part in its group's sum: all ones is group 63 with code 3; 64 is group 0)
            out.append((f"{name}[{i}] = group 63", name, f.with_element(name, i, 0x3F)))
            continue
        if name in ("slab_lrow", "pb_dst") or relative:
            pass  # (all ones is "no row" / padding / the offset -1: legal values)
        else:
            out.append((f"{name}[{i}] = -1", name, f.with_element(name, i, -1)))
        if name in ("er_blocks", "items", "segs", "slab_meta", "pb_units1", "pb_units2"):
            per = 8 if name in ("items", "segs") else 4
            rec = (n // per // 2) * per
            for w in range(per):
                b = _bound(f, name, rec + w)
                if b < (1 << 32) and not (name == "er_blocks" and w == 3):
                    out.append((f"{name}[{rec + w}] = {b}, one past", name, f.with_element(name, rec + w, b)))
        elif name != "ell_col":
            b = _bound(f, name, i)
            out.append((f"{name}[{i}] = {b}, one past", name, f.with_element(name, i, b)))
        if name in PREFIX and n >= 3:
            # descend at one place: an inner element below its predecessor (or, where that one is 0, the successor above the end)
            j = next((k for k in range(1, n - 1) if a[name][k - 1] > 0), None)
            if j is not None:
                out.append((f"{name}[{j}] descends", name, f.with_element(name, j, int(a[name][j - 1]) - 1)))
    # the image length of a column word: one past the last slot of its partition's window
    i = _live_ell_col(f)
    if i is not None and not f.scalars["direct"]:
        meta = a["slab_meta"].reshape(-1, 4)
        s = int(np.searchsorted(a["slab_col_ptr"], i, side="right")) - 1
        p = int(a["slab_part"][s])
        image = int(a["part_boundary"][p] & 1) + int(a["win_len"][p]) + int(a["halo_ptr"][p + 1] - a["halo_ptr"][p])
        if not (meta[s, 3] & 0x80):
            out.append((f"ell_col[{i}] low half = {image}, one past the image", "ell_col", f.with_element("ell_col", i, (int(a["ell_col"][i]) & 0xFFFF0000) | image)))
            out.append((f"ell_col[{i}] high half = {image}", "ell_col", f.with_element("ell_col", i, (int(a["ell_col"][i]) & 0xFFFF) | (image << 16))))
        else:
            out.append((f"ell_col[{i}] low half = 0x8000, relative", "ell_col", f.with_element("ell_col", i, (int(a["ell_col"][i]) & 0xFFFF0000) | 0x8000)))
    # records against their duplicates
    nslab, nsegs = len(a["slab_row"]), len(a["segs"]) // 8
    if nslab:
        s = nslab // 2
        out.append((f"slab_row[{s}] + 1 against slab_meta", "slab_row", f.with_element("slab_row", s, int(a["slab_row"][s]) + 1)))
        out.append((f"slab_meta[{4 * s + 2}] + 1 against slab_row", "slab_meta", f.with_element("slab_meta", 4 * s + 2, int(a["slab_meta"][4 * s + 2]) + 1)))
        out.append((f"slab_meta[{4 * s + 3}] + a pair", "slab_meta", f.with_element("slab_meta", 4 * s + 3, int(a["slab_meta"][4 * s + 3]) + (1 << 16))))
        out.append((f"slab_meta[{4 * s + 3}] bit 6 (the device's flag)", "slab_meta", f.with_element("slab_meta", 4 * s + 3, int(a["slab_meta"][4 * s + 3]) | 0x40)))
    if nsegs:
        g = nsegs // 2
        p = int(a["segs"][8 * g])
        out.append((f"segs[{8 * g + 6}] - 1 against win_len", "segs", f.with_element("segs", 8 * g + 6, int(a["segs"][8 * g + 6]) - 1)))
        out.append((f"win_len[{p}] - 1 against segs", "win_len", f.with_element("win_len", p, int(a["win_len"][p]) - 1)))
        out.append((f"segs[{8 * g + 3}] + 1 against halo_ptr", "segs", f.with_element("segs", 8 * g + 3, int(a["segs"][8 * g + 3]) + 1)))
    if len(a["perm"]):
        out.append(("perm[1] = perm[0]", "perm", f.with_element("perm", 1, int(a["perm"][0]))))
    for word, value in (("threads", 128), ("threads", 768), ("threads", 0), ("er_threads", 512), ("er_threads", 64), ("ell_variant", 2), ("ell_variant", 7),
                        ("er_panel_threads", 256), ("er_panel_threads", 2048), ("host_threads", -5)):
        out.append((f"config {word} = {value}", "config", f.with_cfg(word, value)))
    return out


def random_mutants(f, seed, count):
    """-> [(label, array name, bytes)]: `count` mutants, each one element of one index array (drawn evenly over the arrays the form
    has) replaced -- every other one by a value from the full 32-bit range, the others by one within +-8 of the element's own."""
    rng = np.random.default_rng(seed)
    names = [n for n in INDEX_ARRAYS if len(f.a[n]) > 0]
    out = []
    for k in range(count):
        name = names[k // 2 % len(names)]
        i = int(rng.integers(0, len(f.a[name])))
        old = int(f.a[name][i])
        while True:
            if k % 2 == 0:
                new = int(rng.integers(-(1 << 31), 1 << 32))
            else:
                new = old + int(rng.integers(-8, 9))
            width = 8 * f.a[name].dtype.itemsize
            if new % (1 << width) != old % (1 << width):
                break
        out.append((f"{name}[{i}]: {old} -> {new}", name, f.with_element(name, i, new)))
    return out


# ---------------------------------------------------------------------------------------------- the strict walk
class OutOfBounds(AssertionError):
    pass


def _need(ok, what):
    if not bool(np.all(ok)):
        raise OutOfBounds(what)


def _inside(idx, n, what):
    """every index in [0, n) -- checked before it is used"""
    idx = np.asarray(idx, dtype=np.int64)
    _need((idx >= 0) & (idx < n), f"{what}: index outside [0, {n})")
    return idx


def _i32(v):
    """a stored 32-bit word as the kernels' int"""
    v = np.asarray(v).astype(np.int64)
    return ((v + (1 << 31)) % (1 << 32)) - (1 << 31)


def spmm_width(f):
    """ehyb_spmm_max_k (ehyb_internal.h spmm_width): the widest pass the launches size their LDS for"""
    s = f.scalars
    k = 4
    if s["er_panel"] and s["pb_panel_cols"] > 0 and s["pb_rows_max"] > 0:
        k = min(k, (LDS_MAX - 1) // int(s["pb_panel_cols"]), LDS_MAX // int(s["pb_rows_max"]))
    cap = (int(s["lds_doubles"]) + 1) // 2 * 2
    if not s["direct"] and cap > 0:
        k = min(k, (LDS_MAX * 8 - 16) // (8 * cap))
    k = max(1, k)
    return 1 if s["val_f32"] == 1 else k


def strict_walk(f):
    """Walks a (loadable) file's arrays as every entry point a loaded plan can be given to addresses them -- ehyb_spmv / _phase /
    _walk / ehyb_spmm (the window kernel with and without the inline residual, the CSR-segment kernel adding or assigning, both
    panel passes), ehyb_spmv_t (the same slabs, columns and segments: what the forward kernel reads from x or LDS it adds into
    y or LDS there, plus x[row]), ehyb_spmv_part (the pass-1 items of a column segment), the column transcoder of the upload
    (device_cols), ehyb_plan_resident_bytes and the cost model of ehyb_plan_tune on the host.  Raises OutOfBounds at the first
    index outside the array (or LDS allocation) it indexes.  x and y are n_cols long."""
    s, a = f.scalars, f.a
    n = int(s["n_cols"])
    sym, direct, inline, panel = bool(s["sym"]), bool(s["direct"]), bool(s["inline_er"]), bool(s["er_panel"])
    assign_mode = bool(s["pb_assign"]) and panel
    kmax = spmm_width(f)
    win_cap = (int(s["lds_doubles"]) + 1) // 2 * 2
    items, segs = _i32(a["items"]).reshape(-1, 8), _i32(a["segs"]).reshape(-1, 8)
    meta = a["slab_meta"].astype(np.int64).reshape(-1, 4)
    nslab = len(meta)
    ell_col, ell_pairs = a["ell_col"].astype(np.int64), len(a["ell_val"]) // 2
    lane_group, halo_cols = a["lane_group"].astype(np.int64), _i32(a["halo_cols"])
    lanes = np.arange(64)
    if len(items) and not direct and not (assign_mode and len(segs) == 0):
        _need(kmax * win_cap * 8 + 16 <= LDS_MAX * 8, "the window launch asks for more LDS than a workgroup has")
        for it in items:
            # (the host's cost model of ehyb_plan_tune walks the item's slabs)
            _need(it[2] >= it[3] or (0 <= it[2] and it[3] <= nslab), "items: slab range outside slab_meta")
            for g in range(int(it[0]), int(it[1])):
                _inside(g, len(segs), "segs[item's segment]")
                p_, sb, se, hn, ps, pe, wl, hb = (int(v) for v in segs[g])
                if not sym and wl == 0 and hn == 0:
                    if not assign_mode:   # y = 0 over the rows of the partition's slabs
                        r0 = max(ps, int(_i32(meta[_inside(sb, nslab, "slab_meta[first slab of a windowless segment]"), 2])))
                        r1 = min(pe, r0 + (se - sb) * 64)
                        _need(r1 <= r0 or (r0 >= 0 and r1 <= n), "y rows of a windowless segment")
                    continue
                base, cnt = ps & ~1, wl + (ps & 1)
                _need(cnt >= 0 and hn >= 0, "segs: negative window or halo count")
                _need(cnt == 0 or (base >= 0 and base + cnt <= n), "x[window of the segment]")
                if hn > 0:
                    _need(hb >= 0 and hb + hn <= len(halo_cols), "halo_cols[segment's halo]")
                    _inside(halo_cols[hb:hb + hn], n, "x[halo_cols]")
                image = cnt + hn
                _need(image + (cnt if sym else 0) <= win_cap, "LDS: image (and accumulators) beyond the window capacity")
                if sym:
                    _need(cnt == (ps & 1) or (base + cnt <= n), "y[rows of the partition's accumulators]")
                for sl in range(sb, se):
                    _inside(sl, nslab, "slab_meta[slab of a segment]")
                    vp, cp, r0, shape = (int(v) for v in meta[sl])
                    r0 = int(_i32(r0))
                    npairs, ner, G, rel, coded = shape >> 16, (shape >> 8) & 0xFF, (shape & 0x3F) + 1, bool(shape & 0x80), bool(shape & 0x40)
                    _need(not coded, "slab_meta: the device's flag for triple-coded words in a host record (the kernels would decode pair words as triples)")
                    _need((vp + npairs + (ner if inline else 0)) <= ell_pairs // 64, "ell_val[slab's pairs]")
                    lg = lane_group[_inside(sl * 64 + lanes, len(lane_group), "lane_group[slab]")]
                    grp = lg & 0x3F if sym else lg
                    # the transcoder of the upload copies (or recodes) the slab's host words
                    _need(cp + npairs * G + ner * 128 <= len(ell_col), "ell_col[slab's words], as device_cols reads them")
                    rows = r0 + lanes
                    if sym:
                        lrow = a["slab_lrow"].astype(np.int64)[_inside(sl * 64 + lanes, len(a["slab_lrow"]), "slab_lrow[slab]")]
                        has = lrow != 0xFFFF
                        _inside(lrow[has], cnt, "LDS accumulator of a lane's row (slab_lrow)")
                    else:
                        has = rows < pe
                        lrow = rows - base
                        _inside(rows[has], n, "y[row of a lane]")
                        _inside(lrow[has], max(image, 1), "LDS image[a lane's own row] (x . y on the side)")
                    if npairs:
                        w = ell_col[_inside(cp + grp[None, :] + np.arange(npairs)[:, None] * G, len(ell_col), "ell_col[pair, lane's group]")]
                        c = np.stack([w & 0xFFFF, w >> 16], axis=2)          # [pair][lane][half]
                        if sym:
                            mirror = (c & 0x8000) != 0
                            c = c & 0x7FFF
                            _inside(c, image, "LDS image[column] (symmetric pairs)")
                            _inside(c[mirror], cnt, "LDS accumulator[mirror target]")
                        elif rel:
                            _inside(((c + lrow[None, :, None]) & 0xFFFF)[:, has, :], image, "LDS image[row + offset] (relative columns)")
                        else:
                            _inside(c[:, has, :], image, "LDS image[column]")
                    if ner and inline:
                        ce = ell_col[_inside(cp + npairs * G + np.arange(ner * 128), len(ell_col), "ell_col[inline residual words]")]
                        _inside(ce, n, "x[inline residual column]")
    # the host's walk over the segments (ehyb_plan_resident_bytes, device_cols' slot counts)
    for g in range(len(segs)):
        sb, se = int(segs[g, 1]), int(segs[g, 2])
        _need(se <= sb or (sb >= 0 and se <= nslab), "slab_meta[slabs of a segment], on the host")
    # ---- the CSR-segment residual (the residual launch of a plan without a panel form; the direct shape's only launch)
    seg_ptr, seg_row, er_col, blocks = a["er_seg_ptr"].astype(np.int64), _i32(a["er_seg_row"]), _i32(a["er_col"]), _i32(a["er_blocks"]).reshape(-1, 4)
    if not panel and int(s["er_bins"][3]) != 0:
        for lo, hi, lanes_per, _ in blocks:
            if hi <= lo:
                continue
            sg = _inside(np.arange(lo, hi), len(seg_row), "er_seg_row[segment of a block]")
            _inside(sg + 1, len(seg_ptr), "er_seg_ptr[segment + 1]")
            b, e = seg_ptr[sg], seg_ptr[sg + 1]
            live = e > b
            _need((b[live] >= 0) & (e[live] <= len(er_col)), "er_col[entries of a segment]")
            r = seg_row[sg]
            _inside(r if direct else r & 0x7FFFFFFF, n, "y[row of a segment]")
            for b1, e1 in zip(b[live], e[live]):
                _inside(er_col[b1:e1], n, "x[er_col]")
    # ---- the panel form: pass 1 per item and unit, pass 2 per row block
    if panel:
        u1, it1 = _i32(a["pb_units1"]).reshape(-1, 4), _i32(a["pb_items1"]).reshape(-1, 2)
        u2 = _i32(a["pb_units2"]).reshape(-1, 4)
        col, dst, prow = a["pb_col"].astype(np.int64), a["pb_dst"].astype(np.int64), a["pb_row"].astype(np.int64)
        P, W, R = int(s["pb_partials"]), int(s["pb_panel_cols"]), int(s["pb_rows_max"])
        nchunks = len(dst) // 64
        _need(len(col) == len(dst) == len(a["pb_val"]) and len(dst) % 64 == 0, "the pass-1 streams differ in length")
        # k panel images and the hand-over word; the LDS-sum arm (one vector) adds a word per thread of up to 1024
        _need(kmax * W + 1 <= LDS_MAX and W + 1024 + 1 <= LDS_MAX, "LDS of pass 1")
        _need(R * kmax <= LDS_MAX, "LDS of pass 2")
        # (ehyb_spmv_part launches the items [pb_seg_item[s], pb_seg_item[s + 1]): a range outside the item list is refused by the launch itself)
        for i0, i1 in it1:
            for ui in range(int(i0), int(i1)):
                c0, ncol, b, e = (int(v) for v in u1[_inside(ui, len(u1), "pb_units1[unit of an item]")])
                _need(ncol >= 0 and (ncol == 0 or (c0 >= 0 and c0 + ncol <= n)), "x[panel of a unit]")
                _need(ncol <= W, "LDS: a unit's panel beyond pb_panel_cols")
                ch0, ch1 = b >> 6, e >> 6
                # the chunk records of the first step are fetched whatever the count: chunk[max(ch0, min(.., ch1 - 1))] and the one behind
                _inside(max(ch0, ch1 - 1) + 1, nchunks + 1, "pb_chunk[first chunk of a unit + 1]")
                _inside(ch0, nchunks + 1, "pb_chunk[first chunk of a unit]")
                if ch1 > ch0:
                    _need(ch1 <= nchunks, "pb_val[entries of a unit]")
                    k = np.arange(ch0 * 64, ch1 * 64)
                    _inside(col[k] & 0x3FFF, max(ncol, 1), "LDS panel[column of an entry]")
                    live = dst[k] != 0xFFFFFFFF
                    _inside(dst[k][live], P, "partial[slot of an entry]")
        for q0, q1, r0, rows in u2:
            rows = abs(int(rows))
            _need(rows <= R, "LDS: a row block beyond pb_rows_max")
            _need(rows == 0 or (r0 >= 0 and r0 + rows <= n), "y[rows of a block]")
            if q1 > q0:
                _need(q0 >= 0 and q1 <= P and q1 <= len(prow), "partial[partials of a block]")
                _inside(prow[q0:q1], rows, "LDS accumulator[pb_row]")
    perm = _i32(a["perm"])
    if len(perm):
        _need(len(perm) == n, "perm: not n_cols long")
        _inside(perm, n, "perm")          # (vector_reorder / vector_recover index with it)
        _need(len(np.unique(perm)) == n, "perm: an entry repeats")
    return True
