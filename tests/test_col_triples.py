"""The column words as the device holds them (cfg.ell_triples; csrc/col_triples.h): ehyb_plan_upload sends one 16-bit base per node
triple where a slab's column lists allow it.  CPU only: ehyb_plan_device_cols returns the arrays of a host plan, and a numpy
decoder of the device form, written here from the description in include/ehyb.h, must give -- slab by slab, lane by lane -- the
columns of the canonical decode of EHYB_ARR_ELL_COL.  The one allowed difference: a padding slot (value 0.0 in EHYB_ARR_ELL_VAL)
may read column 1 or 2 where the canonical form reads 0."""
import ctypes as C

import numpy as np
import pytest

TRIPLES = 0x40          # bit 6 of a device record's shape word
FEM6 = ("fem3d", (6000, 3, 12, 12, 20000, 1, 5))
FEM24 = ("fem3d", (24000, 3, 20, 20, 13500, 1, 4))
# 16 partitions asked for instead of the sizing's own count, heavily scrambled: windows too large for four columns per pass
# (ehyb_spmm_max_k = 3) whose halo overflows, so a plan with symmetric pairs AND an inline residual that still gets coded slabs
WIDE = ("fem3d", (24000, 3, 12, 12, 250000, 1, 5), 16)
WIDE_KW = dict(lds_doubles=6144, cap_split=2, fuse_er=1, sym_pairs=1)

# (id, generator, configuration)
CASES = [
    ("fem6000-sym", FEM6, dict(lds_doubles=1024, sym_pairs=1)),
    ("fem6000-plain", FEM6, dict(lds_doubles=1024)),
    ("fem6000-sym-inline", FEM6, dict(lds_doubles=1024, sym_pairs=1, fuse_er=1)),
    ("fem6000-plain-inline", FEM6, dict(lds_doubles=1024, fuse_er=1)),
    ("fem24000-sym", FEM24, dict(sym_pairs=1)),
    ("wide-sym-inline", WIDE, WIDE_KW),
    ("dof1", ("fem3d", (6000, 1, 12, 12, 20000, 1, 5)), dict(lds_doubles=1024, sym_pairs=1)),
    ("dof2", ("fem3d", (6000, 2, 12, 12, 20000, 1, 5)), dict(lds_doubles=1024, sym_pairs=1)),
    ("dof6", ("fem3d", (6000, 6, 12, 12, 20000, 1, 5)), dict(lds_doubles=1024, sym_pairs=1)),
    ("dof6-plain", ("fem3d", (6000, 6, 12, 12, 20000, 1, 5)), dict(lds_doubles=1024)),
    ("banded", ("banded", (1 << 16, 32, 1024)), dict(direct=2)),
    ("rmat", ("rmat", (13, 1 << 16, 2)), dict(lds_doubles=1024)),
    # short rows, which none of the generators' cases has: slabs of 2, 5 and 6 pairs
    ("nodes", ("nodes", (2048,)), dict(lds_doubles=1024, direct=2)),
]


def node_matrix(n_nodes, dof=3, seed=1):
    """CSR of a matrix of n_nodes nodes with dof unknowns each: the first half of the nodes couple to themselves only (3 entries per
    row: slabs of 2 pairs, one of them padding), the second half to the nodes i-1 .. i+2 of their half (12 entries: 6 pairs; 9 at the
    end: 5 pairs)."""
    half = n_nodes // 2
    rows = []
    for i in range(n_nodes):
        nb = [i] if i < half else [j for j in (i - 1, i, i + 1, i + 2) if half <= j < n_nodes]
        rows += [np.concatenate([np.arange(dof * j, dof * j + dof) for j in nb])] * dof
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    indices = np.concatenate(rows)
    return indptr, indices, np.random.default_rng(seed).uniform(0.5, 1.5, len(indices))


def make_matrix(E, gen, cfg):
    if gen[0] == "nodes":
        return E.Matrix.from_csr(*node_matrix(*gen[1]), cfg)
    m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
    if len(gen) > 2:
        m.c.nParts = gen[2]       # partitions the reorder step is asked for
    return m


def device_cols(plan):
    """ehyb_plan_device_col_words / ehyb_plan_device_cols -> (words, records [n_slabs, 4])"""
    lib = plan.lib
    n = int(lib.ehyb_plan_device_col_words(plan.h))
    assert n >= 0
    words = np.zeros(max(n, 1), dtype=np.uint32)
    meta = np.zeros(max(len(plan.array("slab_meta")), 1), dtype=np.uint32)
    assert lib.ehyb_plan_device_cols(plan.h, words.ctypes.data_as(C.POINTER(C.c_uint32)), meta.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    return words[:n], meta[:len(plan.array("slab_meta"))].reshape(-1, 4)


def canonical_entries(col, rec):
    """The 16-bit entries [2 np, G] of a slab of the HOST form: entry 2k is the low half of word (pair k, group g), 2k + 1 the high."""
    npairs, G = int(rec[3]) >> 16, (int(rec[3]) & 0x3F) + 1
    w = col[int(rec[1]):int(rec[1]) + npairs * G].reshape(npairs, G)
    e = np.empty((2 * npairs, G), dtype=np.uint32)
    e[0::2], e[1::2] = w & 0xFFFF, w >> 16
    return e


def decode_triples(words, rec):
    """The entries [2 np, G] of a triple-coded slab of the DEVICE form: T = ceil(2 np / 3) bases per group, two per word (low half
    first), W = ceil(T / 2) words per group at [word][group]; with (A, B) = word j the pairs 3j, 3j+1, 3j+2 read the columns
    (A, A+1), (A+2, B), (B+1, B+2)."""
    npairs, G = int(rec[3]) >> 16, (int(rec[3]) & 0x3F) + 1
    T = -(-2 * npairs // 3)
    W = -(-T // 2)
    w = words[int(rec[1]):int(rec[1]) + W * G].reshape(W, G)
    bases = np.empty((2 * W, G), dtype=np.uint32)
    bases[0::2], bases[1::2] = w & 0xFFFF, w >> 16
    e = (np.repeat(bases, 3, axis=0) + np.tile(np.arange(3, dtype=np.uint32), 2 * W)[:, None])[:2 * npairs]
    return e, W * G


def window_slots(plan, n_slabs):
    """slots of the LDS image every slab reads from (own rows from the even row down, then the halo)"""
    segs = plan.array("segs").reshape(-1, 8)
    slots = np.zeros(n_slabs, dtype=np.int64)
    for part, sb, se, hn, r0, r1, wl, hb in segs:
        slots[sb:se] = wl + (r0 & 1) + hn
    return slots


def check_plan(E, plan):
    """Decodes every slab of the device form against the host form -> list of (np, G) of the triple-coded slabs"""
    st = plan.stats
    col, meta = plan.array("ell_col"), plan.array("slab_meta").reshape(-1, 4)
    val = plan.array("ell_val")
    words, dmeta = device_cols(plan)
    n_slabs = len(meta)
    assert dmeta.shape == meta.shape
    assert np.array_equal(dmeta[:, [0, 2]], meta[:, [0, 2]]) and np.array_equal(dmeta[:, 3] & ~np.uint32(TRIPLES), meta[:, 3])
    assert not (meta[:, 3] & TRIPLES).any(), "bit 6 is free in the host records"
    slots = window_slots(plan, n_slabs)
    coded, at = [], 0
    for s in range(n_slabs):
        rec, drec = meta[s], dmeta[s]
        npairs, ner, G, rel = int(rec[3]) >> 16, (int(rec[3]) >> 8) & 0xFF, (int(rec[3]) & 0x3F) + 1, bool(rec[3] & 0x80)
        assert int(drec[1]) == at, "the slabs follow each other in the device array"
        host_words = npairs * G + ner * 128
        if not drec[3] & TRIPLES:
            assert np.array_equal(words[at:at + host_words], col[int(rec[1]):int(rec[1]) + host_words]), s
            at += host_words
            continue
        assert ner == 0 and not rel and slots[s] >= 3 and npairs > 0, s
        want = canonical_entries(col, rec)
        got, used = decode_triples(words, drec)
        at += used
        lg = plan.array("lane_group")[64 * s:64 * s + 64] & 0x3F
        # lane by lane: pair k of lane l holds ell_val[((pair_ptr + k) * 64 + l) * 2 + half]
        v = val[int(rec[0]) * 128:(int(rec[0]) + npairs) * 128].reshape(npairs, 64, 2).transpose(0, 2, 1).reshape(2 * npairs, 64)
        w_l, g_l = want[:, lg], got[:, lg]
        differ = w_l != g_l
        if differ.any():
            assert (v[differ] == 0.0).all(), f"slab {s}: a stored entry reads another column"
            assert (w_l[differ] == 0).all() and (g_l[differ] <= 2).all(), f"slab {s}: padding reads past column 2"
        assert (g_l & 0x7FFF).max() < slots[s], s
        coded.append((npairs, G))
    assert at == len(words)
    return coded, len(words)


@pytest.fixture(scope="module")
def plans(E):
    out = {}
    for name, gen, kw in CASES:
        cfg = E.make_config(**kw)
        m = make_matrix(E, gen, cfg)
        m.reorder(cfg)
        out[name] = (E.Plan(m, cfg, upload=False), m, cfg, kw)
    return out


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_device_form_decodes_to_the_host_columns(E, plans, name):
    plan, m, cfg, kw = plans[name]
    st = plan.stats
    assert cfg.ell_triples == 1
    coded, n_words = check_plan(E, plan)
    meta = plan.array("slab_meta").reshape(-1, 4)
    if "inline" in name:
        assert st["er_inline"] > 0 and ((meta[:, 3] >> 8) & 0xFF).any(), "the case must hold slabs with inline pairs"
    if name == "banded":
        assert (meta[:, 3] & 0x80).any(), "the case must hold relative slabs"
    if name == "fem6000-sym-inline":
        # four columns per pass fit, and the kernel of that width with symmetric pairs and an inline residual has no triple
        # arm: the whole plan keeps the host's words (include/ehyb.h)
        assert plan.spmm_max_k == 4 and not coded and n_words == st["col_words"]
    if name == "wide-sym-inline":
        assert plan.spmm_max_k < 4 and st["sym_pairs"] > 0 and len(coded) > 0, "slabs with inline pairs beside coded ones"
    if name in ("fem6000-sym", "fem6000-plain", "fem24000-sym", "dof6", "dof6-plain", "nodes"):
        assert len(coded) > 0 and n_words < st["col_words"]
    if name in ("dof1", "dof2", "rmat"):
        assert n_words <= st["col_words"]
    if name == "fem24000-sym":
        assert n_words <= 0.36 * st["col_words"], (n_words, st["col_words"])


def test_cases_cover_every_tail_and_length(E, plans):
    nps = set()
    for name in plans:
        nps |= {c[0] for c in check_plan(E, plans[name][0])[0]}
    assert {p % 3 for p in nps} == {0, 1, 2}, sorted(nps)
    assert any(p < 3 for p in nps) and 6 in nps and any(p > 6 for p in nps), sorted(nps)


@pytest.mark.parametrize("name", ["fem6000-sym", "fem6000-plain-inline", "banded"])
def test_switch_off_returns_the_host_arrays(E, plans, name):
    _, m, _, kw = plans[name]
    for value, on in ((0, True), (1, True), (2, False)):
        cfg = E.make_config(ell_triples=value, **kw)
        assert cfg.ell_triples == (1 if on else 2)
        plan = E.Plan(m, cfg, upload=False)
        words, dmeta = device_cols(plan)
        same = np.array_equal(words, plan.array("ell_col")) and np.array_equal(dmeta.ravel(), plan.array("slab_meta"))
        if on:
            w1, m1 = device_cols(plans[name][0])
            assert np.array_equal(words, w1) and np.array_equal(dmeta, m1)
            assert same == (not (dmeta[:, 3] & TRIPLES).any())
        else:
            assert same and len(words) == plan.stats["col_words"]
        plan.destroy()


@pytest.mark.parametrize("name", ["fem6000-sym", "fem24000-sym", "rmat"])
def test_two_builds_agree_byte_for_byte(E, plans, name):
    plan, m, cfg, kw = plans[name]
    a = device_cols(plan)
    other = E.Plan(m, E.make_config(host_threads=3, **kw), upload=False)
    b = device_cols(other)
    c = device_cols(plan)
    for x, y in ((a, b), (a, c)):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
    other.destroy()


def test_host_layout_and_stats_do_not_depend_on_the_switch(E, plans):
    plan, m, cfg, kw = plans["fem6000-sym"]
    off = E.Plan(m, E.make_config(ell_triples=2, **kw), upload=False)
    assert off.stats == plan.stats and off.resident_bytes == plan.resident_bytes
    for name in ("ell_col", "slab_meta", "slab_col_ptr", "lane_group", "segs"):
        assert np.array_equal(off.array(name), plan.array(name)), name
    off.destroy()
