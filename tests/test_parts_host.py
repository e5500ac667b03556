"""The proof that the cases of parts_cases.py exercise what test_gpu_parts_exact.py claims, from the plans' host arrays alone (no
GPU): the oracle walk gives the exact product, the column segments are the ones asked for, pass 1 of a segment stays inside the
segment's columns, every ghost chunk has panels of its own, the split case has row blocks on both sides of cfg.row_split and
none across it, and no window of a plan with windows holds a ghost column."""
import numpy as np
import pytest

import parts_cases as PC
from exact_cases import assert_exact


@pytest.fixture(scope="module", params=list(PC.CASES))
def cp(request, E):
    c = PC.case(E, request.param)
    return c, c.plan(upload=False)


def _segment_units(plan, s):
    """the pass-1 units of column segment s (rows of pb_units1)"""
    u1, it1, si = plan.array("pb_units1").reshape(-1, 4), plan.array("pb_items1").reshape(-1, 2), plan.array("pb_seg_item")
    return u1[it1[si[s], 0]:it1[si[s + 1] - 1, 1]] if si[s + 1] > si[s] else u1[:0]


def test_the_oracle_walk_gives_the_exact_product(O, cp):
    c, plan = cp
    y, written = O.walk_plan(plan, c.x)
    assert np.all(written[:c.n_rows] == 1), c.name
    assert_exact(np.asarray(y)[:c.n_rows], c.y_ref, c.name)
    st = plan.stats
    assert st["n_rows"] == c.n_rows and st["n_cols"] == c.n and st["nnz_ell"] + st["nnz_er"] == len(c.V), c.name
    # the form the case names: panel residual or CSR segments; windows kept or every one given up; no plan of one launch
    assert (st["er_partials"] > 0) == c.panel and (st["nnz_ell"] > 0) == c.windows and st["er_inline"] == 0 and st["nnz_er"] > 0, (c.name, st)
    assert st["er_segments"] < c.n_rows or c.windows, "the direct shape (one segment per row, no window) has no parts"


def test_the_column_segments_are_as_asked(cp):
    c, plan = cp
    n0 = c.n0
    want = [0, n0, n0 + 700, n0 + 958, n0 + 958, n0 + 960]
    assert plan.col_segs == 5 and list(plan.array("col_seg_first")) == want == list(c.segs) and want[-1] == c.n, c.name
    assert n0 % 2 == 0 and all(s % 2 == 0 for s in want)


def test_pass_1_of_a_segment_stays_inside_its_columns(cp):
    c, plan = cp
    if not c.panel:
        assert len(plan.array("pb_units1")) == 0 and len(plan.array("pb_seg_item")) == 0
        return
    it1, si = plan.array("pb_items1").reshape(-1, 2), plan.array("pb_seg_item")
    assert len(si) == c.n_segs + 1 and si[0] == 0 and si[-1] == len(it1) and np.all(np.diff(si) >= 0), c.name
    for s in range(c.n_segs):
        uu = _segment_units(plan, s)
        assert np.all(uu[:, 0] >= c.segs[s]) and np.all(uu[:, 0] + uu[:, 1] <= c.segs[s + 1]), (c.name, s)
        assert np.all(uu[:, 1] <= PC.PANEL_COLS)
    # every entry of a ghost column lies in a unit of that column's segment: the chunks' entries, no more and no fewer
    u1, col = plan.array("pb_units1").reshape(-1, 4), plan.array("pb_col").astype(np.int64)
    live = plan.array("pb_dst") != 0xFFFFFFFF
    for s in range(c.n_segs):
        uu = _segment_units(plan, s)
        got = sum(int(live[b:e].sum()) for _, _, b, e in uu)
        assert got == int(((c.J >= c.segs[s]) & (c.J < c.segs[s + 1])).sum()) - (int((plan.array("ell_src") >= 0).sum()) if s == 0 and c.windows else 0), (c.name, s)
        for c0, nc, b, e in uu:
            assert col[b:e][live[b:e]].max(initial=0) < nc


def test_every_ghost_chunk_has_panels_of_its_own(cp):
    c, plan = cp
    if not c.panel:
        # CSR form: every entry of a ghost column sits in the residual, which EHYB_PART_LAST multiplies
        er_col = plan.array("er_col")
        assert int((er_col >= c.n0).sum()) == int((c.J >= c.n0).sum()) > 0, c.name
        for _, c0, c1 in c.chunks():
            assert (c1 > c0) == bool(np.any((er_col >= c0) & (er_col < c1)))
        return
    for s, c0, c1 in c.chunks():
        panels = len(np.unique(_segment_units(plan, s)[:, 0]))
        assert (panels == 0) == (c1 == c0), (c.name, s)
        if c1 - c0 == 700:
            assert panels >= 3, "the 700-column chunk: two whole panels and a ragged one"
        if c1 - c0 == 258:
            assert panels == 2, "barely over one panel"
    assert [c1 - c0 for _, c0, c1 in c.chunks()] == list(PC.CHUNK_COLS)


def test_the_split_case_has_row_blocks_on_both_sides_and_none_across(cp):
    c, plan = cp
    if not c.panel:
        return
    u2 = plan.array("pb_units2").reshape(-1, 4)
    first, rows = u2[:, 2], np.abs(u2[:, 3])
    assert np.all(np.diff(first) > 0), "pass2_split searches units that ascend by first row"
    assert len(u2) > 1 and rows.max() <= 100, "more than one row block (cfg.er_block_rows)"
    if not c.split:
        assert c.cfg.row_split == 0 and first.max() + rows[-1] <= c.n0
        return
    split = c.cfg.row_split
    assert split == c.n0 and c.n_rows - split == PC.N_FOREIGN
    before, behind = first + rows <= split, first >= split
    assert before.sum() >= 2 and behind.sum() >= 2 and np.all(before | behind), c.name
    # the foreign rows have entries in own columns only: segment 0's pass 1 completes them
    assert c.J[c.I >= split].max() < c.n0 and len(np.unique(c.I[c.I >= split])) >= PC.N_FOREIGN - 20


def test_no_window_holds_a_ghost_column(cp):
    c, plan = cp
    pb, wl, hc = plan.array("part_boundary"), plan.array("win_len"), plan.array("halo_cols")
    if not c.windows:
        assert not wl.any() and len(hc) == 0, "every window given up"
        return
    assert (wl > 0).any() and len(hc) > 0, c.name
    assert int((pb[:-1] + wl)[wl > 0].max()) <= c.n0 and int(hc.max()) < c.n0, c.name
    # and what the window launch alone leaves in y differs from the whole product: the intermediate check of the GPU test is not idle
    yw, rows = c.window_product(plan, c.x)
    assert rows.all() and np.any(yw != c.y_ref) and np.any(yw != 0)


def test_the_f32_arm_has_the_same_exact_product(E):
    """cfg.val_f32 = 1 rounds the values to fp32 at upload; the cases' small integers survive that, so the product of the rounded
    values is the exact product of csr-windows."""
    c = PC.case(E, "csr-windows-f32")
    assert c.cfg.val_f32 == 1 and np.array_equal(c.V.astype(np.float32).astype(np.float64), c.V)
    assert np.array_equal(c.y_ref, PC.case(E, "csr-windows").y_ref)
