"""ehyb_spmm_max_k of a plan whose residual is in panel form: the width one pass over the matrix serves is what FITS the LDS --

    k_panel  = min(4, (20480 - 1) // pb_panel_cols, 20480 // pb_rows_max)     pass 1: k panel images + the hand-over word;
                                                                              pass 2: k accumulators per row of the largest block
    k_window = the window rule (4 where the plan has no window launch)
    k_max    = min(k_panel, k_window)

pb_panel_cols is the CONFIGURED panel width (cfg.er_panel_cols, default 16,384), so default plans stay at 1.  Every test asserts
the shape of the plan it is named for before it asserts the width.  Host only: plans are built with upload=False."""
import numpy as np
import pytest

from util import fem_plus_rmat

LDS_MAX = 20480                          # EHYB_LDS_MAX_DOUBLES
RMAT14 = ("rmat", (14, 1 << 17, 1))
RMAT17 = ("rmat", (17, 1 << 20, 3))
ALL_RESIDUAL = dict(er_mode=2, fuse_er=2, direct=2)


def host_plan(E, gen, **kw):
    cfg = E.make_config(**kw)
    m = fem_plus_rmat(E, cfg) if gen == "fem_plus_rmat" else E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
    m.reorder(cfg)
    return E.Plan(m, cfg, upload=False)


def units2(plan):
    return plan.array("pb_units2").reshape(-1, 4)


def rows_max(plan):
    return int(np.abs(units2(plan)[:, 3]).max())


def window_formula(plan):
    """min(4, (LDS bytes - 16-byte slab counter) / bytes of one window image); no window launch: 4"""
    lds_doubles = plan.stats["lds_bytes"] // 8
    if lds_doubles == 0:
        return 4
    win_cap = (lds_doubles + 1) // 2 * 2
    return max(1, min(4, (LDS_MAX * 8 - 16) // (8 * win_cap)))


def panel_formula(plan, panel_cols):
    return max(1, min(4, (LDS_MAX - 1) // panel_cols, LDS_MAX // rows_max(plan)))


@pytest.mark.parametrize("panel_cols,k", [(4096, 4), (5120, 3), (8192, 2), (16384, 1)])
def test_all_residual_plan_serves_what_its_panels_allow(E, panel_cols, k):
    plan = host_plan(E, RMAT14, lds_doubles=512, er_panel_cols=panel_cols, **ALL_RESIDUAL)
    st = plan.stats
    u2 = units2(plan)
    assert st["nnz_ell"] == 0 and st["er_partials"] > 0
    assert len(u2) == 35 and (u2[:, 3] < 0).all() and rows_max(plan) == 712          # every row block assigns
    assert plan.spmm_max_k == k == panel_formula(plan, panel_cols)


def test_the_largest_row_block_binds(E):
    """Four panel images fit, four accumulators per row of a 5,566-row block do not."""
    plan = host_plan(E, RMAT14, lds_doubles=512, er_panel_cols=4096, er_block_rows=16384, er_units2=2, **ALL_RESIDUAL)
    assert plan.stats["nnz_ell"] == 0 and plan.stats["er_partials"] > 0
    assert rows_max(plan) == 5566
    assert (LDS_MAX - 1) // 4096 == 4 and LDS_MAX // 5566 == 3
    assert plan.spmm_max_k == 3


@pytest.mark.parametrize("lds,panel_cols,k,binds", [(4096, 4096, 4, "both allow four"), (10240, 4096, 2, "the window term"),
                                                    (4096, 16384, 1, "the panel term")])
def test_windows_kept_beside_the_panel_form(E, lds, panel_cols, k, binds):
    plan = host_plan(E, "fem_plus_rmat", partitioner=1, er_mode=2, lds_doubles=lds, er_panel_cols=panel_cols)
    st = plan.stats
    u2 = units2(plan)
    assert st["nnz_ell"] > 0 and st["er_partials"] > 0 and st["lds_bytes"] > 0
    assert (u2[:, 3] < 0).any() and (u2[:, 3] > 0).any()                              # both kinds of row block
    assert plan.spmm_max_k == k == min(panel_formula(plan, panel_cols), window_formula(plan)), binds
    if binds == "the window term":
        assert window_formula(plan) == 2 and panel_formula(plan, panel_cols) == 4
    if binds == "the panel term":
        assert window_formula(plan) == 4 and panel_formula(plan, panel_cols) == 1


@pytest.mark.parametrize("lds,k", [(None, 1), (5120, 4)])
def test_a_window_that_holds_nothing_still_counts(E, lds, k):
    """er_mode = 2 forces the panel form but keeps the windows: the window launch runs (it writes the zeros the adding row blocks
    add to), so its LDS image counts although no entry is in it."""
    kw = dict(er_panel_cols=2048, **ALL_RESIDUAL)
    if lds is not None:
        kw["lds_doubles"] = lds
    plan = host_plan(E, RMAT17, **kw)
    st = plan.stats
    assert st["er_partials"] > 0
    assert st["lds_bytes"] > 0 and (units2(plan)[:, 3] > 0).any()                    # a window launch, and row blocks that add to it
    if lds is None:                                                                  # (the default window: no entry fits it, 143 items run)
        assert st["nnz_ell"] == 0 and st["lds_bytes"] == 163824
    assert panel_formula(plan, 2048) == 4
    assert plan.spmm_max_k == k == window_formula(plan)
