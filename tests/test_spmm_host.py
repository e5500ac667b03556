"""ehyb_spmm / ehyb_spmm_max_k on the host: the width a plan serves in one pass over the matrix, worked out from its host
layout, and the argument checks of the k-vector multiply -- everything that does not need a device."""
import ctypes as C

import pytest

LDS_MAX = 20480                          # EHYB_LDS_MAX_DOUBLES
ERR_ARG, ERR_STATE = 1, 8                # EHYB_ERR_ARG, EHYB_ERR_STATE
FEM = ("fem3d", (90000, 3, 30, 30, 13500, 1, 1))
FEM_SMALL = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))


def host_plan(E, gen, **kw):
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
    m.reorder(cfg)
    return E.Plan(m, cfg, upload=False)


def window_formula(plan):
    """min(4, (LDS bytes - 16-byte slab counter) / bytes of one window image)"""
    lds_doubles = plan.stats["lds_bytes"] // 8
    win_cap = (lds_doubles + 1) // 2 * 2
    return min(4, (LDS_MAX * 8 - 16) // (8 * win_cap))


# Plans with the default lds_doubles whose windows fill the LDS: partitions of a whole window of own rows (reference window
# mode), and symmetric pair storage where the halo columns fill it (the default sizing makes mid-size matrices' windows small).
DEFAULT_FULL = [
    ("plain", FEM_SMALL, dict(window_mode=1)),
    ("sym", ("rmat", (15, 1 << 21, 1)), dict(sym_pairs=1, direct=2)),
]


@pytest.mark.parametrize("name,gen,kw", DEFAULT_FULL, ids=[d[0] for d in DEFAULT_FULL])
def test_default_window_plan_serves_one_vector(E, name, gen, kw):
    plan = host_plan(E, gen, **kw)
    st = plan.stats
    assert st["nnz_ell"] > 0 and st["er_partials"] == 0
    assert (st["sym_pairs"] > 0) == (name == "sym")
    assert st["lds_bytes"] > LDS_MAX * 8 // 2          # more than half the LDS: no second image fits
    assert plan.spmm_max_k == 1 == window_formula(plan)


@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_window_plan_built_for_k_serves_k(E, k, sym):
    """cfg.lds_doubles = EHYB_LDS_MAX_DOUBLES / k: the partitions are sized so that k window images fit the LDS."""
    plan = host_plan(E, FEM, sym_pairs=sym, direct=2, lds_doubles=LDS_MAX // k)
    st = plan.stats
    assert st["nnz_ell"] > 0 and st["er_partials"] == 0 and (st["sym_pairs"] > 0) == bool(sym)
    assert plan.spmm_max_k >= k
    assert plan.spmm_max_k == window_formula(plan)


def test_direct_shape_serves_four(E):
    plan = host_plan(E, FEM_SMALL, direct=1)
    st = plan.stats
    assert st["nnz_ell"] == 0 and st["nnz_er"] == st["nnz"] and st["er_segments"] == st["n_rows"]
    assert plan.spmm_max_k == 4


def test_panel_residual_serves_one_vector(E):
    plan = host_plan(E, ("rmat", (14, 1 << 17, 1)), er_mode=2, fuse_er=2, direct=2, lds_doubles=512)
    assert plan.stats["er_partials"] > 0
    assert plan.spmm_max_k == 1


def test_max_k_null_arguments(E):
    lib = E.host._lib.load()
    k = C.c_int(0)
    assert lib.ehyb_spmm_max_k(None, C.byref(k)) == ERR_ARG
    assert lib.ehyb_last_error()
    plan = host_plan(E, FEM_SMALL, direct=1)
    assert lib.ehyb_spmm_max_k(plan.h, None) == ERR_ARG
    assert lib.ehyb_last_error()


def test_spmm_argument_and_state_errors(E):
    """Argument errors are reported first, then the missing upload; nothing is dereferenced on either path."""
    lib = E.host._lib.load()
    plan = host_plan(E, FEM_SMALL, lds_doubles=LDS_MAX // 4, direct=2)
    n = plan.n
    X, Y = C.c_void_p(0x10000), C.c_void_p(0x20000)   # never read: every call below fails before any device work

    def call(h=plan.h, x=X, ldx=n, y=Y, ldy=n, k=2, walk=-1):
        rc = lib.ehyb_spmm(h, x, ldx, y, ldy, k, None, walk)
        return rc, lib.ehyb_last_error()

    rc, msg = call()
    assert rc == ERR_STATE and b"upload" in msg
    for bad in (dict(k=0), dict(k=-3), dict(ldx=n - 1), dict(ldy=n - 1), dict(x=None), dict(y=None), dict(h=None), dict(walk=2)):
        rc, msg = call(**bad)
        assert rc == ERR_ARG, bad
        assert msg, bad
    rc, _ = call(ldx=n + 7, ldy=n + 5, k=9, walk=1)     # wide leading dimensions are fine: only the upload is missing
    assert rc == ERR_STATE
    with pytest.raises(E.EhybError) as ei:
        plan.spmm(X.value, Y.value, 3)
    assert "ehyb_spmm" in str(ei.value) and "status 8" in str(ei.value)
