"""ehyb_spmm on a plan whose residual is in panel form: both panel passes k columns wide (k <= spmm_max_k), on the device.

Every path of the wide passes is checked column by column against the EXACT product (exact_cases.py: integer values and x, so
the product is one number whatever the order of the LDS adds of pass 2), for k = 1..8 (several passes where k > k_max), both
explicit walks and the plan's own alternation; every row first asserts that the plan serves the width the rule gives
(test_spmm_panel_host.py) -- which is more than 1, so that the wide kernels are what runs -- and the stats that prove the path.
Then the layout (odd leading dimensions, gaps), real data against the one-vector multiply and the CPU oracle, the non-finite
contract per column, cg_multi on a panel-form plan and the device-memory life cycle.  Everything runs in the permuted numbering."""
import ctypes as C

import numpy as np
import pytest

from exact_cases import assert_exact, exact_reference, integer_values, integer_x, nonfinite_reference, value_class
from test_gpu_cg import cpu_cg, spd_matrix
from test_gpu_cg_multi import System
from test_gpu_spmm import KS, spmm, spmv
from util import Case, fem_plus_rmat

pytestmark = pytest.mark.gpu

LDS_MAX = 20480
RMAT14 = ("rmat", (14, 1 << 17, 1))
RMAT16 = ("rmat", (16, 1 << 19, 5))
RMAT17 = ("rmat", (17, 1 << 20, 3))
ALL_RES = dict(er_mode=2, fuse_er=2, direct=2)
SMALL = dict(lds_doubles=512, **ALL_RES)          # R-MAT 2^14: no entry in a window, 35 row blocks that all assign
KEPT = dict(partitioner=1, er_mode=2, lds_doubles=4096, er_panel_cols=4096)    # fem_plus_rmat: windows kept, both kinds of row block


def units2(plan):
    return plan.array("pb_units2").reshape(-1, 4)


def rule(plan, panel_cols):
    """ehyb_spmm_max_k of a panel-form plan, from what the plan reports (include/ehyb.h)"""
    rows_max = int(np.abs(units2(plan)[:, 3]).max())
    k = min(4, (LDS_MAX - 1) // panel_cols, LDS_MAX // rows_max)
    lds_doubles = plan.stats["lds_bytes"] // 8
    if lds_doubles:
        k = min(k, (LDS_MAX * 8 - 16) // (8 * ((lds_doubles + 1) // 2 * 2)))
    return max(1, k)


class IntCase:
    """matrix -> integer values -> reorder; k integer columns (seeds 1..k) in the permuted numbering and their exact products"""

    def __init__(self, E, gen, cfg, k=max(KS)):
        if gen == "fem_plus_rmat":
            m = fem_plus_rmat(E, cfg)
        elif gen == "fem_plus_rmat_odd":
            m = fem_plus_rmat(E, cfg, fem_rows=29997)
        else:
            m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
        m.V[:] = integer_values(m.I, m.J, False)
        m.reorder(cfg)
        self.m, self.n = m, m.n
        self.X = np.stack([integer_x(m.n, j + 1) for j in range(k)])
        self.Y = np.stack([exact_reference(m.n, m.I, m.J, m.V, x) for x in self.X])


def all_assign(p):
    return p.stats["nnz_ell"] == 0 and bool((units2(p)[:, 3] < 0).all())


def n_items(p):
    return len(p.array("pb_items1")) // 2


# (id, matrix, config, panel columns of the config, k_max, what the stats must show)
PATHS = [
    ("all-residual-k4", RMAT14, dict(er_panel_cols=4096, **SMALL), 4096, 4, all_assign),
    ("all-residual-k3", RMAT14, dict(er_panel_cols=5120, **SMALL), 5120, 3, all_assign),
    ("all-residual-k2", RMAT14, dict(er_panel_cols=8192, **SMALL), 8192, 2, all_assign),
    ("pass1-512-threads", RMAT14, dict(er_panel_cols=2048, er_panel_threads=512, **SMALL), 2048, 4, all_assign),
    ("pass1-1024-threads", RMAT14, dict(er_panel_cols=2048, er_panel_threads=1024, **SMALL), 2048, 4, all_assign),
    # more items than the 512 resident workgroups of a 512-thread pass 1: the per-XCD queues run
    ("xcd-queues", RMAT17, dict(er_queue=1, er_units1=3000, er_panel_cols=2048, lds_doubles=5120, **ALL_RES), 2048, 4,
     lambda p: p.stats["er_partials"] > 0 and n_items(p) > 512),
    ("few-fat-items", RMAT16, dict(er_units1=7, er_panel_cols=1024, **ALL_RES), 1024, 4,
     lambda p: p.stats["er_partials"] > 0 and p.stats["nnz_ell"] == 0 and n_items(p) <= 8),
    ("windows-kept-add-and-assign", "fem_plus_rmat", KEPT, 4096, 4,
     lambda p: p.stats["nnz_ell"] > 0 and p.stats["er_partials"] > 0 and bool((units2(p)[:, 3] < 0).any()) and bool((units2(p)[:, 3] > 0).any())),
    # 62,765 columns: odd, and no multiple of the panel width -- the last panel is short and ends on an odd column
    ("odd-columns-short-last-panel", "fem_plus_rmat_odd", KEPT, 4096, 4,
     lambda p: p.n == 62765 and p.stats["nnz_ell"] > 0 and p.stats["er_partials"] > 0),
    ("many-small-row-blocks", RMAT14, dict(er_panel_cols=4096, er_block_rows=64, **SMALL), 4096, 4,
     lambda p: all_assign(p) and len(units2(p)) >= 153),
    # pass 2 with its LDS nearly full: 3 accumulators per row of a 5,566-row block
    ("5566-row-block-k3", RMAT14, dict(er_panel_cols=4096, er_block_rows=16384, er_units2=2, **SMALL), 4096, 3,
     lambda p: all_assign(p) and int(np.abs(units2(p)[:, 3]).max()) == 5566),
]


@pytest.mark.parametrize("name,gen,kw,panel_cols,kmax,taken", PATHS, ids=[p[0] for p in PATHS])
def test_exact_every_path(E, gpu, name, gen, kw, panel_cols, kmax, taken):
    cfg = E.make_config(**kw)
    c = IntCase(E, gen, cfg)
    plan = E.Plan(c.m, cfg)
    assert taken(plan), (name, plan.stats)
    assert plan.spmm_max_k == kmax == rule(plan, panel_cols) and kmax > 1, (name, plan.spmm_max_k)
    for k in KS:
        for walk in (0, 1, None, None):            # (None twice: two successive multiplies of the plan's own alternation)
            Y = spmm(E, plan, c.X[:k], walk=walk)
            for j in range(k):
                assert_exact(Y[j], c.Y[j], f"{name} k={k} walk={walk} column {j}")
    plan.destroy()


def test_device_and_host_built_panel_forms_give_the_same_columns(E, gpu):
    kw = dict(er_panel_cols=4096, lds_doubles=2048, **ALL_RES)
    cfg0 = E.make_config(symbolic=0, **kw)
    c = IntCase(E, ("rmat", (15, 1 << 18, 1)), cfg0, k=5)
    dev = E.Plan(c.m, cfg0, upload=True)
    host = E.Plan(c.m, E.make_config(symbolic=1, **kw))
    for plan in (dev, host):
        assert plan.stats["er_partials"] > 0
        assert plan.spmm_max_k == 4 == rule(plan, 4096)
    assert dev.stats["er_partials"] == host.stats["er_partials"]
    for k in (4, 5):
        for walk in (0, 1):
            Yd, Yh = spmm(E, dev, c.X[:k], walk=walk), spmm(E, host, c.X[:k], walk=walk)
            for j in range(k):
                assert_exact(Yd[j], c.Y[j], f"device-built k={k} walk={walk} column {j}")
                assert_exact(Yh[j], c.Y[j], f"host-built k={k} walk={walk} column {j}")


@pytest.mark.parametrize("name,gen,kw", [("all-residual", RMAT14, dict(er_panel_cols=4096, **SMALL)), ("windows-kept", "fem_plus_rmat", KEPT)],
                         ids=lambda v: v if isinstance(v, str) and "-" in v else None)
def test_layout_gaps_and_odd_leading_dimensions(E, gpu, name, gen, kw):
    """ldx = n + 7, ldy = n + 5 with n even: both odd, so columns 1 and 3 of X and of Y are not 16-byte aligned.  NaN in every
    gap of X and Y: the gaps of Y stay, every column is exact."""
    cfg = E.make_config(**kw)
    c = IntCase(E, gen, cfg, k=4)
    plan = E.Plan(c.m, cfg)
    n = c.n
    assert plan.spmm_max_k == 4 and plan.stats["er_partials"] > 0
    assert (n + 7) % 2 == 1, "the case is built for an odd ldx"
    for k in (2, 3, 4):
        for walk in (0, 1):
            Y = spmm(E, plan, c.X[:k], ldx=n + 7, ldy=n + 5, walk=walk)
            assert np.isnan(Y[:, n:]).all(), "a gap of Y was written"
            for j in range(k):
                assert_exact(Y[j, :n], c.Y[j], f"{name} k={k} walk={walk} column {j}")


@pytest.mark.parametrize("name,gen,kw", [("all-residual", RMAT14, dict(er_panel_cols=4096, **SMALL)), ("windows-kept", "fem_plus_rmat", KEPT)],
                         ids=lambda v: v if isinstance(v, str) and "-" in v else None)
def test_real_data_against_the_one_vector_multiply_and_the_cpu(E, O, gpu, name, gen, kw):
    """The order of the LDS adds of pass 2 is free at every width: a column of a k = 4 multiply agrees with ehyb_spmv of that
    column on the same plan, and with the CPU product, within the project's tolerance relative to sum_j |a_ij x_j| (rows whose
    scale is zero must be exactly zero: check_strict flags them otherwise)."""
    cfg = E.make_config(**kw)
    c = Case(E, O, None, None, cfg, matrix=fem_plus_rmat(E, cfg)) if gen == "fem_plus_rmat" else Case(E, O, *gen, cfg)
    plan = E.Plan(c.m, cfg)
    assert plan.spmm_max_k == 4 and plan.stats["er_partials"] > 0
    rng = np.random.default_rng(9)
    X = np.stack([c.xp] + [rng.uniform(-1, 1, c.n) for _ in range(3)])
    for walk in (0, 1):
        Y = spmm(E, plan, X, walk=walk)
        for j in range(4):
            y1 = spmv(E, plan, X[j], walk)
            scale = O.abs_rowsum(c.n, c.m.I, c.m.J, c.m.V, X[j])      # (c.m was reordered in place: the permuted numbering)
            bad, worst = O.check_strict(Y[j], y1, scale, O.TOLERANCE)
            assert bad == 0, f"{name} walk={walk} column {j} against ehyb_spmv: {bad} rows, worst {worst:.3e}"
            bad, worst = O.check_strict(Y[j], O.spmv_coo(c.n, c.m.I, c.m.J, c.m.V, X[j]), scale, O.TOLERANCE)
            assert bad == 0, f"{name} walk={walk} column {j} against the CPU product: {bad} rows, worst {worst:.3e}"
        bad, worst = c.check(Y[0])
        assert bad == 0, f"{name} walk={walk} column 0 against the original numbering's product: worst {worst:.3e}"


def test_nonfinite_x_reaches_its_own_column_and_rows_only(E, gpu):
    """A plan WITHOUT windows ("the padding of the panel form reads nothing"): NaN / +inf / -inf in X[c, 1] -- exactly the rows of
    column 1 that store column c are non-finite, of the class the products give; every other row and column is the exact product."""
    cfg = E.make_config(er_panel_cols=4096, **SMALL)
    c = IntCase(E, RMAT14, cfg, k=4)
    plan = E.Plan(c.m, cfg)
    assert all_assign(plan) and plan.spmm_max_k == 4
    rng = np.random.default_rng(11)
    X = c.X[:4].copy()
    cols = np.unique(np.concatenate([[0], rng.choice(np.arange(1, c.n), 6, replace=False)]))
    X[1, cols] = np.resize([np.nan, np.inf, -np.inf], len(cols))
    y_ref = nonfinite_reference(c.n, c.m.I, c.m.J, c.m.V, X[1])
    stores = np.zeros(c.n, dtype=bool)
    stores[c.m.I[np.isin(c.m.J, cols)]] = True
    assert stores.any() and np.array_equal(stores, ~np.isfinite(y_ref))
    for walk in (0, 1):
        Y = spmm(E, plan, X, walk=walk)
        for j in (0, 2, 3):
            assert_exact(Y[j], c.Y[j], f"walk={walk}: column {j} was reached from column 1")
        assert np.array_equal(value_class(Y[1]), value_class(y_ref)), f"walk={walk}: not the rows that store such a column"
        assert_exact(Y[1], y_ref, f"walk={walk} column 1")


@pytest.mark.parametrize("graphs", [0, 2])
@pytest.mark.parametrize("k", [4, 5])
def test_cg_multi_on_a_panel_form_plan(E, O, gpu, k, graphs):
    """An SPD system forced into panel form beside a small reference window; every column converges and meets what the symmetric
    pair plan is held to (the other storage whose order of summation is free)."""
    s = System(E, spd_matrix(120, 100, 3000, 1), sym_pairs=0, er_mode=2, fuse_er=2, direct=2, window_mode=1, lds_doubles=256,
               er_panel_cols=4096, graphs=graphs)
    st = s.plan.stats
    assert s.plan.spmm_max_k == 4
    assert st["er_partials"] > 0 and st["nnz_ell"] > 0, st
    rng = np.random.default_rng(3)
    bs = [O.x_glibc(s.n) + 0.3, s.A @ np.ones(s.n), rng.uniform(-1, 1, s.n), rng.uniform(0, 2, s.n), s.A @ np.linspace(-1, 1, s.n)][:k]
    B = np.stack([E.vector_reorder(b, s.perm) for b in bs])
    X, iters, rel = s.plan.cg_multi(B, max_iter=400, rtol=1e-10, check_every=1)
    for j, b in enumerate(bs):
        x = E.vector_recover(X[j], s.perm)
        x_cpu, it_cpu, _ = cpu_cg(s.A, b, 400, 1e-10)
        assert rel[j] <= 1e-10 and abs(iters[j] - it_cpu) <= 2, (j, iters[j], it_cpu, rel[j])
        assert np.linalg.norm(s.A @ x - b) <= 2e-10 * np.linalg.norm(b), j
        assert np.linalg.norm(x - x_cpu) <= 1e-8 * np.linalg.norm(x_cpu), j


def test_a_wide_panel_plan_gives_its_memory_back(E, gpu):
    """The partial-sum buffer of a k_max = 4 plan is four times a one-vector plan's: upload and destroy six times, the device has
    what it had before (six leaked buffers would be far more than the slack allowed)."""
    lib = E.host._lib.load()

    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        lib.ehyb_dev_sync()
        assert lib.ehyb_dev_mem_info(C.byref(f), C.byref(t)) == 0
        return f.value

    cfg = E.make_config(er_panel_cols=2048, lds_doubles=5120, **ALL_RES)
    m = E.Matrix.generate(*RMAT17[:1], *RMAT17[1], cfg=cfg)
    m.reorder(cfg)
    E.Plan(m, cfg).destroy()                     # first use: kernels loaded
    free0 = free_bytes()
    for _ in range(6):
        plan = E.Plan(m, cfg, upload=False)
        assert plan.spmm_max_k == 4
        assert 6 * 4 * 8 * plan.stats["er_partials"] > (32 << 20)
        before = free_bytes()
        plan.upload()
        assert free_bytes() <= before - 4 * 8 * plan.stats["er_partials"]
        plan.destroy()
    free1 = free_bytes()
    assert free0 - free1 < (32 << 20), (free0, free1)
