"""ehyb_spmv_t against the EXACT transposed product: the cases and machinery of test_gpu_exact.py (integer values and x: the
product is one number in fp64 whatever the order of the LDS and global atomic adds), always with UNSYMMETRIC values -- with
symmetric values the forward kernel would pass.  The reference is exact_reference with rows and columns swapped, computed in the
permuted numbering; every case asserts that it differs from the forward product.  y is filled with NaN before every multiply (the
call must assign it) and compared with assert_exact.  Every case asserts the path it names and the rows of E.kernel_table_t() it
launches (spmv_t_cases.py says which case launches which row).  The second half pins the non-finite contract under ehyb_spmv_t
in ehyb.h, and one solve shows the multiply captured in a hipGraph."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from exact_cases import assert_exact, exact_reference, integer_values, integer_x, nonfinite_reference, value_class
from spmv_t_cases import EXTRA_PATHS, FUZZ_SEEDS, NAMED, REFUSED, fuzz_case, nodes_and_pairs
from test_col_triples import device_cols
from test_gpu_exact import _BY_NAME, NONFINITE_PATHS, PATHS, ExactCase, _plant, _sync, is_direct
from test_gpu_gmres import RTOL, System, cd_matrix, rhs

pytestmark = pytest.mark.gpu

ERR_ARG = 1
NO_FORWARD_LAUNCH = dict(window=set(), panel=set(), er_csr=set())


class TCase(ExactCase):
    """ExactCase with unsymmetric values, and the exact A^T x beside the exact A x (both in the permuted numbering)"""

    def __init__(self, E, O, gen, cfg, salt=0):
        super().__init__(E, O, gen, cfg, symmetric=False, salt=salt)
        m = self.m
        self.yt_ref_p = exact_reference(m.n, m.J, m.I, m.V, self.xp, O)
        assert (self.yt_ref_p != self.y_ref_p).sum() > self.n // 2, "the transposed product must differ from the forward one"


def multiply_t(E, plan, xp, times=1):
    """`times` transposed multiplies through plan.spmv_t, each into a y filled with NaN -> the y of each (permuted numbering)"""
    n = len(xp)
    dx, dy = E.DeviceBuffer(n).upload(xp), E.DeviceBuffer(n)
    out = []
    for _ in range(times):
        dy.upload(np.full(n, np.nan))
        plan.spmv_t(dx.ptr, dy.ptr)
        _sync(E)
        out.append(dy.download())
    dx.free(), dy.free()
    return out


def odd_start_with_a_ragged_last_slab(plan):
    """partitions that start at an odd row (win[0] is the row before: never flushed) and whose last slab has lanes without rows"""
    pb, slab_row, slab_part = plan.array("part_boundary"), plan.array("slab_row"), plan.array("slab_part")
    last = {int(p): int(r) for p, r in zip(slab_part, slab_row)}        # (slabs ascend: the last slab of every partition stays)
    return [p for p in range(len(pb) - 1) if pb[p] & 1 and p in last and last[p] + 64 > pb[p + 1]]


# named paths with such a partition (asserted below from part_boundary and slab_row)
ODD_START = {"refwindow-t256-lds1024", "halo-t512-lds64", "halo-t1024-lds20480", "relative-columns"}

NAMED_CASES = [(p[0], p[1], p[2], p[4], NAMED[p[0]]) for p in PATHS if p[0] in NAMED] + EXTRA_PATHS


def test_every_named_path_of_the_issue_is_a_path_of_test_gpu_exact():
    assert {p[0] for p in PATHS} >= set(NAMED) and len(NAMED_CASES) == len(NAMED) + len(EXTRA_PATHS)


@pytest.mark.parametrize("name,gen,kw,taken,rows", NAMED_CASES, ids=[c[0] for c in NAMED_CASES])
def test_exact_named_path(E, O, gpu, name, gen, kw, taken, rows):
    cfg = E.make_config(**kw)
    c = TCase(E, O, gen, cfg)
    plan = E.Plan(c.m, cfg)
    assert taken(plan, c.n), (name, plan.stats)
    assert plan.spmv_t_supported and plan.stats["nnz_ell"] + plan.stats["nnz_er"] == c.m.nnz
    if name in ODD_START:
        assert odd_start_with_a_ragged_last_slab(plan), name
    plan.launched_clear()
    for k, y in enumerate(multiply_t(E, plan, c.xp, times=2)):
        assert_exact(y, c.yt_ref_p, f"{name} multiply {k}")
    assert plan.launched_t() == rows, (name, plan.launched_t())
    assert plan.launched() == NO_FORWARD_LAUNCH
    plan.launched_clear()
    assert plan.launched_t() == set()
    # the forward multiply of the same plan is what it was, and logs in its own tables only
    dx, dy = E.DeviceBuffer(c.n).upload(c.xp), E.DeviceBuffer(c.n).upload(np.full(c.n, np.nan))
    plan.spmv(dx.ptr, dy.ptr)
    _sync(E)
    assert_exact(dy.download(), c.y_ref_p, f"{name} forward")
    assert plan.launched_t() == set() and plan.launched() != NO_FORWARD_LAUNCH
    dx.free(), dy.free()
    plan.destroy()


# ---------------------------------------------------------------------------------------------- triple-coded column words
def _coded_pairs_mod3(plan):
    _, dmeta = device_cols(plan)
    coded = (dmeta[:, 3] & 0x40) != 0
    return set(((dmeta[coded, 3] >> 16) % 3).tolist())


@pytest.mark.parametrize("arm", [0, 2], ids=["triple-coded", "pair-form"])
def test_fem_with_and_without_triple_words(E, O, gpu, arm):
    """FEM (3 unknowns per node) under cfg.ell_triples 0 (= on: coded slabs, of 3 k and 3 k + 2 pairs -- rows of whole node triples
    never give 3 k + 1) and 2 (the host's pair words): both exact"""
    kw = dict(lds_doubles=4096, direct=2)
    cfg = E.make_config(ell_triples=arm, **kw)
    c = TCase(E, O, _BY_NAME["halo-t1024-lds20480"][1], cfg)
    plan = E.Plan(c.m, cfg)
    words, col_words = int(plan.lib.ehyb_plan_device_col_words(plan.h)), plan.stats["col_words"]
    if arm == 0:
        assert words < 0.9 * col_words and _coded_pairs_mod3(plan) == {0, 2}
    else:
        assert words == col_words and _coded_pairs_mod3(plan) == set()
    for k, y in enumerate(multiply_t(E, plan, c.xp, times=2)):
        assert_exact(y, c.yt_ref_p, f"ell_triples={arm} multiply {k}")
    plan.destroy()


def test_triple_words_for_one_two_and_three_pairs_and_odd_starts(E, O, gpu):
    """nodes_and_pairs (spmv_t_cases.py): coded slabs of 1, 2 and 6 pairs -- pairs % 3 of 1, 2 and 0: the whole-word steps and
    both tails of the triple arm --, partitions with an odd start and lanes without rows"""
    cfg = E.make_config(lds_doubles=1024, direct=2)
    indptr, indices = nodes_and_pairs()
    I = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    m = E.Matrix.from_csr(indptr, indices, integer_values(I, indices, False), cfg)
    m.reorder(cfg)
    plan = E.Plan(m, cfg)
    assert int(plan.lib.ehyb_plan_device_col_words(plan.h)) < 0.9 * plan.stats["col_words"]
    assert _coded_pairs_mod3(plan) == {0, 1, 2}
    assert odd_start_with_a_ragged_last_slab(plan)
    xp = integer_x(m.n, 3)
    yt = exact_reference(m.n, m.J, m.I, m.V, xp, O)
    assert (yt != exact_reference(m.n, m.I, m.J, m.V, xp)).sum() > m.n // 2
    for k, y in enumerate(multiply_t(E, plan, xp, times=2)):
        assert_exact(y, yt, f"nodes and pairs, multiply {k}")
    plan.destroy()


# ---------------------------------------------------------------------------------------------- fuzz seeds
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_exact_random_plan(E, O, gpu, seed):
    """the seeds of test_gpu_exact.test_exact_random_plan that draw a served plan, as drawn and with ell_alternate = 1: two
    multiplies each"""
    for more in ({}, dict(ell_alternate=1)):
        m, cfg, xp, yt = fuzz_case(E, O, seed, **more)
        plan = E.Plan(m, cfg)
        assert plan.spmv_t_supported, (seed, plan.spmv_t_refusal)
        for k, y in enumerate(multiply_t(E, plan, xp, times=2)):
            assert_exact(y, yt, f"seed {seed} {more} multiply {k}")
        plan.destroy()


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("name,gen,kw,words", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_leave_y_alone(E, O, gpu, name, gen, kw, words):
    cfg = E.make_config(**kw)
    c = ExactCase(E, O, gen, cfg, symmetric=False)
    plan = E.Plan(c.m, cfg)
    assert not plan.spmv_t_supported
    dx, dy = E.DeviceBuffer(c.n).upload(c.xp), E.DeviceBuffer(c.n).upload(np.full(c.n, np.nan))
    with pytest.raises(E.EhybError) as ei:
        plan.spmv_t(dx.ptr, dy.ptr)
    assert ei.value.code == ERR_ARG and words in str(ei.value), str(ei.value)
    _sync(E)
    assert np.isnan(dy.download()).all() and plan.launched_t() == set()
    dx.free(), dy.free()
    plan.destroy()


def test_x_equal_y_is_refused_on_a_served_plan(E, O, gpu):
    cfg = E.make_config(lds_doubles=4096, direct=2)
    c = TCase(E, O, _BY_NAME["halo-t1024-lds20480"][1], cfg)
    plan = E.Plan(c.m, cfg)
    dx = E.DeviceBuffer(c.n).upload(c.xp)
    with pytest.raises(E.EhybError) as ei:
        plan.spmv_t(dx.ptr, dx.ptr)
    assert ei.value.code == ERR_ARG and "same vector" in str(ei.value)
    _sync(E)
    assert np.array_equal(dx.download(), c.xp) and plan.launched_t() == set()
    dx.free()
    plan.destroy()


# ---------------------------------------------------------------------------------------------- non-finite values
NONFINITE_T = [n for n in NONFINITE_PATHS if n in NAMED]


def test_the_nonfinite_paths_are_the_served_ones():
    assert NONFINITE_T == ["refwindow-t256-lds1024", "halo-t1024-lds20480", "inline-residual", "csr-split-16", "direct-rmat",
                           "relative-columns"]


@pytest.mark.parametrize("name", NONFINITE_T)
def test_nonfinite_matrix_values(E, O, gpu, name):
    """NaN / +inf / -inf in A, finite x: every COLUMN's class (finite, NaN, +inf, -inf) as in the exact transposed product, and
    every finite column bit-exact: a non-finite value reaches exactly the columns of the rows that store it"""
    _, gen, kw, _, taken = _BY_NAME[name]
    cfg = E.make_config(value_map=1, **kw)
    c = TCase(E, O, gen, cfg)
    probe = E.Plan(c.m, cfg, upload=False)
    picks = _plant(probe, c, np.random.default_rng(7))
    probe.destroy()
    plan = E.Plan(c.m, cfg)
    assert taken(plan, c.n), (name, plan.stats)
    y_ref = nonfinite_reference(c.n, c.m.J, c.m.I, c.m.V, c.xp)
    assert (value_class(y_ref) != 0).sum() >= 2, "the planted values must reach the product"
    for k, y in enumerate(multiply_t(E, plan, c.xp, times=2)):
        assert np.array_equal(value_class(y), value_class(y_ref)), (name, k, picks)
        assert_exact(y, y_ref, f"{name} multiply {k}")
    plan.destroy()


@pytest.mark.parametrize("name", NONFINITE_T)
def test_nonfinite_x(E, O, gpu, name):
    """NaN / +inf / -inf in x: every column that a non-finite row stores comes out non-finite (a NaN is never lost; an inf may turn
    NaN), every other column is the exact product -- or NaN, through padding slots (value 0.0) of that row, which add 0 * inf or
    0 * NaN to columns 0-2 of the row's window, to the row's own column (relative columns) or to y[0] (inline residual).  Those
    columns are counted."""
    _, gen, kw, _, taken = _BY_NAME[name]
    cfg = E.make_config(**kw)
    c = TCase(E, O, gen, cfg)
    plan = E.Plan(c.m, cfg)
    rng = np.random.default_rng(11)
    xp = c.xp.copy()
    rows = np.unique(np.concatenate([[0], rng.choice(np.arange(1, c.n), 6, replace=False)]))
    xp[rows] = np.resize([np.nan, np.inf, -np.inf], len(rows))
    y_ref = nonfinite_reference(c.n, c.m.J, c.m.I, c.m.V, xp)
    stores = np.zeros(c.n, dtype=bool)
    stores[c.m.J[np.isin(c.m.I, rows)]] = True
    assert stores.sum() >= 6 and np.array_equal(~np.isfinite(y_ref), stores)
    for k, y in enumerate(multiply_t(E, plan, xp, times=2)):
        assert not np.isfinite(y[stores]).any(), (name, k, "a non-finite x was lost")
        assert np.isnan(y[stores & np.isnan(y_ref)]).all(), (name, k, "a NaN turned into something else")
        other = ~stores
        ok = (y[other] == y_ref[other]) | np.isnan(y[other])
        assert ok.all(), (name, k, "a column that no non-finite row stores is neither exact nor NaN")
        # at most three window columns, the own column and y[0] per non-finite row
        assert int(np.isnan(y[other]).sum()) <= 5 * len(rows), (name, k, int(np.isnan(y[other]).sum()))
        print(f"{name} multiply {k}: {int(np.isnan(y[other]).sum())} of {int(other.sum())} columns that no non-finite row "
              f"stores came out NaN (padding)")
    plan.destroy()


# ---------------------------------------------------------------------------------------------- captured in a hipGraph
def test_the_multiply_captured_in_a_graph(E, gpu):
    """gmres_t captures every cycle -- memset node and launches of ehyb_spmv_t included -- into one hipGraph (cfg.graphs default);
    cfg.graphs = 2 issues the same launches plainly.  The adds arrive in any order, so both are held to the same tolerances, not
    compared bit for bit."""
    A = cd_matrix(120, 100, 3000, 6)
    kw = dict(window_mode=2, lds_doubles=2048, sym_pairs=0)
    s = System(E, A, **kw)
    plain = E.Plan(s.m, E.make_config(graphs=2, **kw))
    b = rhs(s.n)
    bp = E.vector_reorder(b, s.perm)
    x_ref = spla.spsolve(A.T.tocsc(), b)
    for what, plan in (("graph", s.plan), ("plain launches", plain)):
        plan.launched_clear()
        xp, it, rel = plan.gmres_t(bp, restart=10, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag)
        x = E.vector_recover(xp, s.perm)
        assert 10 < it < 2000 and rel <= RTOL, (what, it, rel)                       # (more than one cycle: the graph was replayed)
        assert np.linalg.norm(b - A.T @ x) <= 10 * RTOL * np.linalg.norm(b), what
        assert np.linalg.norm(x - x_ref) <= 1e-6 * np.linalg.norm(x_ref), what
        assert plan.launched_t() and plan.launched() == NO_FORWARD_LAUNCH, what
    plain.destroy()
