"""cfg.ell_triples on the device: the window kernels read one column base per node triple where ehyb_plan_upload coded a slab
(csrc/col_triples.h; the form itself is decoded on the CPU in test_col_triples.py).  The entry order and the accumulators are
those of the pair form, so plain storage gives the same bits with the switch on (0) and off (2), and symmetric pairs give the
exact product on integer data (exact_cases.py) in both arms -- for one vector and ehyb_spmm with k = 1..4, both walk directions,
after a refill, from a captured graph and inside a CG solve."""
import numpy as np
import pytest
import scipy.sparse as sp

from exact_cases import assert_exact, exact_reference, integer_values, integer_x
from test_col_triples import FEM6, FEM24, WIDE, WIDE_KW, make_matrix

pytestmark = pytest.mark.gpu

# (id, generator, configuration): slabs of 11..48 pairs with every tail (fem3d), and of 2, 5 and 6 pairs (nodes)
CASES = [
    ("fem6000", FEM6, dict(lds_doubles=1024)),
    ("fem24000", FEM24, dict(lds_doubles=4096)),
    ("nodes", ("nodes", (2048,)), dict(lds_doubles=1024, direct=2)),
    # the kernels with the inline residual in them, on a plan with coded slabs (plain storage, k = 1..4)
    ("fem6000-inline", FEM6, dict(lds_doubles=1024, fuse_er=1)),
]
# the same with symmetric pairs: k = 1..3 (the plan's widest pass; a plan that can take four keeps the pair form whole)
WIDE_CASE = ("wide-inline", WIDE, {k: v for k, v in WIDE_KW.items() if k != "sym_pairs"})
ARMS = (0, 2)


def _sync(E):
    assert E.host._lib.load().ehyb_dev_sync() == 0


def _coded_words(plan):
    return int(plan.lib.ehyb_plan_device_col_words(plan.h))


def _products(E, plan, X):
    """X (4, n) permuted -> {(k, walk): Y}: one vector through ehyb_spmv_walk, k = 1..4 (or the plan's widest pass) through
    ehyb_spmm, both directions; y is NaN before every multiply."""
    kmax, n = min(X.shape[0], plan.spmm_max_k), X.shape[1]
    X = X[:kmax]
    dx = E.DeviceBuffer(kmax * n).upload(X.ravel())
    dy = E.DeviceBuffer(kmax * n)
    out = {}
    for walk in (0, 1):
        dy.upload(np.full(kmax * n, np.nan))
        plan.spmv(dx.ptr, dy.ptr, walk=walk)
        _sync(E)
        out[(0, walk)] = dy.download()[:n].copy()
        for k in range(1, kmax + 1):
            dy.upload(np.full(kmax * n, np.nan))
            plan.spmm(dx.ptr, dy.ptr, k, walk=walk)
            _sync(E)
            out[(k, walk)] = dy.download().reshape(kmax, n)[:k].copy()
    dx.free(), dy.free()
    return out


def _plans(E, m, kw, **more):
    """the matrix under both arms -> {arm: plan}; the arm that is on must have coded slabs"""
    plans = {}
    for arm in ARMS:
        cfg = E.make_config(ell_triples=arm, **kw, **more)
        assert cfg.ell_triples == (2 if arm == 2 else 1)
        plans[arm] = E.Plan(m, cfg)
    st = plans[0].stats
    assert plans[2].stats == st and st["nnz_ell"] > 0
    assert _coded_words(plans[2]) == st["col_words"] and _coded_words(plans[0]) < 0.9 * st["col_words"]
    return plans


@pytest.mark.parametrize("name,gen,kw", CASES, ids=[c[0] for c in CASES])
def test_plain_storage_gives_the_same_bits_in_both_arms(E, O, gpu, name, gen, kw):
    cfg = E.make_config(**kw)
    m = make_matrix(E, gen, cfg)
    n = m.n
    x = O.x_glibc(n)
    y_ref, scale = O.spmv_coo(n, m.I, m.J, m.V, x), O.abs_rowsum(n, m.I, m.J, m.V, x)
    m.reorder(cfg)
    perm = m.reorder_list.copy()
    X = np.stack([E.vector_reorder(np.roll(x, 7 * j) * (1.0 + j), perm) for j in range(4)])
    plans = _plans(E, m, kw)
    assert plans[0].stats["sym_pairs"] == 0 and plans[0].spmm_max_k == 4
    assert plans[0].stats["er_inline"] > 0 or "inline" not in name
    got = {arm: _products(E, plans[arm], X) for arm in ARMS}
    assert O.check_strict(E.vector_recover(got[2][(0, 0)], perm), y_ref, scale)[0] == 0
    for key in got[2]:
        assert np.array_equal(got[0][key], got[2][key]), key
        if key[0]:                                           # column 0 of a plain k-wide multiply is the one-vector multiply
            assert np.array_equal(got[0][key][0], got[0][(0, key[1])]), key
    for p in plans.values():
        p.destroy()


# (the nodes pattern is not symmetric: plain storage only)
EXACT = [(c, 0) for c in CASES] + [(c, 1) for c in CASES if c[0] not in ("nodes", "fem6000-inline")] + [(WIDE_CASE, 1)]


@pytest.mark.parametrize("case,sym", EXACT, ids=[f"{c[0]}-{'symmetric-pairs' if s else 'plain'}" for c, s in EXACT])
def test_both_arms_are_exact_on_integers_and_after_a_refill(E, O, gpu, case, sym):
    name, gen, kw = case
    base = dict(kw, sym_pairs=sym, value_map=1)
    cfg = E.make_config(**base)
    m = make_matrix(E, gen, cfg)
    n = m.n
    symmetric_values = name != "nodes"
    I0, J0, rp0 = m.I.copy(), m.J.copy(), m.row_idx.copy()
    m.V[:] = integer_values(I0, J0, symmetric_values)
    xs = [integer_x(n, seed) for seed in range(1, 5)]
    refs = [exact_reference(n, I0, J0, m.V, x, O) for x in xs]
    m.reorder(cfg)
    perm = m.reorder_list.copy()
    X = np.stack([E.vector_reorder(x, perm) for x in xs])
    plans = _plans(E, m, base)
    if sym and symmetric_values:
        assert plans[0].stats["sym_pairs"] > 0.2 * plans[0].stats["nnz"]
    assert plans[0].stats["er_inline"] > 0 or "inline" not in name
    assert plans[0].spmm_max_k == (3 if name == "wide-inline" else 4)

    def check(refs, what):
        for arm in ARMS:
            got = _products(E, plans[arm], X)
            for (k, walk), Y in got.items():
                if k == 0:
                    assert_exact(Y, E.vector_reorder(refs[0], perm), f"{what} arm {arm} one vector walk {walk}")
                for j in range(k):
                    assert_exact(Y[j], E.vector_reorder(refs[j], perm), f"{what} arm {arm} k = {k} column {j} walk {walk}")

    check(refs, "as built")
    # new values on the same pattern: the slot maps do not know about the form of the column words
    V2 = integer_values(I0, J0, symmetric_values, salt=1)
    order = E.entry_order(rp0, perm)
    for arm in ARMS:
        plans[arm].set_values(V2[order])
    _sync(E)
    check([exact_reference(n, I0, J0, V2, x) for x in xs], "refilled")
    for p in plans.values():
        p.destroy()


@pytest.mark.parametrize("sym", [0, 1], ids=["plain", "symmetric-pairs"])
def test_captured_graph(E, O, gpu, sym):
    kw = dict(lds_doubles=1024, sym_pairs=sym)
    cfg = E.make_config(**kw)
    m = make_matrix(E, FEM6, cfg)
    n = m.n
    m.V[:] = integer_values(m.I, m.J, True)
    x = integer_x(n, 3)
    y_ref = exact_reference(n, m.I, m.J, m.V, x, O)
    m.reorder(cfg)
    perm = m.reorder_list.copy()
    plans = _plans(E, m, kw)
    for arm in ARMS:
        dx, dy = E.DeviceBuffer(n).upload(E.vector_reorder(x, perm)), E.DeviceBuffer(n)
        for multiplies in (1, 2):
            g = plans[arm].graph(dx.ptr, dy.ptr, multiplies)
            for _ in range(3):
                dy.upload(np.full(n, np.nan))
                g.launch()
                _sync(E)
                assert_exact(dy.download(), E.vector_reorder(y_ref, perm), f"arm {arm}, {multiplies} multiplies per graph")
            g.destroy()
        dx.free(), dy.free()
    for p in plans.values():
        p.destroy()


@pytest.mark.parametrize("sym", [0, 1], ids=["plain", "symmetric-pairs"])
def test_pcg_takes_the_same_iterations_in_both_arms(E, O, gpu, sym):
    """The CG column kernels share the window body.  A strictly diagonally dominant matrix on the 6000-row pattern: the residual
    falls by a large factor per iteration, so the count at rtol = 1e-8 does not hang on the last bits of a sum."""
    kw = dict(lds_doubles=1024, sym_pairs=sym)
    cfg = E.make_config(**kw)
    g = make_matrix(E, FEM6, cfg)
    A = g.to_scipy()
    g.free()
    A = ((A + A.T) * 0.5).tolil()
    A.setdiag(0.0)
    A = A.tocsr()
    A.eliminate_zeros()
    diag = np.asarray(abs(A).sum(axis=1)).ravel() + 1.0
    A = (A + sp.diags(diag)).tocsr()
    A.sort_indices()
    n = A.shape[0]
    b = O.x_glibc(n) + 0.3
    sols = {}
    for arm in ARMS:
        c = E.make_config(ell_triples=arm, **kw)
        m = E.Matrix.from_csr(A.indptr, A.indices, A.data, c, symmetric=True)
        m.reorder(c)
        perm = m.reorder_list.copy()
        plan = E.Plan(m, c)
        if arm == 0:
            assert _coded_words(plan) < 0.9 * plan.stats["col_words"]
        xp, iters, rel = plan.cg(E.vector_reorder(b, perm), max_iter=200, rtol=1e-8, check_every=1,
                                 inv_diag=E.vector_reorder(1.0 / diag, perm))
        assert rel <= 1e-8 and 2 < iters < 200
        sols[arm] = (E.vector_recover(xp, perm), iters)
        plan.destroy()
    (x0, it0), (x2, it2) = sols[0], sols[2]
    assert it0 == it2
    assert np.linalg.norm(A @ x0 - b) <= 2e-8 * np.linalg.norm(b)
    if sym:
        assert np.linalg.norm(x0 - x2) <= 1e-8 * np.linalg.norm(x2)
    else:
        assert np.array_equal(x0, x2)
