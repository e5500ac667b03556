"""cfg.ell_nt = 4 / 5: a fixed set of slabs is read with plain loads, the rest of the value stream with the non-temporal hint.
Which loads carry the hint changes no result: plain storage is bit-identical to cfg.ell_nt = 2 (plain loads throughout), symmetric
pairs bit-identical on exact-integer inputs (exact_cases.py) and within the suite's 1e-12 row bound of the oracle otherwise (their
LDS adds are unordered) -- for K = 1 and K = 4 columns, both walk directions, and inside a CG solve.  The matrices are far smaller
than the Infinity Cache; cfg.ell_keep forces a share all the same."""
import numpy as np
import pytest

from exact_cases import assert_exact, exact_reference, integer_values, integer_x

pytestmark = pytest.mark.gpu

FEM = ("fem3d", (60000, 3, 28, 28, 13500, 1, 1))
K = 4


def _sync(E):
    assert E.host._lib.load().ehyb_dev_sync() == 0


def _products(E, plan, X):
    """X (K, n) permuted -> {(k, walk): Y}: K = 1 through ehyb_spmv_walk, K = 4 through ehyb_spmm, both directions."""
    k, n = X.shape
    assert plan.spmm_max_k >= k
    dx = E.DeviceBuffer(k * n).upload(X.ravel())
    out = {}
    for walk in (0, 1):
        dy = E.DeviceBuffer(k * n).upload(np.full(k * n, np.nan))
        plan.spmv(dx.ptr, dy.ptr, walk=walk)
        _sync(E)
        out[(1, walk)] = dy.download()[:n].copy()
        dy.upload(np.full(k * n, np.nan))
        plan.spmm(dx.ptr, dy.ptr, k, walk=walk)
        _sync(E)
        out[(k, walk)] = dy.download().reshape(k, n).copy()
        dy.free()
    dx.free()
    return out


@pytest.mark.parametrize("ell_nt", [4, 5], ids=["spread", "block"])
@pytest.mark.parametrize("ell_keep", [1, 400, 1000])
def test_plain_storage_is_bit_identical_to_plain_loads(E, O, gpu, ell_nt, ell_keep):
    kw = dict(lds_doubles=4096)
    base_cfg = E.make_config(ell_nt=2, **kw)
    m = E.Matrix.generate(*FEM[:1], *FEM[1], cfg=base_cfg)
    x = O.x_glibc(m.n)
    y_ref, scale = O.spmv_coo(m.n, m.I, m.J, m.V, x), O.abs_rowsum(m.n, m.I, m.J, m.V, x)
    m.reorder(base_cfg)
    perm = m.reorder_list
    X = np.stack([E.vector_reorder(np.roll(x, 7 * j) * (1.0 + j), perm) for j in range(K)])
    base = E.Plan(m, base_cfg)
    want = _products(E, base, X)
    assert O.check_strict(E.vector_recover(want[(1, 0)], perm), y_ref, scale)[0] == 0
    cfg = E.make_config(ell_nt=ell_nt, ell_keep=ell_keep, **kw)
    assert (cfg.ell_nt, cfg.ell_keep) == (ell_nt, ell_keep)
    plan = E.Plan(m, cfg)
    st = plan.stats
    assert st["nnz_ell"] > 0 and st["sym_pairs"] == 0
    assert plan.resident_bytes <= 8 * st["size_block_ell"] * (ell_keep * 1024 // 1000) // 1024
    got = _products(E, plan, X)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    base.destroy(), plan.destroy()


@pytest.mark.parametrize("ell_nt", [4, 5], ids=["spread", "block"])
@pytest.mark.parametrize("ell_keep", [1, 400, 1000])
def test_symmetric_pairs_exact_and_within_the_row_bound(E, O, gpu, ell_nt, ell_keep):
    cfg = E.make_config(lds_doubles=4096, sym_pairs=1, ell_nt=ell_nt, ell_keep=ell_keep)
    # exact integers: one possible product, whatever the order of the LDS adds
    m = E.Matrix.generate(*FEM[:1], *FEM[1], cfg=cfg)
    n = m.n
    m.V[:] = integer_values(m.I, m.J, True)
    xs = [integer_x(n, seed) for seed in range(1, K + 1)]
    refs = [exact_reference(n, m.I, m.J, m.V, x, O) for x in xs]
    m.reorder(cfg)
    perm = m.reorder_list
    plan = E.Plan(m, cfg)
    assert plan.stats["sym_pairs"] > 0.2 * plan.stats["nnz"]
    got = _products(E, plan, np.stack([E.vector_reorder(x, perm) for x in xs]))
    for walk in (0, 1):
        assert_exact(got[(1, walk)], E.vector_reorder(refs[0], perm), f"K = 1 walk {walk}")
        for j in range(K):
            assert_exact(got[(K, walk)][j], E.vector_reorder(refs[j], perm), f"K = {K} column {j} walk {walk}")
    plan.destroy()
    # the generator's own values: every row within 1e-12 of the oracle
    m = E.Matrix.generate(*FEM[:1], *FEM[1], cfg=cfg)
    xs = [np.roll(O.x_glibc(n), 7 * j) * (1.0 + j) for j in range(K)]
    refs = [(O.spmv_coo(n, m.I, m.J, m.V, x), O.abs_rowsum(n, m.I, m.J, m.V, x)) for x in xs]
    m.reorder(cfg)
    perm = m.reorder_list
    plan = E.Plan(m, cfg)
    got = _products(E, plan, np.stack([E.vector_reorder(x, perm) for x in xs]))
    for walk in (0, 1):
        assert O.check_strict(E.vector_recover(got[(1, walk)], perm), *refs[0])[0] == 0, walk
        for j in range(K):
            assert O.check_strict(E.vector_recover(got[(K, walk)][j], perm), *refs[j])[0] == 0, (walk, j)
    plan.destroy()


@pytest.mark.parametrize("sym", [0, 1], ids=["plain", "symmetric-pairs"])
@pytest.mark.parametrize("ell_nt", [4, 5], ids=["spread", "block"])
def test_cg_solve_with_a_pinned_set(E, O, gpu, sym, ell_nt):
    """The CG column kernels run the same window body: plain storage iterates bit for bit as with plain loads, symmetric pairs
    reach the same solution."""
    from test_gpu_cg import spd_matrix

    A = spd_matrix(120, 100, 3000, 1)
    n = A.shape[0]
    b = O.x_glibc(n) + 0.3
    sols = []
    for nt, keep in ((2, 0), (ell_nt, 400)):
        cfg = E.make_config(lds_doubles=2048, sym_pairs=sym, ell_nt=nt, ell_keep=keep)
        m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=True)
        m.reorder(cfg)
        perm = m.reorder_list.copy()
        plan = E.Plan(m, cfg)
        xp, iters, rel = plan.cg(E.vector_reorder(b, perm), max_iter=400, rtol=1e-10, check_every=1)
        assert rel <= 1e-10
        sols.append((E.vector_recover(xp, perm), iters))
        plan.destroy()
    (x0, it0), (x1, it1) = sols
    assert np.linalg.norm(A @ x1 - b) <= 2e-10 * np.linalg.norm(b)
    if sym:
        assert abs(it0 - it1) <= 2 and np.linalg.norm(x1 - x0) <= 1e-8 * np.linalg.norm(x0)
    else:
        assert it0 == it1 and np.array_equal(x0, x1)
