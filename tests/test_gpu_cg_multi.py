"""ehyb_cg_multi / ehyb_pcg_multi: k independent CG solves that share every multiply (ehyb_spmm of the k directions).

Column j is ehyb_pcg(b_j) by construction -- the same grid, index walk and summation order per column, its own alpha, beta
and stopping test -- so with plain storage (and no residual row split into segments) every column must equal the
one-vector solve bit for bit: X, iterations and relative residual.  Symmetric pair storage is checked against the CPU's
recurrences instead.  Everything runs in the permuted numbering."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_cg import cpu_cg, spd_matrix

pytestmark = pytest.mark.gpu

LDS_MAX = 20480
ERR_ARG = 1
KS = (1, 2, 3, 5, 8)

# plain storage plans over the three multiply shapes; p . q always from the dot kernel in the one-vector solve too
PLAIN = [
    ("window-halo", dict(lds_doubles=5120, direct=2)),
    ("window-csr-residual", dict(window_mode=1, fuse_er=2, lds_doubles=2048, direct=2)),
    ("direct", dict(direct=1)),
]


class System:
    def __init__(self, E, A, **kw):
        self.A = A
        self.n = A.shape[0]
        self.cfg = E.make_config(**kw)
        self.m = E.Matrix.from_csr(A.indptr, A.indices, A.data, self.cfg, symmetric=True)
        self.m.reorder(self.cfg)
        self.perm = self.m.reorder_list.copy()
        self.plan = E.Plan(self.m, self.cfg)
        self.inv_diag = E.vector_reorder(1.0 / A.diagonal(), self.perm)


def rhs_bank(E, sysm, k, seed=0):
    """k right-hand sides (permuted) that converge at different iteration counts: smooth ones, random ones, a few spikes."""
    rng = np.random.default_rng(seed)
    n = sysm.n
    out = []
    for j in range(k):
        kind = j % 4
        if kind == 0:
            b = sysm.A @ np.ones(n)
        elif kind == 1:
            b = rng.uniform(-1, 1, n) * 10.0 ** (j - 4)
        elif kind == 2:
            b = np.zeros(n)
            b[rng.integers(0, n, 3 + j)] = 1.0
        else:
            b = sysm.A @ np.sin(np.arange(n) * (0.001 * (j + 1))) + 0.01 * rng.uniform(-1, 1, n)
        out.append(E.vector_reorder(b, sysm.perm))
    return np.stack(out)


def singles(plan, B, X0=None, **kw):
    xs, its, rels = [], [], []
    for j in range(len(B)):
        x, it, rel = plan.cg(B[j], x0=None if X0 is None else X0[j], **kw)
        xs.append(x)
        its.append(it)
        rels.append(rel)
    return np.stack(xs), np.array(its), np.array(rels)


def assert_same_bits(got, want, what):
    X, it, rel = got
    Xw, itw, relw = want
    assert np.array_equal(it, itw), (what, it, itw)
    assert np.array_equal(rel, relw, equal_nan=True), (what, rel, relw)
    for j in range(len(X)):
        assert np.array_equal(X[j].view(np.int64), Xw[j].view(np.int64)), (what, j, np.abs(X[j] - Xw[j]).max())


@pytest.fixture(scope="module", params=PLAIN, ids=[p[0] for p in PLAIN])
def plain_system(request):
    import ehyb_spmv_gpu_amd as E

    name, kw = request.param
    s = System(E, spd_matrix(120, 100, 3000, 11), sym_pairs=0, cg_fused_dot=2, **kw)
    st = s.plan.stats
    assert st["sym_pairs"] == 0
    assert (s.plan.array("er_seg_row") >= 0).all(), "no residual row may be split into segments"
    if name == "direct":
        assert st["nnz_ell"] == 0
    elif name == "window-csr-residual":
        assert st["nnz_er"] > 0 and st["er_inline"] == 0 and st["er_partials"] == 0
    else:
        assert st["nnz_ell"] > 0
    return s


@pytest.mark.parametrize("k", KS)
def test_bit_identity_with_the_single_solve(E, gpu, plain_system, k):
    s = plain_system
    B = rhs_bank(E, s, k, seed=k)
    rng = np.random.default_rng(100 + k)
    X0 = np.zeros_like(B)
    X0[::2] = 0.01 * rng.uniform(-1, 1, X0[::2].shape)       # some columns start from a guess
    all_iters = set()
    for inv in (None, s.inv_diag):
        for check_every in (1, 3, 10):
            kw = dict(max_iter=300, rtol=1e-10, check_every=check_every, inv_diag=inv)
            want = singles(s.plan, B, X0, **kw)
            got = s.plan.cg_multi(B, X0, **kw)
            assert_same_bits(got, want, f"k={k} jacobi={inv is not None} check_every={check_every}")
            all_iters |= set(int(i) for i in got[1])
    if k >= 3:
        assert len(all_iters) >= 3, all_iters       # the columns froze at different check points


def test_symmetric_pairs_k4_plan_against_the_cpu(E, O, gpu):
    s = System(E, spd_matrix(120, 100, 3000, 1), lds_doubles=LDS_MAX // 4, sym_pairs=1, direct=2)
    assert s.plan.stats["sym_pairs"] > 0.25 * s.A.nnz and s.plan.spmm_max_k == 4
    rng = np.random.default_rng(3)
    bs = [O.x_glibc(s.n) + 0.3, s.A @ np.ones(s.n), rng.uniform(-1, 1, s.n), rng.uniform(0, 2, s.n)]
    B = np.stack([E.vector_reorder(b, s.perm) for b in bs])
    X, iters, rel = s.plan.cg_multi(B, max_iter=400, rtol=1e-10, check_every=1)
    for j, b in enumerate(bs):
        x = E.vector_recover(X[j], s.perm)
        x_cpu, it_cpu, _ = cpu_cg(s.A, b, 400, 1e-10)
        assert rel[j] <= 1e-10 and abs(iters[j] - it_cpu) <= 2, (j, iters[j], it_cpu, rel[j])
        assert np.linalg.norm(s.A @ x - b) <= 2e-10 * np.linalg.norm(b), j
        assert np.linalg.norm(x - x_cpu) <= 1e-8 * np.linalg.norm(x_cpu), j


def test_jacobi_pcg_on_a_badly_scaled_system(E, gpu):
    A0 = spd_matrix(100, 90, 2000, 3)
    n = A0.shape[0]
    d = 10.0 ** np.random.default_rng(5).uniform(-2, 2, n)
    A = (sp.diags(d) @ A0 @ sp.diags(d)).tocsr()
    s = System(E, A, lds_doubles=2048, sym_pairs=1)
    rng = np.random.default_rng(6)
    bs = [A @ np.ones(n), A @ rng.uniform(0, 1, n), A @ np.linspace(-1, 1, n)]
    B = np.stack([E.vector_reorder(b, s.perm) for b in bs])
    X, it_pcg, rel = s.plan.cg_multi(B, max_iter=3000, rtol=1e-9, check_every=5, inv_diag=s.inv_diag)
    _, it_cg, rel_cg = s.plan.cg_multi(B, max_iter=3000, rtol=1e-9, check_every=5)
    for j, b in enumerate(bs):
        x = E.vector_recover(X[j], s.perm)
        assert rel[j] <= 1e-9 and np.linalg.norm(A @ x - b) <= 5e-9 * np.linalg.norm(b), j
        assert it_pcg[j] * 3 < it_cg[j] or rel_cg[j] > 1e-9, (j, it_pcg[j], it_cg[j], rel_cg[j])


def test_converged_and_zero_columns_do_not_move(E, gpu):
    s = System(E, spd_matrix(110, 90, 2500, 4), lds_doubles=2048, sym_pairs=0)
    B = rhs_bank(E, s, 4, seed=9)
    x_sol, it_sol, _ = s.plan.cg(B[1], max_iter=500, rtol=1e-12)
    assert it_sol > 0
    B[2] = 0.0                                      # zero b from a zero guess: r = 0
    X0 = np.zeros_like(B)
    X0[1] = x_sol                                   # already a solution to 1e-12, asked for 1e-8
    X, iters, rel = s.plan.cg_multi(B, X0, max_iter=500, rtol=1e-8, check_every=4)
    assert iters[1] == 0 and iters[2] == 0, iters
    assert iters[0] > 0 and iters[3] > 0, iters
    assert np.array_equal(X[1].view(np.int64), X0[1].view(np.int64))
    assert np.array_equal(X[2].view(np.int64), X0[2].view(np.int64))
    assert rel[2] == 0.0 and rel[1] <= 1e-8
    assert_same_bits((X[[0, 3]], iters[[0, 3]], rel[[0, 3]]), singles(s.plan, B[[0, 3]], max_iter=500, rtol=1e-8, check_every=4),
                     "live columns")


def test_breakdown_stays_in_its_column(E, gpu):
    s = System(E, spd_matrix(110, 90, 2500, 4), lds_doubles=2048, sym_pairs=0)
    B = rhs_bank(E, s, 3, seed=2)
    B[1, s.n // 3] = np.nan
    kw = dict(max_iter=300, rtol=1e-10, check_every=2)
    with pytest.raises(E.EhybError) as ei:
        s.plan.cg_multi(B, **kw)
    assert "breakdown" in str(ei.value) and "ehyb_pcg_multi" in str(ei.value)
    X, iters, rel = s.plan.cg_multi(B, allow_breakdown=True, **kw)
    assert np.isnan(rel[1]) and iters[1] == 0 and not np.isnan(rel[[0, 2]]).any()
    assert np.array_equal(X[1], np.zeros(s.n))                     # frozen at the start: x0 untouched
    assert_same_bits((X[[0, 2]], iters[[0, 2]], rel[[0, 2]]), singles(s.plan, B[[0, 2]], **kw), "finite columns")
    with pytest.raises(E.EhybError):
        s.plan.cg(B[1], **kw)                                       # the one-vector solve calls it a breakdown as well


def test_leading_dimensions_leave_the_gaps_alone(E, gpu):
    s = System(E, spd_matrix(110, 90, 2500, 4), lds_doubles=2048, sym_pairs=0)
    n, k = s.n, 3
    B = rhs_bank(E, s, k, seed=5)
    ldb, ldx = n + 37, n + 5
    Bb = np.full((k, ldb), -7.25)
    Bb[:, :n] = B
    Xb = np.full((k, ldx), 1e300)
    Xb[:, :n] = 0.0
    db, dx = E.DeviceBuffer(k * ldb).upload(Bb.ravel()), E.DeviceBuffer(k * ldx).upload(Xb.ravel())
    lib = E.host._lib.load()
    it = (C.c_int * k)()
    rel = (C.c_double * k)()
    rc = lib.ehyb_cg_multi(s.plan.h, C.c_void_p(db.ptr), ldb, C.c_void_p(dx.ptr), ldx, k, 300, 1e-10, 6, None, it, rel)
    assert rc == 0, lib.ehyb_last_error()
    Xo = dx.download().reshape(k, ldx)
    assert np.array_equal(db.download().reshape(k, ldb), Bb)
    assert (Xo[:, n:] == 1e300).all()
    want = s.plan.cg_multi(B, max_iter=300, rtol=1e-10, check_every=6)
    assert_same_bits((Xo[:, :n], np.array(list(it)), np.array(list(rel))), want, "ld > n")
    # NULL outputs are allowed
    dx.upload(Xb.ravel())
    assert lib.ehyb_cg_multi(s.plan.h, C.c_void_p(db.ptr), ldb, C.c_void_p(dx.ptr), ldx, k, 300, 1e-10, 6, None, None, None) == 0
    assert np.array_equal(dx.download().reshape(k, ldx), np.concatenate([want[0], Xb[:, n:]], axis=1))


def test_streams_and_graphs_give_the_same_bits(E, gpu):
    A = spd_matrix(110, 90, 2500, 8)
    s = System(E, A, lds_doubles=LDS_MAX // 4, sym_pairs=0, direct=2)
    plain = E.Plan(s.m, E.make_config(lds_doubles=LDS_MAX // 4, sym_pairs=0, direct=2, graphs=2))
    B = rhs_bank(E, s, 5, seed=8)
    kw = dict(max_iter=61, rtol=1e-30, check_every=8)
    ref = s.plan.cg_multi(B, **kw)
    assert (ref[1] == 61).all()
    st = E.Stream()
    try:
        assert_same_bits(s.plan.cg_multi(B, stream=st.ptr, **kw), ref, "explicit stream")
    finally:
        st.destroy()
    assert_same_bits(plain.cg_multi(B, **kw), ref, "graphs = 2")
    assert_same_bits(s.plan.cg_multi(B, **kw), ref, "again")


def test_full_size_symmetric_pairs_k4(E, gpu):
    """The audikw_1-like system made diagonally dominant (as tools/cg_time.py), a symmetric pair plan built for k = 4, 40
    iterations at rtol = 0: every column's relative residual within 1e-6 (relative) of the one-vector solve on the same plan."""
    import bench as Bn

    gen, gargs, _ = Bn.WORKLOADS["audikw_1-like"]
    cfg = E.make_config(lds_doubles=LDS_MAX // 4, sym_pairs=1)
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    I, J, V = m.I, m.J, m.V
    off = np.bincount(I, weights=np.abs(V) * (I != J), minlength=m.n)
    V[I == J] = (off + 1.0)[I[I == J]]
    m.reorder(cfg)
    plan = E.Plan(m, cfg)
    assert plan.stats["sym_pairs"] > 0 and plan.spmm_max_k == 4
    rng = np.random.default_rng(40)
    B = np.stack([np.ones(m.n)] + [rng.uniform(-1, 1, m.n) for _ in range(3)])
    X, iters, rel = plan.cg_multi(B, max_iter=40, rtol=0.0, check_every=10)
    assert (iters == 40).all()
    for j in range(4):
        _, it1, rel1 = plan.cg(B[j], max_iter=40, rtol=0.0, check_every=10)
        assert it1 == 40 and 0 < rel1
        assert abs(rel[j] - rel1) <= 1e-6 * rel1, (j, rel[j], rel1)
