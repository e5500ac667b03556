"""ehyb_minres / ehyb_minres_multi: MINRES on the device for symmetric indefinite systems.

The test matrices are a 2-D 5-point Laplacian plus n/8 random symmetric couplings in (-0.3, 0.3), minus 0.35 I: symmetric with
eigenvalues of both signs (asserted).  cpu_minres restates the device's recurrences, stop and breakdown rules in numpy; the
device must agree with it to a few per cent of the iteration count, reach the true residual, and agree with scipy's direct
solve.  With plain storage the device decides when to stop, so x, the iteration count and the relative residual are the same
bits whatever check_every, graph use or stream, and column j of a k-column solve is the one-vector solve of b_j.  Everything
runs in the permuted numbering unless said otherwise."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

ERR_ARG = 1
PLAIN = dict(window_mode=2, lds_doubles=256, direct=2, sym_pairs=0)


def indefinite_matrix(nx, ny, seed, shift=0.35):
    """5-point Laplacian (4 on the diagonal, -1 to every neighbour) + n/8 random symmetric couplings in (-0.3, 0.3) - shift I"""
    rng = np.random.default_rng(seed)
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    r = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    c = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    v = -np.ones(len(r))
    er, ec = rng.integers(0, n, n // 8), rng.integers(0, n, n // 8)
    ev = rng.uniform(-0.3, 0.3, n // 8)
    keep = er != ec
    r, c, v = np.concatenate([r, er[keep]]), np.concatenate([c, ec[keep]]), np.concatenate([v, ev[keep]])
    A = sp.coo_matrix((np.concatenate([v, v]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    return (A + sp.diags(np.full(n, 4.0 - shift))).tocsr()


def assert_indefinite(A, nx, ny):
    """x.Ax < 0 for the constant vector and > 0 for the checkerboard: eigenvalues of both signs"""
    n = A.shape[0]
    assert abs(A - A.T).nnz == 0
    smooth = np.ones(n)
    board = ((np.arange(n) % nx + np.arange(n) // nx) % 2 * 2 - 1).astype(np.float64)
    assert smooth @ (A @ smooth) < 0 < board @ (A @ board)


def cpu_minres(A, b, x0=None, max_iter=1000, rtol=1e-10, dinv=None):
    """The device's recurrences, stop and breakdown rules in numpy.  -> (x, iterations, relative residual, status)"""
    d = np.ones(len(b)) if dinv is None else dinv
    x = np.zeros_like(b) if x0 is None else x0.copy()
    ra = b - A @ x
    z = d * ra
    b2, bb = ra @ z, b @ (d * b)
    thr = rtol * rtol
    if not (np.isfinite(b2) and np.isfinite(bb)):
        return x, 0, np.nan, "breakdown"
    bb = bb if bb > 0 else 1.0
    with np.errstate(invalid="ignore"):
        phibar = np.sqrt(b2)
    rel = lambda: phibar / np.sqrt(bb)                   # noqa: E731
    if phibar * phibar <= thr * bb:
        return x, 0, rel(), "converged"
    if not b2 > 0:
        return x, 0, rel(), "breakdown"
    dbar = eps = sn = beta_old = 0.0
    cs = -1.0
    rb, wa, wb = np.zeros_like(b), np.zeros_like(b), np.zeros_like(b)
    it = 0
    while it < max_iter:
        if phibar * phibar <= thr * bb:
            return x, it, rel(), "converged"
        q = A @ z
        zq = z @ q
        alpha, beta = zq / b2, np.sqrt(b2)
        if not (np.isfinite(zq) and np.isfinite(alpha / beta)):
            return x, it, rel(), "breakdown"
        rn = q / beta - (alpha / beta) * ra
        if beta_old != 0:
            rn -= (beta / beta_old) * rb
        zn = d * rn
        b2n = rn @ zn
        if not (np.isfinite(b2n) and b2n >= 0):
            return x, it, rel(), "breakdown"
        beta_new = np.sqrt(b2n)
        delta, gbar = cs * dbar + sn * alpha, sn * dbar - cs * alpha
        gamma = np.sqrt(gbar * gbar + beta_new * beta_new)
        if not (np.isfinite(gamma) and gamma > 0):
            return x, it, rel(), "breakdown"
        cs_new, sn_new = gbar / gamma, beta_new / gamma
        wn = (d * ra / beta - eps * wb - delta * wa) / gamma
        x = x + (cs_new * phibar) * wn
        eps, dbar, phibar = sn * beta_new, -cs * beta_new, sn_new * phibar
        cs, sn, beta_old = cs_new, sn_new, beta
        ra, rb, wa, wb, z, b2 = rn, ra, wn, wa, zn, b2n
        it += 1
    return x, it, rel(), "converged" if phibar * phibar <= thr * bb else "max_iter"


class System:
    def __init__(self, E, A, **kw):
        self.A = A.tocsr()
        self.n = A.shape[0]
        self.kw = kw
        self.cfg = E.make_config(**kw)
        self.m = E.Matrix.from_csr(self.A.indptr, self.A.indices, self.A.data, self.cfg, symmetric=True)
        self.m.reorder(self.cfg)
        self.perm = self.m.reorder_list.copy()
        self.parts = len(self.m.part_boundary) - 1
        self.plan = E.Plan(self.m, self.cfg)
        self.inv_diag = E.vector_reorder(E.minres_inv_diag(self.A.diagonal()), self.perm)

    def solve(self, E, b, jacobi=False, x0=None, **kw):
        """b, x0 in the original numbering -> (x in the original numbering, iterations, relative residual)"""
        x, it, rel = self.plan.minres(E.vector_reorder(b, self.perm), x0=None if x0 is None else E.vector_reorder(x0, self.perm),
                                      inv_diag=self.inv_diag if jacobi else None, **kw)
        return E.vector_recover(x, self.perm), it, rel


NX, NY = 40, 36                       # 1,440 rows; 64 x 48 = 3,072 for the Jacobi test


@pytest.fixture(scope="module")
def small():
    """the 40 x 36 system, two right-hand sides, and per right-hand side what the tests compare against: cpu_minres at
    rtol 1e-10 and scipy's direct solve -- computed once"""
    A = indefinite_matrix(NX, NY, 3)
    assert_indefinite(A, NX, NY)
    n = A.shape[0]
    rhs = [A @ np.sin(np.arange(n) * 0.01) + 0.1, np.random.default_rng(7).uniform(-1, 1, n)]
    lu = spla.splu(A.tocsc())
    ref = []
    for b in rhs:
        _, it_cpu, rel_cpu, status = cpu_minres(A, b, max_iter=2000, rtol=1e-10)
        assert status == "converged" and it_cpu < 2000, (it_cpu, rel_cpu, status)
        ref.append((it_cpu, lu.solve(b)))
    return A, rhs, ref


@pytest.fixture(scope="module")
def plain(E, gpu, small):
    return System(E, small[0], **PLAIN)


SHAPES = [
    ("halo-window", dict(window_mode=2, lds_doubles=256, direct=2, sym_pairs=0), lambda st, nnz: st["nnz_ell"] > 0),
    ("reference-window-csr-residual", dict(window_mode=1, lds_doubles=128, direct=2, sym_pairs=0),
     lambda st, nnz: st["nnz_er"] > 0 and st["nnz_ell"] > 0),
    ("symmetric-pairs", dict(window_mode=2, lds_doubles=256, direct=2, sym_pairs=1), lambda st, nnz: st["sym_pairs"] > 0.25 * nnz),
    ("direct", dict(direct=1, lds_doubles=256), lambda st, nnz: st["nnz_ell"] == 0),
]


@pytest.mark.parametrize("name,kw,taken", SHAPES, ids=[s[0] for s in SHAPES])
def test_plan_shapes_against_cpu_and_scipy(E, gpu, small, name, kw, taken):
    A, rhs, ref = small
    s = System(E, A, **kw)
    assert taken(s.plan.stats, A.nnz), (name, s.plan.stats)
    assert s.parts >= 4, (name, s.parts)
    rtol = 1e-10
    for b, (it_cpu, x_ref) in zip(rhs, ref):
        x, it, rel = s.solve(E, b, max_iter=2000, rtol=rtol, check_every=4)
        true = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
        err = np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)
        print(name, "device", it, rel, "cpu", it_cpu, "true residual", true, "error", err)
        assert 0 < it < 2000 and rel <= rtol, (name, it, rel)
        assert abs(it - it_cpu) <= max(2, 0.03 * it_cpu), (name, it, it_cpu)
        assert true <= 2 * rtol, (name, true)
        assert err <= 1e-5, (name, err)


def test_jacobi_on_a_badly_scaled_system(E, gpu):
    """D A D with D = exp(U(-1, 1)): 1 / |a_ii| undoes most of the scaling.  The stop is in the M^-1 norm, and
    min(M^-1) ||r||_2^2 <= r.M^-1 r, b.M^-1 b <= max(M^-1) ||b||_2^2, which gives the bound on the true 2-norm residual."""
    nx, ny = 64, 48
    A0 = indefinite_matrix(nx, ny, 3)
    assert_indefinite(A0, nx, ny)
    n = A0.shape[0]
    d = np.exp(np.random.default_rng(5).uniform(-1, 1, n))
    A = (sp.diags(d) @ A0 @ sp.diags(d)).tocsr()
    s = System(E, A, **PLAIN)
    assert s.parts >= 4
    rtol = 1e-8
    b = A @ np.linspace(-1, 1, n)
    x_pre, it_pre, rel_pre = s.solve(E, b, jacobi=True, max_iter=6000, rtol=rtol)
    x_none, it_none, rel_none = s.solve(E, b, jacobi=False, max_iter=6000, rtol=rtol)
    m_inv = 1.0 / np.abs(A.diagonal())
    true_pre = np.linalg.norm(b - A @ x_pre) / np.linalg.norm(b)
    true_none = np.linalg.norm(b - A @ x_none) / np.linalg.norm(b)
    print("jacobi", it_pre, rel_pre, true_pre, "plain", it_none, rel_none, true_none, "bound", 2 * rtol * np.sqrt(m_inv.max() / m_inv.min()))
    assert rel_pre <= rtol and rel_none <= rtol, (rel_pre, rel_none)
    assert 0 < it_pre and 2 * it_pre < it_none, (it_pre, it_none)
    assert true_pre <= 2 * rtol * np.sqrt(m_inv.max() / m_inv.min()), true_pre
    assert true_none <= 2 * rtol, true_none


def test_the_residual_estimate_never_rises(E, gpu, small, plain):
    b = E.vector_reorder(small[1][1], plain.perm)
    before = np.inf
    for max_iter in (5, 10, 20, 40, 80):
        _, it, rel = plain.plan.minres(b, max_iter=max_iter, rtol=1e-30)
        assert it == max_iter and 0 < rel <= before, (max_iter, it, rel, before)
        before = rel


def _same_bits(got, want, what):
    x, it, rel = got
    xw, itw, relw = want
    assert it == itw, (what, it, itw)
    assert np.array_equal(np.array([rel]), np.array([relw]), equal_nan=True), (what, rel, relw)
    assert np.array_equal(x.view(np.int64), xw.view(np.int64)), (what, np.abs(x - xw).max())


@pytest.mark.parametrize("max_iter", [2000, 23], ids=["converges", "max-iter-odd"])
def test_plain_storage_is_exact_for_every_check_every_graph_and_stream(E, gpu, small, plain, max_iter):
    s = plain
    launches = E.Plan(s.m, E.make_config(graphs=2, **PLAIN))
    b = E.vector_reorder(small[1][1], s.perm)
    run = dict(max_iter=max_iter, rtol=1e-10, inv_diag=s.inv_diag)
    ref = s.plan.minres(b, check_every=1, **run)
    assert ref[1] > 0 and (ref[1] < max_iter) == (max_iter == 2000), ref[1:]
    if max_iter == 23:
        assert ref[1] == 23
    for check_every in (2, 10, 50):
        _same_bits(s.plan.minres(b, check_every=check_every, **run), ref, f"check_every={check_every}")
        _same_bits(launches.minres(b, check_every=check_every, **run), ref, f"graphs=2 check_every={check_every}")
    _same_bits(launches.minres(b, check_every=1, **run), ref, "graphs=2 check_every=1")
    st = E.Stream()
    try:
        _same_bits(s.plan.minres(b, check_every=10, stream=st.ptr, **run), ref, "user stream")
    finally:
        st.destroy()
    _same_bits(s.plan.minres(b, check_every=1, **run), ref, "second run")


def test_edges(E, gpu, small, plain):
    A, rhs, ref = small
    s = plain
    n = s.n
    # b = 0: nothing to do, x untouched; max_iter = 0
    x, it, rel = s.plan.minres(np.zeros(n), rtol=0.0)
    assert it == 0 and rel == 0.0 and np.array_equal(x.view(np.int64), np.zeros(n).view(np.int64))
    x, it, rel = s.plan.minres(E.vector_reorder(rhs[1], s.perm), max_iter=0)
    assert it == 0 and rel == 1.0 and not x.any(), (it, rel)
    # x0 = the solution: 0 iterations and x comes back as it went in (the residual of the direct solve is far below 1e-8)
    x0 = E.vector_reorder(ref[0][1], s.perm)
    x, it, rel = s.plan.minres(E.vector_reorder(rhs[0], s.perm), x0=x0, rtol=1e-8)
    assert it == 0 and rel <= 1e-8 and np.array_equal(x.view(np.int64), x0.view(np.int64)), (it, rel)
    # x0 != 0 reaches the same answer
    start = np.random.default_rng(4).uniform(-1, 1, n)
    x, it, rel = s.solve(E, rhs[1], x0=start, max_iter=2000, rtol=1e-10)
    assert 0 < it < 2000 and rel <= 1e-10
    assert np.linalg.norm(x - ref[1][1]) <= 1e-5 * np.linalg.norm(ref[1][1])


def test_a_diagonal_of_plus_and_minus_one_needs_two_iterations(E, gpu):
    """two distinct eigenvalues: the Krylov space is exhausted after two steps"""
    n = 5000
    sign = np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
    s = System(E, sp.diags(sign).tocsr(), **PLAIN)
    b = np.random.default_rng(2).uniform(-1, 1, n)
    x, it, rel = s.solve(E, b, max_iter=50, rtol=1e-12)
    assert 1 <= it <= 2 and rel <= 1e-12, (it, rel)
    assert np.linalg.norm(x - sign * b) <= 1e-12 * np.linalg.norm(b)


def test_nan_in_b_is_a_breakdown_and_x_stays(E, gpu, plain):
    s = plain
    rng = np.random.default_rng(12)
    b = rng.uniform(-1, 1, s.n)
    b[s.n // 3] = np.nan
    x0 = rng.uniform(-1, 1, s.n)
    with pytest.raises(E.EhybError) as ei:
        s.plan.minres(b, x0=x0, inv_diag=s.inv_diag)
    assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value)
    x, it, rel = s.plan.minres(b, x0=x0, inv_diag=s.inv_diag, allow_breakdown=True)
    assert it == 0 and np.isnan(rel)
    assert np.array_equal(x.view(np.int64), x0.view(np.int64))


def test_a_negative_preconditioner_is_a_breakdown(E, gpu, small, plain):
    """one entry of inv_diag hugely negative: beta_1^2 = r.M^-1 r < 0 at the start; every entry negative likewise.  The call comes
    back at once (no hang), x unchanged."""
    s = plain
    b = E.vector_reorder(small[1][1], s.perm)
    one = s.inv_diag.copy()
    one[s.n // 2] = -1e9
    assert abs(b[s.n // 2]) > 1e-3
    for inv in (one, -s.inv_diag):
        with pytest.raises(E.EhybError) as ei:
            s.plan.minres(b, inv_diag=inv, max_iter=200)
        assert "breakdown" in str(ei.value)
        x, it, rel = s.plan.minres(b, inv_diag=inv, max_iter=200, allow_breakdown=True)
        assert it == 0 and not x.any(), (it, rel)
    assert cpu_minres(small[0], small[1][1], dinv=-np.ones(s.n))[3] == "breakdown"


def test_null_outputs_and_the_c_abi(E, gpu, small, plain):
    s = plain
    b = E.vector_reorder(small[1][0], s.perm)
    want = s.plan.minres(b, rtol=1e-10, max_iter=2000)
    db, dx = E.DeviceBuffer(s.n).upload(b), E.DeviceBuffer(s.n).upload(np.zeros(s.n))
    lib = E.host._lib.load()
    assert lib.ehyb_minres(s.plan.h, None, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), 2000, 1e-10, 10, None, None, None) == 0
    assert np.array_equal(dx.download().view(np.int64), want[0].view(np.int64))
    assert np.array_equal(db.download(), b)


# ------------------------------------------------------------------ k columns
def column_mix(E, s, A, rhs):
    """ordinary, early-converging (b = A applied to a few smooth modes, started next to the solution), zero, NaN, ordinary"""
    n = s.n
    i = np.arange(n)
    smooth = sum(np.sin((k + 1) * np.pi * (i % NX + 1) / (NX + 1)) * np.sin((k + 1) * np.pi * (i // NX + 1) / (NY + 1)) for k in range(3))
    nan = rhs[0].copy()
    nan[7] = np.nan
    B = [rhs[1], A @ smooth, np.zeros(n), nan, rhs[0]]
    X0 = [np.zeros(n), smooth * (1 + 1e-4), np.zeros(n), np.zeros(n), np.zeros(n)]
    return np.stack([E.vector_reorder(b, s.perm) for b in B]), np.stack([E.vector_reorder(x, s.perm) for x in X0])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_every_column_of_a_multi_solve_is_the_single_solve(E, gpu, small, plain, k):
    """k = 5: launches 3 + 2 columns wide.  The NaN column (from k = 4 on) breaks down at the start, the zero column and the
    early one stop before the others; each finite column is ehyb_minres on it, bit for bit."""
    A, rhs, _ = small
    s = plain
    B, X0 = column_mix(E, s, A, rhs)
    run = dict(max_iter=2000, rtol=1e-6, check_every=4, inv_diag=s.inv_diag)
    if k >= 4:
        with pytest.raises(E.EhybError) as ei:
            s.plan.minres_multi(B[:k], X0[:k], **run)
        assert ei.value.code == ERR_ARG and "breakdown in column 3" in str(ei.value)
    X, it, rel = s.plan.minres_multi(B[:k], X0[:k], allow_breakdown=True, **run)
    print("k", k, "iterations", list(it), "residuals", list(rel))
    for j in range(k):
        if j == 3:
            assert it[j] == 0 and np.isnan(rel[j]) and np.array_equal(X[j], X0[j])
            continue
        _same_bits((X[j], int(it[j]), float(rel[j])), s.plan.minres(B[j], x0=X0[j], **run), f"k={k} column {j}")
    assert 0 < it[0] and rel[0] <= 1e-6
    if k >= 3:
        assert it[2] == 0 and 0 < it[1] < it[0], list(it)


def test_multi_with_leading_dimensions(E, gpu, small, plain):
    A, rhs, _ = small
    s, n, k = plain, plain.n, 3
    B, X0 = column_mix(E, s, A, rhs)
    ldb, ldx = n + 37, n + 5
    Bb = np.full((k, ldb), -7.25)
    Bb[:, :n] = B[:k]
    Xb = np.full((k, ldx), -6.02214076e23)
    Xb[:, :n] = X0[:k]
    db, dx = E.DeviceBuffer(k * ldb).upload(Bb.ravel()), E.DeviceBuffer(k * ldx).upload(Xb.ravel())
    it, rel = (C.c_int * k)(), (C.c_double * k)()
    lib = E.host._lib.load()
    rc = lib.ehyb_minres_multi(s.plan.h, None, C.c_void_p(db.ptr), ldb, C.c_void_p(dx.ptr), ldx, k, 2000, 1e-6, 4, None, it, rel)
    assert rc == 0, lib.ehyb_last_error()
    Xo = dx.download().reshape(k, ldx)
    assert np.array_equal(Xo[:, n:].view(np.int64), Xb[:, n:].view(np.int64)), "the gap behind the columns of X"
    for j in range(k):
        _same_bits((Xo[j, :n].copy(), it[j], rel[j]), s.plan.minres(B[j], x0=X0[j], max_iter=2000, rtol=1e-6, check_every=4), f"column {j}")


# ------------------------------------------------------------------ past the unrolled loops in a composed solve
BIG_NX, BIG_NY = 725, 724             # 524,900 rows > 4 * 131,072: every thread of the vector kernels runs an unrolled trip
NEVER = 1e-150


def test_six_iterations_past_the_unrolled_loops(E, gpu):
    """a shifted 5-point stencil (4 - 2.1 on the diagonal: indefinite), six iterations at a tolerance that never stops, against
    cpu_minres: an indexing error is O(1), six iterations of rounding stay near 1e-15.  Then columns 2, 3 and 4 wide: each
    column is the single solve, bit for bit, where the K-wide kernels run their unrolled bodies."""
    import solver_cases as sc

    n = BIG_NX * BIG_NY
    idx = np.arange(n).reshape(BIG_NY, BIG_NX)
    r = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    c = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    A = (sp.coo_matrix((-np.ones(2 * len(r)), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)) + sp.diags(np.full(n, 1.9))).tocsr()
    assert_indefinite(A, BIG_NX, BIG_NY)
    s = System(E, A, lds_doubles=5120, direct=2, sym_pairs=0)
    assert s.plan.stats["sym_pairs"] == 0 and s.plan.stats["er_partials"] == 0
    assert (s.plan.array("er_seg_row") >= 0).all(), "no residual row may be split into segments"
    assert n >= 4 * sc.S + 1 and sc.solver_grid(n) == sc.STEP_GRID
    assert {(1, 0), (1, 1)} <= sc.walk_profile(n, sc.STEP_GRID)
    rng = np.random.default_rng(9)
    B = rng.uniform(-1, 1, (4, n))
    singles = []
    for j, jacobi in ((0, False), (1, True)):
        x, it, rel = s.solve(E, B[j], jacobi=jacobi, max_iter=6, rtol=NEVER)
        x_cpu, it_cpu, rel_cpu, _ = cpu_minres(A, B[j], max_iter=6, rtol=NEVER, dinv=1.0 / np.abs(A.diagonal()) if jacobi else None)
        err = np.linalg.norm(x - x_cpu) / np.linalg.norm(x_cpu)
        print("jacobi", jacobi, "error against cpu_minres", err, "residuals", rel, rel_cpu)
        assert it == 6 == it_cpu and err <= 1e-12 and abs(rel - rel_cpu) <= 1e-12 * rel_cpu, (it, err, rel, rel_cpu)
    Bp = np.stack([E.vector_reorder(b, s.perm) for b in B])
    run = dict(max_iter=6, rtol=NEVER, inv_diag=s.inv_diag)
    singles = [s.plan.minres(Bp[j], **run) for j in range(4)]
    for k in (2, 3, 4):
        X, it, rel = s.plan.minres_multi(Bp[:k], **run)
        for j in range(k):
            _same_bits((X[j], int(it[j]), float(rel[j])), singles[j], f"k={k} column {j}")
