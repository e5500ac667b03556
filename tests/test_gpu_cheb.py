"""ehyb_pcg_cheb / ehyb_pcg_cheb_multi / ehyb_lambda_max on the device: CG with a Chebyshev polynomial preconditioner
against the numpy restatement of cheb_cases.py and against ehyb_pcg in the same process.  The solve arms cover plain
storage, symmetric pairs, the polynomial on the cfg.val_f32 plan of the same reordered matrix, and a plan with a CSR
residual; then reproducibility (runs, graphs against plain launches, check_every), the k-column solve bit for bit against
the one-vector one, and the breakdown of a polynomial whose lmax is no upper bound.  Everything in the permuted numbering."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import cheb_cases as cc
from test_gpu_cg import spd_matrix
from test_gpu_cg_multi import assert_same_bits
from val_f32_cases import f32

pytestmark = pytest.mark.gpu

ERR_STATE = 8
RTOL = 1e-10
DEGREE = 4


class System:
    """A, b = A 1, the CPU's numbers (computed once), and plans of the one reordered matrix by configuration"""

    def __init__(self, E, A, **kw):
        self.E, self.A, self.n = E, A, A.shape[0]
        self.cfg = E.make_config(**kw)
        self.m = E.Matrix.from_csr(A.indptr, A.indices, A.data, self.cfg, symmetric=True)
        self.m.reorder(self.cfg)
        self.perm = self.m.reorder_list.copy()
        self.kw = kw
        self.plans = {}
        self.b = A @ np.ones(self.n)
        self.dinv = 1.0 / A.diagonal()
        self.bp, self.inv_diag = E.vector_reorder(self.b, self.perm), E.vector_reorder(self.dinv, self.perm)
        half = sp.diags(np.sqrt(self.dinv))
        self.top = float(spla.eigsh(half @ A @ half, k=1, which="LA", return_eigenvectors=False)[0])

    def plan(self, **over):
        key = tuple(sorted(over.items()))
        if key not in self.plans:
            self.plans[key] = self.E.Plan(self.m, self.E.make_config(**{**self.kw, **over}))
        return self.plans[key]

    def cpu(self, degree, lmax, rounded=False):
        P = sp.csr_matrix((f32(self.A.data), self.A.indices, self.A.indptr), shape=self.A.shape) if rounded else None
        return cc.pcg(self.A, self.b, degree, lmax / 30, lmax, self.dinv, poly_A=P, rtol=RTOL)


@pytest.fixture(scope="module")
def big(E):
    return System(E, spd_matrix(120, 100, 3000, 1), lds_doubles=2048, sym_pairs=0)


@pytest.fixture(scope="module")
def small(E):
    return System(E, spd_matrix(60, 50, 500, 2), lds_doubles=1024, sym_pairs=0)


# ------------------------------------------------------------------ the estimate
@pytest.mark.parametrize("which", ["small", "big"])
def test_lambda_max_is_a_lower_estimate(E, gpu, request, which):
    """0.9 lambda <= the Rayleigh quotient after 20 steps <= lambda (1 + 1e-10); the restatement gives 0.961 and 0.959."""
    s = request.getfixturevalue(which)
    lam = s.plan().lambda_max(s.inv_diag, 20)
    v0 = E.vector_recover(cc.start_vector(s.n), s.perm)      # the device numbers its start vector by the permuted index
    cpu = cc.lambda_max(s.A, s.dinv, 20, v0)
    print(f"{which}: largest eigenvalue {s.top:.6f}, device {lam / s.top:.4f} of it, restatement {cpu / s.top:.4f} "
          f"({cc.lambda_max(s.A, s.dinv, 20) / s.top:.4f} from the start vector in the matrix's own numbering)")
    assert 0.9 * s.top <= lam <= s.top * (1 + 1e-10)
    assert abs(lam - cpu) <= 1e-9 * cpu
    # without inv_diag: the same on A itself
    top_a = float(spla.eigsh(s.A, k=1, which="LA", return_eigenvectors=False)[0])
    lam_a = s.plan().lambda_max(None, 20)
    assert 0.9 * top_a <= lam_a <= top_a * (1 + 1e-10) and abs(lam_a - cc.lambda_max(s.A, None, 20, v0)) <= 1e-9 * lam_a


# ------------------------------------------------------------------ the solve
ARMS = [("plain", dict(), dict(), False),
        ("symmetric-pairs", dict(sym_pairs=1), dict(sym_pairs=1), False),
        ("val-f32-polynomial", dict(), dict(val_f32=1), True),
        ("csr-residual", dict(window_mode=1, lds_doubles=512), dict(window_mode=1, lds_doubles=512), False)]


@pytest.mark.parametrize("name,plan_kw,poly_kw,rounded", ARMS, ids=[a[0] for a in ARMS])
def test_cheb_pcg_against_the_restatement_and_jacobi(E, gpu, big, name, plan_kw, poly_kw, rounded):
    s = big
    plan, poly = s.plan(**plan_kw), s.plan(**poly_kw)
    if name == "symmetric-pairs":
        assert plan.stats["sym_pairs"] > 0.25 * s.A.nnz
    if name == "csr-residual":
        assert plan.stats["nnz_er"] > 0
    if rounded:
        assert poly is not plan and 0 < poly.device_value_bytes[0] < plan.device_value_bytes[0] and (f32(s.A.data) != s.A.data).mean() > 0.9
    lmax = 1.1 * poly.lambda_max(s.inv_diag, 20)
    xp, it, rel = plan.cg_cheb(s.bp, DEGREE, poly_plan=None if poly is plan else poly, lmax=lmax, rtol=RTOL, check_every=1,
                               inv_diag=s.inv_diag)
    x = E.vector_recover(xp, s.perm)
    x_cpu, it_cpu, rz_min = s.cpu(DEGREE, lmax, rounded)
    _, it_jacobi, rel_jacobi = plan.cg(s.bp, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    res = np.linalg.norm(s.A @ x - s.b) / np.linalg.norm(s.b)
    print(f"{name}: {it} iterations (restatement {it_cpu}, Jacobi-PCG on the device {it_jacobi}), rel {rel:.2e}, true residual {res:.2e}, "
          f"multiplies {(1 + DEGREE) * it / it_jacobi:.2f} of Jacobi's")
    assert rz_min > 0 and rel_jacobi <= RTOL
    assert rel <= RTOL
    assert res <= 2e-10
    assert abs(it - it_cpu) <= 2, (it, it_cpu)
    assert np.linalg.norm(x - x_cpu) <= 1e-8 * np.linalg.norm(x_cpu)
    assert 3 * it < it_jacobi, (it, it_jacobi)
    assert (1 + DEGREE) * it <= 1.25 * it_jacobi, (it, it_jacobi)
    # lmax = 0 and lmin = 0: the defaults are this estimate times 1.1 and lmax / 30 -- the same solve
    xd, itd, reld = plan.cg_cheb(s.bp, DEGREE, poly_plan=None if poly is plan else poly, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    assert itd == it and np.linalg.norm(xd - xp) <= 1e-9 * np.linalg.norm(xp)


def test_cheb_pcg_on_a_badly_scaled_system(E, gpu):
    """D A D of test_jacobi_pcg_on_a_badly_scaled_system: the polynomial is one in D^-1 A, which the scaling leaves alone.
    The restatement gives 16 iterations against Jacobi's 70, 1.14 times the multiplies."""
    A0 = spd_matrix(100, 90, 2000, 3)
    d = 10.0 ** np.random.default_rng(5).uniform(-2, 2, A0.shape[0])
    s = System(E, (sp.diags(d) @ A0 @ sp.diags(d)).tocsr(), lds_doubles=2048, sym_pairs=1)
    plan = s.plan()
    lmax = 1.1 * plan.lambda_max(s.inv_diag, 20)
    xp, it, rel = plan.cg_cheb(s.bp, DEGREE, lmax=lmax, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    _, it_cpu, rz_min = s.cpu(DEGREE, lmax)
    _, it_jacobi, rel_jacobi = plan.cg(s.bp, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    print(f"badly scaled: {it} iterations (restatement {it_cpu}, Jacobi-PCG on the device {it_jacobi}), rel {rel:.2e}")
    assert rz_min > 0 and rel <= RTOL and rel_jacobi <= RTOL
    assert abs(it - it_cpu) <= 2 and 3 * it < it_jacobi and (1 + DEGREE) * it <= 1.25 * it_jacobi, (it, it_cpu, it_jacobi)


# ------------------------------------------------------------------ reproducibility
def test_degree_zero_is_scaled_jacobi(E, gpu, big):
    """(lmin, lmax) = (0.5, 1.5): theta = 1, c0 = 1, z = D^-1 r -- ehyb_pcg's preconditioner through other kernels."""
    s = big
    x0, it0, rel0 = s.plan().cg_cheb(s.bp, 0, lmin=0.5, lmax=1.5, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    xj, itj, relj = s.plan().cg(s.bp, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    assert rel0 <= RTOL and relj <= RTOL and abs(it0 - itj) <= 1, (it0, itj)
    assert np.linalg.norm(x0 - xj) <= 1e-9 * np.linalg.norm(xj)


def test_runs_graphs_and_check_every_agree_bit_for_bit(E, gpu, big):
    s = big
    plan, plain = s.plan(), s.plan(graphs=2)
    kw = dict(lmax=2.1, rtol=RTOL, check_every=2, inv_diag=s.inv_diag)       # a given bound: no estimate in the way
    x1, it1, rel1 = plan.cg_cheb(s.bp, DEGREE, **kw)
    x2, it2, rel2 = plan.cg_cheb(s.bp, DEGREE, **kw)
    x3, it3, rel3 = plain.cg_cheb(s.bp, DEGREE, **kw)
    assert rel1 <= RTOL and it1 == it2 == it3 and rel1 == rel2 == rel3
    assert np.array_equal(x1.view(np.int64), x2.view(np.int64)) and np.array_equal(x1.view(np.int64), x3.view(np.int64))
    # with the estimate on the way
    xe1, ite1, rele1 = plan.cg_cheb(s.bp, DEGREE, rtol=RTOL, inv_diag=s.inv_diag)
    xe2, ite2, rele2 = plan.cg_cheb(s.bp, DEGREE, rtol=RTOL, inv_diag=s.inv_diag)
    assert ite1 == ite2 and rele1 == rele2 and np.array_equal(xe1.view(np.int64), xe2.view(np.int64))
    # a fixed number of iterations, looked at after every pair or once in eight
    runs = [p.cg_cheb(s.bp, DEGREE, lmax=2.1, rtol=1e-30, max_iter=12, check_every=ce, inv_diag=s.inv_diag) for ce in (1, 8) for p in (plan, plain)]
    for x, it, rel in runs[1:]:
        assert it == runs[0][1] == 12 and rel == runs[0][2] and 0 < rel < 1e-4 and np.array_equal(x.view(np.int64), runs[0][0].view(np.int64))


# ------------------------------------------------------------------ k right-hand sides
@pytest.fixture(scope="module")
def wide(E):
    """a small window, so that one pass serves four columns"""
    s = System(E, spd_matrix(120, 100, 3000, 1), lds_doubles=20480 // 4, sym_pairs=0, direct=2)
    assert s.plan().spmm_max_k == 4 and s.plan().stats["sym_pairs"] == 0
    assert (s.plan().array("er_seg_row") >= 0).all(), "no residual row may be split into segments"
    return s


def rhs(s, k, seed):
    rng = np.random.default_rng(seed)
    B = np.stack([s.bp * (j + 1) if j % 3 == 0 else s.E.vector_reorder(s.A @ rng.uniform(-1, 1, s.n), s.perm) for j in range(k)])
    B[1] = 0.0          # done at 0 iterations while the others run
    return B


def singles(plan, B, degree, **kw):
    out = [plan.cg_cheb(B[j], degree, **kw) for j in range(len(B))]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


@pytest.mark.parametrize("k", [3, 4, 5])
def test_multi_is_the_single_solve_column_by_column(E, gpu, wide, k):
    """k = 3, 4: one launch three, four columns wide; k = 5: 3 + 2"""
    s = wide
    B = rhs(s, k, seed=k)
    for inv in (s.inv_diag, None):
        kw = dict(lmax=2.1 if inv is not None else 1.05 * float(abs(s.A).sum(axis=1).max()), rtol=RTOL, check_every=2, inv_diag=inv, max_iter=60)
        want = singles(s.plan(), B, DEGREE if inv is not None else 2, **kw)
        got = s.plan().cg_cheb_multi(B, DEGREE if inv is not None else 2, **kw)
        assert_same_bits(got, want, f"k={k} inv_diag={inv is not None}")
        assert got[1][1] == 0 and got[2][1] == 0.0 and not got[0][1].any()
        if inv is not None:
            assert (got[2] <= RTOL).all() and got[1][0] > 0 and got[1][2] > 0, (got[1], got[2])


def test_multi_with_the_polynomial_on_the_val_f32_plan(E, gpu, wide):
    """k_max of a val_f32 plan is 1: three passes of width 1 per multiply of the polynomial, the same bits as three solves"""
    s = wide
    plan, poly = s.plan(), s.plan(val_f32=1)
    assert poly.spmm_max_k == 1 and plan.spmm_max_k == 4
    B = rhs(s, 3, seed=7)
    kw = dict(poly_plan=poly, lmax=2.1, rtol=RTOL, check_every=2, inv_diag=s.inv_diag)
    want = singles(plan, B, DEGREE, **kw)
    got = plan.cg_cheb_multi(B, DEGREE, **kw)
    assert_same_bits(got, want, "val_f32 polynomial, k=3")
    assert (got[2] <= RTOL).all() and got[1][1] == 0
    for j in (0, 2):
        x = E.vector_recover(got[0][j], s.perm)
        bj = E.vector_recover(B[j], s.perm)
        assert np.linalg.norm(s.A @ x - bj) <= 2e-10 * np.linalg.norm(bj)


# ------------------------------------------------------------------ the small ends
@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_small_tridiagonal_systems(E, gpu, n):
    """cheb_cases.tridiagonal, n = 1, 2, 65: one workgroup, most of its threads (all but one) without an element; n = 257:
    two.  The eigenvalues of D^-1 A lie in (0.024, 1.976): lmax = 2.1 is an upper bound.  x against spsolve: cond(A) <= 4.05 / 0.05
    = 81, so rel <= 1e-10 leaves an error below 8.1e-9 -- the 1e-8 of this file."""
    A = cc.tridiagonal(n)
    cfg = E.make_config(sym_pairs=0)
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=True)
    m.reorder(cfg)
    perm = m.reorder_list.copy()
    plan = E.Plan(m, cfg)
    assert plan.stats["sym_pairs"] == 0 and not (plan.array("er_seg_row") < 0).any() and -(-n // 256) == (2 if n == 257 else 1)
    xs = np.stack([np.ones(n), np.cos(np.arange(n) * 0.3) + 2.0, np.random.default_rng(n).uniform(-1, 1, n)])
    B = np.stack([E.vector_reorder(A @ x, perm) for x in xs])
    kw = dict(lmax=2.1, rtol=RTOL, check_every=1, inv_diag=E.vector_reorder(1.0 / A.diagonal(), perm))
    want = singles(plan, B, 3, **kw)
    got = plan.cg_cheb_multi(B, 3, **kw)
    print(f"n={n}: iterations {list(got[1])}, relative residuals {list(got[2])}")
    assert_same_bits(got, want, f"tridiagonal n={n}")
    assert (got[2] <= RTOL).all() and (want[2] <= RTOL).all(), (got[2], want[2])
    for j in range(3):
        x_ref = np.atleast_1d(spla.spsolve(A.tocsc(), A @ xs[j]))
        assert np.linalg.norm(E.vector_recover(got[0][j], perm) - x_ref) <= 1e-8 * np.linalg.norm(x_ref), j
    plan.destroy()


def test_lambda_max_of_a_one_by_one_matrix(E, gpu):
    """[4.0]: u = 1, A u = 4, every scale a power of two -- the quotient is exactly 1 with inv_diag = [0.25], exactly 4 without"""
    A = sp.csr_matrix(np.array([[4.0]]))
    cfg = E.make_config()
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=True)
    m.reorder(cfg)
    plan = E.Plan(m, cfg)
    for iters in (1, 20):
        assert plan.lambda_max(np.array([0.25]), iters) == 1.0
        assert plan.lambda_max(None, iters) == 4.0
    plan.destroy()


# ------------------------------------------------------------------ breakdown, and the state error that needs a device
def test_lmax_below_the_spectrum_breaks_down_or_converges(E, gpu, small):
    """Degree 1 with lmax at half the largest eigenvalue: the polynomial is negative on part of the spectrum.  Either a normal
    return with rel <= rtol, or EhybError with "breakdown" -- never a NaN returned as success."""
    s = small
    b = E.vector_reorder(np.ones(s.n), s.perm)
    _, rz_min = cc.pcg(s.A, np.ones(s.n), 1, 0.5 * s.top / 30, 0.5 * s.top, s.dinv, max_iter=100)[1:]
    assert rz_min < 0, "the restatement must see the indefinite preconditioner"
    try:
        _, it, rel = s.plan().cg_cheb(b, 1, lmax=0.5 * s.top, max_iter=200, rtol=RTOL, inv_diag=s.inv_diag)
        assert not np.isnan(rel) and rel <= RTOL
    except E.EhybError as e:
        assert "breakdown" in str(e)
    # allow_breakdown: the same call returns, with NaN as the residual of a broken solve
    _, it, rel = s.plan().cg_cheb(b, 1, lmax=0.5 * s.top, max_iter=200, rtol=RTOL, inv_diag=s.inv_diag, allow_breakdown=True)
    assert np.isnan(rel) or rel <= RTOL
    X, its, rels = s.plan().cg_cheb_multi(np.stack([b, 2 * b]), 1, lmax=0.5 * s.top, max_iter=200, rtol=RTOL, inv_diag=s.inv_diag,
                                          allow_breakdown=True)
    assert (np.isnan(rels) | (rels <= RTOL)).all() and np.isnan(rels[0]) == np.isnan(rel)


def test_polynomial_plan_never_uploaded(E, gpu, small):
    s = small
    cold = E.Plan(s.m, s.cfg, upload=False)
    lib = E.host._lib.load()
    p = C.c_void_p(0x10000)             # never read: the call fails before device work
    rc = lib.ehyb_pcg_cheb(s.plan().h, cold.h, None, p, p, 2, 0.0, 0.0, 10, 1e-8, 10, None, None, None)
    assert rc == ERR_STATE and b"polynomial" in lib.ehyb_last_error()
    rc = lib.ehyb_pcg_cheb_multi(s.plan().h, cold.h, None, p, s.n, p, s.n, 2, 2, 0.0, 0.0, 10, 1e-8, 10, None, None, None)
    assert rc == ERR_STATE and b"polynomial" in lib.ehyb_last_error()
