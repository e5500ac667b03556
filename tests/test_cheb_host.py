"""The Chebyshev preconditioner on the host: ehyb_cheb_coeffs against the numpy restatement (cheb_cases.py), the residual
polynomial the coefficients stand for, every argument check of ehyb_pcg_cheb / ehyb_pcg_cheb_multi / ehyb_lambda_max on plans
that were never uploaded (the checks come before any device work), and the exact cases of the two kernels checked against
themselves as test_solver_cases.py checks those of the CG kernels.  Nothing here needs a GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import cheb_cases as cc
import solver_cases as sc
from test_cg_multi_host import ERR_ARG, ERR_STATE, host_plan
from test_solver_cases import check, fr

DEGREES = [0, 1, 2, 4, 8, 16]
INTERVALS = [(0.07, 2.1), (0.5, 1.5), (1e-3, 1e3)]


def ulps(got, want):
    return np.abs(np.asarray(got, dtype=np.float64).view(np.int64) - np.asarray(want, dtype=np.float64).view(np.int64))


# ------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("lmin,lmax", INTERVALS)
@pytest.mark.parametrize("degree", DEGREES)
def test_coefficients_against_the_restatement(E, lmin, lmax, degree):
    """Within 4 ulp per coefficient: the host compiler may contract a multiply-add (2 sigma - rho), the recurrence carries it on."""
    c0, a, b = E.cheb_coeffs(lmin, lmax, degree)
    w0, wa, wb = cc.coeffs(lmin, lmax, degree)
    assert a.shape == b.shape == (degree,)
    assert ulps(c0, w0) <= 4 and (ulps(a, wa) <= 4).all() and (ulps(b, wb) <= 4).all(), (ulps(c0, w0), ulps(a, wa), ulps(b, wb))
    assert (a > 0).all() and (b > 0).all() and c0 > 0
    if (lmin, lmax) == (0.5, 1.5):
        assert c0 == 1.0             # theta = 1
    # the outputs of a shorter recurrence are the head of a longer one's; entries past `degree` are not written
    lib = E.host._lib.load()
    c = C.c_double(0)
    ga, gb = np.full(cc.MAX_DEGREE + 1, -7.0), np.full(cc.MAX_DEGREE + 1, -7.0)
    assert lib.ehyb_cheb_coeffs(lmin, lmax, degree, C.byref(c), ga.ctypes.data_as(C.POINTER(C.c_double)), gb.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.array_equal(ga[:degree], a) and np.array_equal(gb[:degree], b) and (ga[degree:] == -7.0).all() and (gb[degree:] == -7.0).all()
    _, a16, b16 = E.cheb_coeffs(lmin, lmax, cc.MAX_DEGREE)
    assert np.array_equal(a16[:degree], a) and np.array_equal(b16[:degree], b)


def test_coefficient_argument_errors(E):
    lib = E.host._lib.load()
    c = C.c_double(0)
    buf = np.zeros(cc.MAX_DEGREE)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    for lmin, lmax, degree in [(0.1, 1.0, -1), (0.1, 1.0, cc.MAX_DEGREE + 1), (1.0, 1.0, 2), (2.0, 1.0, 2), (0.0, 1.0, 2), (-1.0, 1.0, 2),
                               (float("nan"), 1.0, 2), (0.1, float("nan"), 2), (0.1, float("inf"), 2)]:
        assert lib.ehyb_cheb_coeffs(lmin, lmax, degree, C.byref(c), p, p) == ERR_ARG, (lmin, lmax, degree)
        assert lib.ehyb_last_error()
    assert lib.ehyb_cheb_coeffs(0.1, 1.0, 2, None, p, p) == ERR_ARG
    assert lib.ehyb_cheb_coeffs(0.1, 1.0, 2, C.byref(c), None, p) == ERR_ARG
    assert lib.ehyb_cheb_coeffs(0.1, 1.0, 0, C.byref(c), None, None) == 0          # degree 0 writes neither a nor b
    with pytest.raises(E.EhybError):
        E.cheb_coeffs(1.0, 0.5, 3)


# ------------------------------------------------------------------ the residual polynomial
@pytest.mark.parametrize("lmin,lmax", INTERVALS)
@pytest.mark.parametrize("degree", DEGREES)
def test_residual_polynomial_is_the_scaled_chebyshev_polynomial(E, lmin, lmax, degree):
    """1 - lambda p(lambda) = T_{m+1}((theta - lambda) / delta) / T_{m+1}(sigma) on 2001 points of [1e-3, 1.1 lmax], within
    1e-11 (the restatement's own coefficients give <= 4e-13 on (0.07, 2.1) and <= 1e-15 on (0.5, 1.5)), and p > 0 up to
    lmax.  On (1e-3, 1e3) the quotient itself grows to 2e4 beyond lmax at degree 16 -- one rounding of it is 4e-12 -- so
    there the bound is relative to the quotient where that is above 1: 1e-11 max(1, |quotient|)."""
    c0, a, b = E.cheb_coeffs(lmin, lmax, degree)
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    lam = np.linspace(1e-3, 1.1 * lmax, 2001)
    p, res = cc.residual_polynomial(lam, c0, a, b)
    want = cc.chebyshev_T(degree + 1, (theta - lam) / delta) / cc.chebyshev_T(degree + 1, np.float64(theta / delta))
    err = np.abs(res - want)
    print(f"[{lmin}, {lmax}] degree {degree}: max |error| {err.max():.3e}, max |quotient| {np.abs(want).max():.3e}")
    bound = 1e-11 * (np.maximum(1.0, np.abs(want)) if (lmin, lmax) == (1e-3, 1e3) else 1.0)
    assert (err <= bound).all(), err.max()
    assert (p[lam <= lmax] > 0).all()
    if degree == 1 and (lmin, lmax) == (0.07, 2.1):
        # why lmax must be an upper bound: degree 1 is negative at 1.1 lmax
        assert p[-1] < 0


def test_restatement_on_a_small_matrix():
    """apply() is p(D^-1 A) D^-1 r: on a diagonal matrix with D = I it is the scalar polynomial entry by entry, and the
    preconditioned CG of the restatement solves a small SPD system in fewer iterations than Jacobi."""
    import scipy.sparse as sp

    lam = np.linspace(0.1, 2.0, 50)
    c0, a, b = cc.coeffs(0.07, 2.1, 5)
    z = cc.apply(lambda v: lam * v, None, np.ones(50), c0, a, b)
    assert np.allclose(z, cc.residual_polynomial(lam, c0, a, b)[0], rtol=0, atol=0)
    n = 400
    A = (sp.diags([-1.0, 2.05, -1.0], [-1, 0, 1], shape=(n, n))).tocsr()
    dinv = 1.0 / A.diagonal()
    rhs = A @ np.ones(n)
    lm = cc.lambda_max(A, dinv, 20)
    top = np.linalg.eigvalsh((sp.diags(np.sqrt(dinv)) @ A @ sp.diags(np.sqrt(dinv))).toarray())[-1]
    assert 0.9 * top <= lm <= top * (1 + 1e-10)
    x, it, rz_min = cc.pcg(A, rhs, 4, 1.1 * lm / 30, 1.1 * lm, dinv)
    assert rz_min > 0 and np.linalg.norm(A @ x - rhs) <= 2e-10 * np.linalg.norm(rhs)
    assert 3 * it < cc.jacobi_pcg(A, rhs, dinv)


# ------------------------------------------------------------------ argument checks, without a device
B, X, D = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000)   # never read: every call fails before device work


@pytest.fixture(scope="module")
def plans(E):
    """never uploaded: the plan, a second one of the same matrix, one over half the rows, one of another size"""
    cfg = E.make_config(direct=2)
    small = E.Matrix.generate("fem3d", 15000, 3, 22, 22, 13500, 1, 1, cfg=cfg)
    small.reorder(cfg)
    out = dict(plan=host_plan(E, direct=2), twin=host_plan(E, direct=2, val_f32=1), half=host_plan(E, half=True, direct=2),
               other=E.Plan(small, cfg, upload=False))
    assert out["other"].n != out["plan"].n and out["half"].n == out["plan"].n and out["half"].rows[1] < out["plan"].n
    return out


def call(lib, plans, multi, plan="plan", poly="twin", d=D, b=B, x=X, ldb=None, ldx=None, k=3, degree=4, lmin=0.0, lmax=0.0, max_iter=50,
         rtol=1e-8):
    h = None if plan is None else plans[plan].h
    ph = None if poly is None else plans[poly].h
    n = plans["plan"].n
    it, rel = (C.c_int * 16)(), (C.c_double * 16)()
    if multi:
        rc = lib.ehyb_pcg_cheb_multi(h, ph, d, b, n if ldb is None else ldb, x, n if ldx is None else ldx, k, degree, lmin, lmax, max_iter,
                                     rtol, 10, None, it, rel)
    else:
        rc = lib.ehyb_pcg_cheb(h, ph, d, b, x, degree, lmin, lmax, max_iter, rtol, 10, None, it, rel)
    return rc, lib.ehyb_last_error()


# in the order the header states, each with the words its message must hold
ARG_ERRORS = [(dict(degree=-1), b"degree"), (dict(degree=cc.MAX_DEGREE + 1), b"degree"), (dict(lmin=2.0, lmax=2.0), b"lmin"),
              (dict(lmin=3.0, lmax=2.0), b"lmin"), (dict(lmin=float("nan")), b"NaN"), (dict(lmax=float("nan")), b"NaN"),
              (dict(poly="other"), b"rows"), (dict(poly="half"), b"all rows")]


@pytest.mark.parametrize("multi", [False, True], ids=["one", "multi"])
def test_argument_errors_in_the_stated_order(E, plans, multi):
    lib = E.host._lib.load()
    # nothing wrong but the upload: the plan's comes first, whatever the polynomial's plan is (NULL = the plan itself)
    for poly in ("twin", None, "plan"):
        rc, msg = call(lib, plans, multi, poly=poly)
        assert rc == ERR_STATE and b"upload" in msg and b"polynomial" not in msg, msg
    for kw in (dict(degree=0), dict(degree=cc.MAX_DEGREE), dict(lmin=0.0, lmax=5.0), dict(lmin=-1.0, lmax=-1.0), dict(lmin=7.0),
               dict(lmin=1.0, lmax=1.0 + 1e-9), dict(d=None), dict(max_iter=0, rtol=0.0)):
        assert call(lib, plans, multi, **kw)[0] == ERR_STATE, kw
    # what the existing solvers reject comes first
    earlier = [dict(b=None), dict(x=None), dict(max_iter=-1), dict(rtol=-1.0), dict(rtol=float("nan")), dict(plan="half", poly="half")]
    if multi:
        earlier = [dict(k=0), dict(ldb=plans["plan"].n - 1), dict(ldx=plans["plan"].n - 1)] + earlier
    for kw in earlier:
        rc, msg = call(lib, plans, multi, **kw)
        assert rc == ERR_ARG and msg, kw
        rc2, msg2 = call(lib, plans, multi, **{**kw, "degree": -1})
        assert rc2 == ERR_ARG and msg2 == msg, (kw, msg, msg2)
    assert call(lib, plans, multi, plan=None)[0] == ERR_ARG
    # every check of this solver: an argument error, before the state error, and before every later one of the list
    for i, (kw, word) in enumerate(ARG_ERRORS):
        rc, msg = call(lib, plans, multi, **kw)
        assert rc == ERR_ARG and word in msg, (kw, msg)
        for later, _ in ARG_ERRORS[i + 1:]:
            if set(later) & set(kw):
                continue
            rc2, msg2 = call(lib, plans, multi, **{**later, **kw})
            assert rc2 == ERR_ARG and msg2 == msg, (kw, later, msg2)
    if multi:
        # k and the leading dimensions before everything else
        rc, msg = call(lib, plans, multi, k=0, b=None, degree=-1)
        assert rc == ERR_ARG and b"right-hand sides" in msg


def test_lambda_max_arguments(E, plans):
    lib = E.host._lib.load()
    lam = C.c_double(-3.0)
    h = plans["plan"].h
    assert lib.ehyb_lambda_max(h, D, 20, None, C.byref(lam)) == ERR_STATE and b"upload" in lib.ehyb_last_error()
    assert lib.ehyb_lambda_max(h, None, 1, None, C.byref(lam)) == ERR_STATE
    for iters in (0, -5):
        assert lib.ehyb_lambda_max(h, D, iters, None, C.byref(lam)) == ERR_ARG and b"steps" in lib.ehyb_last_error()
    assert lib.ehyb_lambda_max(None, D, 20, None, C.byref(lam)) == ERR_ARG
    assert lib.ehyb_lambda_max(h, D, 20, None, None) == ERR_ARG
    assert lib.ehyb_lambda_max(plans["half"].h, D, 20, None, C.byref(lam)) == ERR_ARG and b"all rows" in lib.ehyb_last_error()
    assert lam.value == -3.0


def test_step_argument_errors(E):
    lib = E.host._lib.load()
    p = C.c_void_p(0x10000)
    assert lib.ehyb_cheb_start_step(-1, p, None, 0.5, p, p, p, 0, None) == ERR_ARG
    assert lib.ehyb_cheb_start_step(8, None, None, 0.5, p, p, p, 0, None) == ERR_ARG
    assert lib.ehyb_cheb_start_step(8, p, None, 0.5, p, p, None, 1, None) == ERR_ARG
    for rz in (-2, 2):
        assert lib.ehyb_cheb_start_step(8, p, None, 0.5, p, p, p, rz, None) == ERR_ARG
        assert lib.ehyb_cheb_step(8, p, p, None, 0.5, 0.5, p, p, p, p, p, rz, None) == ERR_ARG
    assert lib.ehyb_cheb_step(-1, p, p, None, 0.5, 0.5, p, p, p, p, p, 0, None) == ERR_ARG
    assert lib.ehyb_cheb_step(8, p, None, None, 0.5, 0.5, p, p, p, p, p, 0, None) == ERR_ARG
    assert lib.ehyb_cheb_step(8, p, p, None, 0.5, 0.5, p, p, p, None, p, 0, None) == ERR_ARG
    assert lib.ehyb_cheb_step(8, p, p, None, 0.5, 0.5, p, p, p, p, None, 1, None) == ERR_ARG


# ------------------------------------------------------------------ the exact cases, checked against themselves
def test_the_sizes_cover_the_walk():
    seen = set()
    for n in cc.SIZES:
        assert n in sc.SIZES
        seen |= cc.asserted_walk(n)
    assert seen >= cc.WANTED_PROFILES, cc.WANTED_PROFILES - seen
    assert Fraction(cc.C0[0], 2 ** cc.C0[1]) == Fraction(3, 8) and [Fraction(n, 2 ** e) for n, e in cc.A_B] == [Fraction(3, 8), Fraction(-5, 4)]


@pytest.mark.parametrize("n,grid", [(0, 1), (1, 1), (257, 1), (700, 2), (2300, 2), (4 * 512 + 3, 2)])
@pytest.mark.parametrize("with_dinv", [False, True])
def test_reference_against_fractions(n, grid, with_dinv):
    d = fr(sc.inv_diag_fx(n)) if with_dinv else [Fraction(1)] * n
    c = cc.start_case(n, with_dinv, seed=3, grid=grid)
    r = fr(c["in"]["r"])
    z = [Fraction(3, 8) * ri * di for ri, di in zip(r, d)]
    assert fr(c["coef"]) == [Fraction(3, 8)]
    check(c, {"d": z, "z": z}, {"rz": [ri * zi for ri, zi in zip(r, z)]}, grid)

    c = cc.step_case(n, with_dinv, seed=4, grid=grid)
    i = {k: fr(v) for k, v in c["in"].items()}
    a, b = fr(c["a"])[0], fr(c["b"])[0]
    assert (a, b) == (Fraction(3, 8), Fraction(-5, 4))
    w = [wi - ti for wi, ti in zip(i["w_in"], i["t"])]
    dn = [a * di + b * wi * ei for di, wi, ei in zip(i["d"], w, d)]
    zn = [zi + di for zi, di in zip(i["z"], dn)]
    check(c, {"w_out": w, "d": dn, "z": zn}, {"rz": [ri * zi for ri, zi in zip(i["r"], zn)]}, grid)


@pytest.mark.parametrize("n", cc.SIZES)
def test_precondition_and_width_at_every_size(n):
    """Building a case asserts that every intermediate and every slot's magnitudes stay below EXACT_LIMIT; on top: every vector
    turns into float64 exactly, at least half of every vector read and of every product summed is wide (more than 24
    significant bits: a pass through fp32 would show), r -- whose square is summed -- being the listed exception."""
    for name, c in cc.all_cases(n):
        for group, length in (("in", n), ("out", n), ("sums", sc.STEP_GRID)):
            for k, v in c[group].items():
                f = v.f(f"{name} {k}")
                assert len(f) == length and np.array_equal(f * 2.0 ** v.e, v.m.astype(np.float64)), (name, group, k)
        for k, v in c["products"].items():
            assert int(np.abs(v.m).sum()) < sc.EXACT_LIMIT, (name, k)
            assert (sc.significant_bits(v.m) > 24).sum() >= n // 2, (name, k, "products too narrow for fp32 to show")
        for k, v in c["in"].items():
            wide = int((sc.significant_bits(v.m) > 24).sum())
            if (name, k) in cc.NARROW:
                assert wide == 0, (name, k)
            else:
                assert wide >= n // 2, (name, k, wide)


# ------------------------------------------------------------------ what test_gpu_cheb_full.py rests on
def test_the_walk_at_full_size_and_at_the_size_of_the_k_column_tests():
    """n = 943,104: the solve launches the grid of the step entry points, every thread runs an unrolled body; at 12,000 none"""
    n = 1024 * 921
    assert sc.solver_grid(n) == sc.STEP_GRID and sc.walk_profile(n, sc.STEP_GRID) == {(1, 3), (2, 0)}
    assert sc.walk_profile(12000, sc.solver_grid(12000)) == {(0, 0), (0, 1)}
    assert -(-n // sc.S) == 8, "trips of the lambda kernels' loop"
    assert [sc.solver_grid(k) for k in (1, 2, 65, 257)] == [1, 1, 1, 2]


def test_the_restatement_from_a_start_vector_and_the_mix_bank():
    """pcg with x0 and check_every on a tridiagonal system: x0 = 0 is the default, the stopping test is made at multiples of
    check_every only; the bank keeps the order of the draws and gives every near column its e by rank"""
    A = cc.tridiagonal(65)
    assert abs(A - A.T).nnz == 0 and A.diagonal().min() == 2.05 and A.nnz == 3 * 65 - 2 and cc.tridiagonal(1).toarray().tolist() == [[2.05]]
    b = A @ np.ones(65)
    x, it, _ = cc.pcg(A, b, 3, 4.05 / 30, 4.05, rtol=1e-10)
    x2, it2, _ = cc.pcg(A, b, 3, 4.05 / 30, 4.05, rtol=1e-10, x0=np.zeros(65), check_every=1)
    assert it == it2 and np.array_equal(x, x2) and np.abs(x - 1).max() < 1e-8
    x4, it4, _ = cc.pcg(A, b, 3, 4.05 / 30, 4.05, rtol=1e-10, check_every=4)
    assert it4 % 4 == 0 and it <= it4 < it + 4
    assert cc.pcg(A, b, 3, 4.05 / 30, 4.05, x0=np.ones(65))[1] == 0
    kinds = [("near", 5e-6), ("zero", 0), ("random", 0), ("near", 1e-6), ("near", 1.2e-5), ("near", 5e-6)]
    x_star, B, U, rank = cc.mix_bank(A, kinds)
    assert rank == [1, None, None, 0, 2, 1] and [u is None for u in U] == [False, True, True, False, False, False]
    assert not B[1].any() and np.array_equal(B[0], A @ x_star) and np.abs(B[2]).max() <= 1 and not np.array_equal(U[0], U[3])
    X0 = cc.mix_x0(x_star, U, rank, (1.0, 2.0, 3.0))
    assert np.array_equal(X0[3], x_star + U[3]) and np.array_equal(X0[4], x_star + 3.0 * U[4]) and not X0[1].any()
    for es in cc.MIX_E.values():
        assert es[0] < es[1] < es[2]
