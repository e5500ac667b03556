"""The Chebyshev polynomial preconditioner (ehyb_cheb.hip) restated in numpy, and exact cases for its two vector kernels
in the style of solver_cases.py.  No tests here (test_cheb_host.py, test_gpu_cheb_kernels.py, test_gpu_cheb.py).

The restatement follows include/ehyb.h line for line: coeffs (the order of the operations of ehyb_cheb_coeffs), apply
(z = M^-1 r), pcg (the CG around it, the polynomial possibly on another matrix A~: the values rounded to fp32), lambda_max
(the power method of ehyb_lambda_max) and residual_polynomial (the recurrence on a scalar lambda).

The exact cases.  Coefficients are dyadic (3/8 and -5/4), inv_diag is the powers of two of solver_cases.inv_diag_fx, every
vector a scaled integer (Fx), every intermediate asserted below EXACT_LIMIT.  r is the one vector that cannot be wide: r.z
of the start kernel is c0 sum D^-1 r^2, a square; in the step case z_new is chosen (13 bits) and z_old = z_new - d follows,
so that r.z_new stays a sum of 26-bit products.  NARROW lists these exceptions to the width rule of solver_cases.py.
"""
import numpy as np

from exact_cases import EXACT_LIMIT
from solver_cases import STEP_GRID, S, WANTED_PROFILES, Fx, asserted_walk, dyadic, inv_diag_fx, odd_ints, partials  # noqa: F401

SIZES = [0, 1, 257, S + 1, 3 * S + 1, 4 * S + 1, 7 * S + 1, 8 * S + 300]   # of solver_cases.SIZES: together they cover WANTED_PROFILES
MAX_DEGREE = 16               # EHYB_CHEB_MAX_DEGREE
C0 = (3, 3)                   # the start kernel's coefficient: 3/8
A_B = ((3, 3), (-5, 2))       # the step kernel's a = 3/8, b = -5/4
NARROW = {("cheb_start", "r"), ("cheb_step", "r")}


# ------------------------------------------------------------------ the restatement
def coeffs(lmin, lmax, degree):
    """c0, a[0 .. degree), b[0 .. degree) in the order of the operations the header states"""
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    c0, rho = 1.0 / theta, 1.0 / sigma
    a, b = np.zeros(degree), np.zeros(degree)
    for j in range(degree):
        rho_j = 1.0 / (2.0 * sigma - rho)
        a[j], b[j] = rho_j * rho, 2.0 * rho_j / delta
        rho = rho_j
    return c0, a, b


def apply(mul, dinv, r, c0, a, b):
    """z = M^-1 r; mul(v) = A~ v; dinv None or the vector inv_diag"""
    s = (lambda v: v) if dinv is None else (lambda v: dinv * v)
    d = c0 * s(r)
    z, w = d.copy(), r
    for aj, bj in zip(a, b):
        w = w - mul(d)
        d = aj * d + bj * s(w)
        z = z + d
    return z


def pcg(A, b, degree, lmin, lmax, dinv=None, poly_A=None, max_iter=1000, rtol=1e-10, x0=None, check_every=1):
    """The solve of ehyb_pcg_cheb, iteration for iteration (x0 None: 0; the stopping test is made every check_every
    iterations, as the device makes it) -> (x, iterations, smallest r.z seen)"""
    P = A if poly_A is None else poly_A
    c0, ca, cb = coeffs(lmin, lmax, degree)
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = b.copy() if x0 is None else b - A @ x0
    z = apply(lambda v: P @ v, dinv, r, c0, ca, cb)
    p, rz, bb = z.copy(), r @ z, (b @ b) or 1.0
    it, rz_min = 0, rz
    while it < max_iter and (it % check_every or np.sqrt((r @ r) / bb) > rtol):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = apply(lambda v: P @ v, dinv, r, c0, ca, cb)
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
        rz_min = min(rz_min, rz)
        it += 1
    return x, it, rz_min


# ------------------------------------------------------------------ the freezing mix at full size (test_gpu_cheb_full.py)
# The right-hand-side bank of test_gpu_solver_kernels.MIX_KINDS with the e of its "near" columns (b = A x*, x0 = x* + e u)
# chosen for this solver.  Relative residual per unit e on spd_matrix(1024, 921, 3000, 21) after 0, 2, 4, 6, 8 iterations, from
# pcg above with lmax = 2.1 and inv_diag (Jacobi) or lmax = 1.05 max_i sum_j |a_ij| without, lmin = lmax / 30:
#   degree 4, Jacobi (the same to three digits with the polynomial on the fp32-rounded matrix)
#                      3.4  0.118  0.0046  0.00127  0.00037     a random b from x0 = 0 is at 9.9e-5 after 12
#   degree 2, plain    3.4  0.146  0.0299  0.0107   0.0049                                   7.8e-3
#   degree 1, Jacobi   3.4  0.264  0.0328  0.0158   0.0078                                   1.2e-2
#   degree 0, Jacobi   3.4  0.354  0.108   0.0487   0.0264   (any lmin, lmax: a scaled z)    7.1e-2
# MIX_E[degree, Jacobi] = the three e that cross MIX_RTOL = 1e-6 at check points 2, 4 and 6 (check_every = 2): each near the
# geometric middle of its interval, 1e-6 / sqrt(residual before * residual after), a factor of 1.4 to 4.8 from either edge.
MIX_E = {(4, True): (5e-6, 1e-4, 5e-4), (2, False): (1.5e-6, 1.5e-5, 5.6e-5), (1, True): (1e-6, 1.1e-5, 4.4e-5),
         (0, True): (9e-7, 5e-6, 1.4e-5)}


def mix_bank(A, kinds, seed=77):
    """The bank of big_spd (test_gpu_solver_kernels.py), drawn in the same order, without its e: -> (x*, B, U, rank) in A's own
    numbering; U[j] is the u of a "near" column (uniform in [-1, 1]) and None otherwise; rank[j] of a near column says which of
    the three e it takes: 0, 1, 2 for the smallest, middle and largest e of `kinds`."""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    x_star = np.sin(np.arange(n) * 1e-3) + 1.5
    order = sorted({e for kind, e in kinds if kind == "near"})
    B, U, rank = [], [], []
    for kind, e in kinds:
        if kind == "near":
            B.append(A @ x_star)
            U.append(rng.uniform(-1, 1, n))
            rank.append(order.index(e))
        else:
            B.append(np.zeros(n) if kind == "zero" else rng.uniform(-1, 1, n))
            U.append(None)
            rank.append(None)
    return x_star, B, U, rank


def mix_x0(x_star, U, rank, es):
    """the start vectors of the bank for the three e of MIX_E"""
    return [np.zeros_like(x_star) if u is None else x_star + es[k] * u for u, k in zip(U, rank)]


def tridiagonal(n):
    """2.05 on the diagonal, -1 beside it: SPD, strictly diagonally dominant, any n >= 1"""
    import scipy.sparse as sp

    return sp.diags([np.full(max(n - 1, 0), -1.0), np.full(n, 2.05), np.full(max(n - 1, 0), -1.0)], [-1, 0, 1], shape=(n, n)).tocsr()


def jacobi_pcg(A, b, dinv, max_iter=1000, rtol=1e-10):
    """ehyb_pcg's recurrences -> iterations"""
    x, r = np.zeros_like(b), b.copy()
    z = dinv * r
    p, rz, bb, it = z.copy(), r @ z, b @ b, 0
    while it < max_iter and np.sqrt((r @ r) / bb) > rtol:
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = dinv * r
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
        it += 1
    return it


def start_vector(n):
    """v_i = 1 + (i mod 7) / 8 -- by the index the plan sees: the permuted numbering"""
    return 1.0 + (np.arange(n) % 7) / 8.0


def lambda_max(A, dinv, iters=20, v0=None):
    """ehyb_lambda_max: `iters` steps v <- D^-1 A v / ||D^-1 A v|| from v0 (None: start_vector in A's own numbering), then
    (v.Av) / (v.Dv)"""
    n = A.shape[0]
    d = np.ones(n) if dinv is None else dinv
    v = start_vector(n) if v0 is None else v0
    for _ in range(iters):
        u = d * (A @ v)
        v = u / np.linalg.norm(u)
    return (v @ (A @ v)) / (v @ (v / d))


def residual_polynomial(lam, c0, a, b):
    """(p(lambda), 1 - lambda p(lambda)) for an array of scalars: the recurrence with A = lambda, D = 1, r = 1"""
    lam = np.asarray(lam, dtype=np.float64)
    z = apply(lambda v: lam * v, None, np.ones_like(lam), c0, a, b)
    return z, 1.0 - lam * z


def chebyshev_T(m, x):
    """T_m(x) by the three-term recurrence (any real x)"""
    x = np.asarray(x, dtype=np.float64)
    t0, t1 = np.ones_like(x), x.copy()
    if m == 0:
        return t0
    for _ in range(m - 1):
        t0, t1 = t1, 2.0 * x * t1 - t0
    return t1


# ------------------------------------------------------------------ exact cases of the two kernels
def _ex(v, what="an intermediate"):
    """v itself, asserted to be below EXACT_LIMIT units: a value the kernel forms on the way (fused or not)"""
    assert v.peak() < EXACT_LIMIT, f"{what}: {v.peak():.3e} units, not exact in fp64"
    return v


def _scaled(v, dinv):
    return v if dinv is None else _ex(v * dinv)


def start_case(n, with_dinv, seed=0, grid=STEP_GRID):
    """d = z = c0 D^-1 r; partials of r.z"""
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    coef = dyadic(*C0)
    r = Fx(odd_ints(rng, n, 12), 3)
    d = _ex(coef * _scaled(r, dinv))
    prod = {"rz": r * d}
    return {"in": {"r": r}, "dinv": dinv, "coef": coef, "out": {"d": d, "z": d},
            "sums": {"rz": partials(prod["rz"], grid, "cheb_start rz")}, "products": prod}


def step_case(n, with_dinv, seed=0, grid=STEP_GRID):
    """w_out = w_in - t; d = a d + b D^-1 w_out; z += d; partials of r.z"""
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    a, b = dyadic(*A_B[0]), dyadic(*A_B[1])
    w_in, t, d_old = Fx(odd_ints(rng, n, 26)), Fx(odd_ints(rng, n, 26), 1), Fx(odd_ints(rng, n, 27), 2)
    w = _ex(w_in - t)
    d = _ex(_ex(a * d_old) + _ex(b * _scaled(w, dinv)))
    z_new = Fx(odd_ints(rng, n, 13), d.e)
    z_old = _ex(z_new - d)
    r = Fx(odd_ints(rng, n, 13), 3)
    prod = {"rz": r * z_new}
    return {"in": {"w_in": w_in, "t": t, "d": d_old, "z": z_old, "r": r}, "dinv": dinv, "a": a, "b": b,
            "out": {"w_out": w, "d": d, "z": z_new},
            "sums": {"rz": partials(prod["rz"], grid, "cheb_step rz")}, "products": prod}


def all_cases(n):
    for with_dinv in (False, True):
        yield "cheb_start", start_case(n, with_dinv, seed=n % 97)
        yield "cheb_step", step_case(n, with_dinv, seed=n % 89)
