"""The factorised sparse approximate inverse (fsai.cpp, ehyb_fsai.hip) restated in numpy, and the bounds its tests hold a row
of G to.  No tests here (test_fsai_host.py, test_gpu_fsai_kernels.py, test_gpu_fsai.py).

The restatement follows include/ehyb.h: pattern (the columns of every row of G, with the row cap and its ties rule), factor
(one dense SPD solve per row, numpy's Cholesky; the fallback to the Jacobi form), apply (z = G^T (G r)) and pcg (the CG around
it, the stopping test made every check_every iterations as the device makes it).  Everything is in the permuted numbering: the
matrix after ehyb_matrix_reorder, taken to be symmetric.

The bounds.  A row g of m entries solves S g = e_m / g_m through S = L L^T and one triangular solve.  The backward error of the
two together is (3 m + 1) eps |L| |L^T| componentwise (Higham, Accuracy and Stability, theorems 10.3 and 8.5), and
|| |L| |L^T| ||_inf <= m ||S||_inf for an SPD S; the scaling by g_m adds a rounding or two.  The tests use
    residual   || S g - e_m / g_m ||_inf <= 8 m eps ||S||_inf ||g||_inf
    forward    || g - g' ||_inf <= cond_inf(S) 8 m eps ||g||_inf     for two computations g, g' of one row (the host's, the device's)
The forward bound is the usual first-order one, cond times the backward error; between two computed rows it leaves the margin
of 8 m over the two (3 m + 1) constants."""
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -53              # the unit roundoff of fp64
MAX_ROW = 64                  # EHYB_FSAI_MAX_ROW


# ------------------------------------------------------------------ the restatement
def pattern(A, row_cap=0):
    """-> (row_ptr (n + 1,) int64, cols int32, capped rows): J_i = the stored columns j < i of row i -- the row_cap - 1 of largest
    |a_ij| where there are more, ties to the lower column -- and i, rising"""
    A = sp.csr_matrix(A)
    cap = MAX_ROW if row_cap <= 0 else row_cap
    rows, capped = [], 0
    for i in range(A.shape[0]):
        c, v = A.indices[A.indptr[i]:A.indptr[i + 1]], A.data[A.indptr[i]:A.indptr[i + 1]]
        below = c < i
        c, v = c[below], np.abs(v[below])
        order = np.argsort(c, kind="stable")
        c, v = c[order], v[order]
        if len(c) > cap - 1:
            keep = np.argsort(-v, kind="stable")[:cap - 1]      # stable: of equal magnitudes the lower column first
            c = np.sort(c[keep])
            capped += 1
        rows.append(np.concatenate([c, [i]]))
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return row_ptr, np.concatenate(rows).astype(np.int32), capped


def block(A, J):
    """S = A[J, J] with its lower triangle mirrored (dense)"""
    S = np.tril(np.asarray(A[J][:, J].todense()))
    return S + np.tril(S, -1).T


def factor_row(S):
    """-> (g, fell back): L^T g = e_m with S = L L^T; a block numpy cannot factor, or a diagonal that is not positive: Jacobi"""
    m = len(S)
    e = np.zeros(m)
    e[-1] = 1.0
    try:
        with np.errstate(all="ignore"):
            L = np.linalg.cholesky(S)
        if not np.isfinite(L).all():
            raise np.linalg.LinAlgError
        return np.linalg.solve(L.T, e), False
    except np.linalg.LinAlgError:
        return e / np.sqrt(S[-1, -1]), True


def factor(A, row_ptr, cols):
    """-> (vals, fallback rows)"""
    A = sp.csr_matrix(A)
    vals, fell = np.zeros(len(cols)), 0
    for i in range(len(row_ptr) - 1):
        J = cols[row_ptr[i]:row_ptr[i + 1]]
        vals[row_ptr[i]:row_ptr[i + 1]], fb = factor_row(block(A, J))
        fell += fb
    return vals, fell


def matrix(row_ptr, cols, vals):
    n = len(row_ptr) - 1
    return sp.csr_matrix((vals, cols, row_ptr), shape=(n, n))


def apply(G, r):
    """z = G^T (G r)"""
    return G.T @ (G @ r)


def pcg(A, b, G, max_iter=1000, rtol=1e-10, x0=None, check_every=1):
    """The solve of ehyb_pcg_fsai, iteration for iteration -> (x, iterations)"""
    Gt = G.T.tocsr()
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = b.copy() if x0 is None else b - A @ x0
    t = G @ r
    z = Gt @ t
    p, rz, bb = z.copy(), t @ t, (b @ b) or 1.0
    it = 0
    while it < max_iter and (it % check_every or np.sqrt((r @ r) / bb) > rtol):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        t = G @ r
        z = Gt @ t
        rz, rz_old = t @ t, rz
        p = z + (rz / rz_old) * p
        it += 1
    return x, it


# ------------------------------------------------------------------ the freezing mix at full size (test_gpu_precond_full.py)
# The right-hand-side bank of test_gpu_solver_kernels.MIX_KINDS (cheb_cases.mix_bank, mix_x0) with the e of its "near" columns
# (b = A x*, x0 = x* + e u) chosen for this solver.  Relative residual per unit e on spd_matrix(1024, 921, 3000, 21) after 0, 2, 4,
# 6, 8 iterations, from pcg above with G = matrix(row_ptr, cols, vals) of the library's host object (no row capped, none fallen
# back, 2,830,367 entries; factor's Python loop over 943,104 rows is too slow, and test_fsai_host.py holds the host factor to its
# bounds), everything in the permuted numbering:
#                      3.40  0.167  0.0348  0.0124  0.0059     a random b from x0 = 0 is at 1.25e-2 after 12
# (the two "near" columns measured, u of columns 0 and 3, agree to two digits.)  MIX_E = the three e that cross MIX_RTOL = 1e-6 at
# check points 2, 4 and 6 (check_every = 2): each near the geometric middle of its interval, 1e-6 / sqrt(residual before *
# residual after), a factor of 1.7 to 4.6 from either edge.  With them pcg above stops the seven columns of the bank after 4, 0,
# 12, 2, 6, 4, 12 iterations.  These numbers are measured from the restatement on the CPU, not from the device; no host test
# repeats them: the restatement alone takes 2.0 s for the bank, the matrix, its reordering and the host object another 2 s, and
# the slowest host test of this solver takes 0.9 s.
MIX_E = (1.3e-6, 1.3e-5, 4.8e-5)


def jacobi_pcg(A, b, max_iter=1000, rtol=1e-10):
    """-> iterations of CG preconditioned with the diagonal, the stopping test made every iteration"""
    dinv = 1.0 / A.diagonal()
    x, r = np.zeros_like(b), b.copy()
    z = dinv * r
    p, rz, bb = z.copy(), r @ z, (b @ b) or 1.0
    it = 0
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


# ------------------------------------------------------------------ the bounds
def residual_excess(S, g):
    """|| S g - e_m / g_m ||_inf over its bound 8 m eps ||S||_inf ||g||_inf: at most 1"""
    m = len(g)
    e = np.zeros(m)
    e[-1] = 1.0 / g[-1]
    bound = 8 * m * EPS * np.abs(S).sum(axis=1).max() * np.abs(g).max()
    return np.abs(S @ g - e).max() / bound


def forward_excess(S, g, other):
    """|| g - other ||_inf over cond_inf(S) 8 m eps ||g||_inf: at most 1"""
    m = len(g)
    cond = np.linalg.cond(S, np.inf)
    return np.abs(g - other).max() / (cond * 8 * m * EPS * np.abs(g).max())


def rows_within_bounds(A, row_ptr, cols, vals, other=None, skip=()):
    """the worst residual_excess (and, with `other`, forward_excess) over the rows of a G, the rows of `skip` left out"""
    A = sp.csr_matrix(A)
    worst_r = worst_f = 0.0
    for i in range(len(row_ptr) - 1):
        if i in skip:
            continue
        lo, hi = row_ptr[i], row_ptr[i + 1]
        S = block(A, cols[lo:hi])
        worst_r = max(worst_r, residual_excess(S, vals[lo:hi]))
        if other is not None:
            worst_f = max(worst_f, forward_excess(S, vals[lo:hi], other[lo:hi]))
    return worst_r, worst_f
