"""The block incomplete Cholesky preconditioner (bic.cpp, ehyb_bic.hip) restated in numpy / scipy, the bounds its tests hold the
factor and the apply to, and the exact cases of the kernel tests.  No tests here (test_bic_host.py, test_gpu_bic_kernels.py,
test_gpu_bic.py).

The restatement follows include/ehyb.h: blocks (every partition in runs of nearly equal length), the two local orders, the
IC(0) factor of every diagonal block with the shift rule -- in Python floats, every product and difference rounded, the sums in
the stated order --, levels, apply and pcg (the CG around it, the stopping test made every check_every iterations as the device
makes it).  Everything is in the permuted numbering: the matrix after ehyb_matrix_reorder, taken to be symmetric (only its lower
triangle is read).

The bounds.
  factor   l_ic is one sum of len + 1 terms (a_ic and the products) and a division, l_ii a sum and a root: two computations of
           it that may differ in whether a product is fused or rounded differ by at most (len + 2) u sum |terms| in the sum;
           carried through the division by l_cc, and for DINV = 1 / sqrt(d) through d^(-3/2) / 2 (and two roundings more, which the
           factor sum |terms| / d >= 1 covers).
  apply    x = T^-1 b by substitution satisfies (T + dT) x = b, |dT| <= gamma |T| (Higham, Accuracy and Stability, theorem 8.5), so
           |x - x^| <= gamma M(T)^-1 |T| M(T)^-1 |b| with the comparison matrix M(T) (|T^-1| <= M(T)^-1, lemma 8.8 there).  Two
           solves: the error of the first goes through the second.  gamma = (longest row + 2) u: the row's terms, the subtraction
           from b, the multiplication by the rounded 1 / l_ii."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

EPS = 2.0 ** -53              # the unit roundoff of fp64
MAX_BLOCK = 20480             # EHYB_BIC_MAX_BLOCK
SHIFTS = [2.0 ** k for k in range(-10, 11)]
FALLBACK = -1.0               # SHIFT of a block in its Jacobi form


# ------------------------------------------------------------------ the restatement
def blocks(part_boundary, block_rows=0):
    """-> block_ptr int32: every partition in ceil(rows / cap) runs of nearly equal length, the first runs one longer"""
    cap = min(block_rows, MAX_BLOCK) if block_rows > 0 else MAX_BLOCK
    ptr = [0]
    for lo, hi in zip(part_boundary[:-1], part_boundary[1:]):
        rows = int(hi - lo)
        if rows < 1:
            continue
        runs = -(-rows // cap)
        base, longer = divmod(rows, runs)
        for r in range(runs):
            ptr.append(ptr[-1] + base + (1 if r < longer else 0))
    return np.array(ptr, dtype=np.int32)


def colour_positions(low, r0, r1):
    """greedy colouring of the block's graph -> (pos (rows,): the position of every row, colours used).  low: tril(A, -1) in CSR
    form; both triangles count as neighbours"""
    rows = r1 - r0
    nbr = [[] for _ in range(rows)]
    for i in range(r0, r1):
        for j in low.indices[low.indptr[i]:low.indptr[i + 1]]:
            if j >= r0:
                nbr[i - r0].append(j - r0)
                nbr[j - r0].append(i - r0)
    colour = np.full(rows, -1)
    for p in range(rows):
        taken = {colour[q] for q in nbr[p] if colour[q] >= 0}
        c = 0
        while c in taken:
            c += 1
        colour[p] = c
    order = np.argsort(colour, kind="stable")          # by (colour, row)
    pos = np.empty(rows, dtype=np.int64)
    pos[order] = np.arange(rows)
    return pos, int(colour.max()) + 1 if rows else 0


def factor_block(rows_cols, rows_a, adiag, alpha):
    """IC(0) of A_b + alpha diag(A_b) -> (rows of l as dicts' values in column order, ldiag, per-entry and per-row sums of
    |terms|) or None at a pivot that is not a positive finite number"""
    n = len(adiag)
    L = [dict() for _ in range(n)]
    ldiag = [0.0] * n
    mag = [None] * n
    dmag = [0.0] * n
    for i in range(n):
        Li, cols, mags = L[i], rows_cols[i], []
        for c, a in zip(cols, rows_a[i]):
            s, m = a, abs(a)
            Lc = L[c]
            for k, lik in Li.items():               # (the columns of row i so far: all below c, rising)
                lck = Lc.get(k)
                if lck is not None:
                    t = lik * lck
                    s = s - t
                    m += abs(t)
            Li[c] = s / ldiag[c]
            mags.append(m)
        d = adiag[i] + alpha * adiag[i]
        m = abs(d)
        for lik in Li.values():
            t = lik * lik
            d = d - t
            m += t
        if not (d > 0 and np.isfinite(d)):
            return None
        ldiag[i] = float(np.sqrt(d))
        mag[i], dmag[i] = mags, (m, d)
    return L, ldiag, mag, dmag


def build(A, part_boundary, block_rows=0, order="stored"):
    """the object of ehyb_bic_create_host -> a dict of its arrays, and "vals_bound", "dinv_bound" (what another computation of the
    same factor may differ by), "colours" (per block; stored order: None)"""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    low = sp.tril(A, -1).tocsr()
    low.sort_indices()
    diag = A.diagonal()
    stored_diag = np.zeros(n, dtype=bool)
    for i in range(n):
        stored_diag[i] = i in A.indices[A.indptr[i]:A.indptr[i + 1]]
    if not (stored_diag & (diag > 0) & np.isfinite(diag)).all():
        raise ValueError("not positive definite")
    block_ptr = blocks(part_boundary, block_rows)
    nb = len(block_ptr) - 1
    perm = np.empty(n, dtype=np.int32)
    row_ptr, cols, vals, vbound = [0], [], [], []
    dinv, dbound = np.empty(n), np.empty(n)
    shift, colours = np.zeros(nb), []
    shifted = fallback = 0
    for b in range(nb):
        r0, r1 = int(block_ptr[b]), int(block_ptr[b + 1])
        rows = r1 - r0
        if order == "stored":
            pos, ncol = np.arange(rows), None
        else:
            pos, ncol = colour_positions(low, r0, r1)
        colours.append(ncol)
        perm[r0 + pos] = np.arange(r0, r1)
        rc = [[] for _ in range(rows)]
        for i in range(r0, r1):
            for e in range(low.indptr[i], low.indptr[i + 1]):
                j = low.indices[e]
                if j >= r0:
                    pi, pj = pos[i - r0], pos[j - r0]
                    rc[max(pi, pj)].append((min(pi, pj), low.data[e]))
        rows_cols, rows_a = [], []
        for p in range(rows):
            rc[p].sort(key=lambda t: t[0])
            rows_cols.append([int(t[0]) for t in rc[p]])
            rows_a.append([float(t[1]) for t in rc[p]])
        adiag = [0.0] * rows
        for i in range(r0, r1):
            adiag[pos[i - r0]] = float(diag[i])
        out = factor_block(rows_cols, rows_a, adiag, 0.0)
        alpha = 0.0
        if out is None:
            for alpha in SHIFTS:
                out = factor_block(rows_cols, rows_a, adiag, alpha)
                if out is not None:
                    shifted += 1
                    break
        if out is None:
            fallback += 1
            alpha = FALLBACK
            L = [dict((c, 0.0) for c in rows_cols[p]) for p in range(rows)]
            ldiag = [float(np.sqrt(a)) for a in adiag]
            mag = [[0.0] * len(rows_cols[p]) for p in range(rows)]
            dmag = [(a, a) for a in adiag]
        else:
            L, ldiag, mag, dmag = out
        shift[b] = alpha
        for p in range(rows):
            ln = len(rows_cols[p])
            cols.extend(rows_cols[p])
            vals.extend(L[p][c] for c in rows_cols[p])
            vbound.extend((ln + 2) * EPS * m / ldiag[c] for m, c in zip(mag[p], rows_cols[p]))
            row_ptr.append(len(cols))
            dinv[r0 + p] = 1.0 / ldiag[p]
            m, d = dmag[p]
            dbound[r0 + p] = (ln + 2) * EPS * (m / d) * dinv[r0 + p]
    f = dict(n=n, block_ptr=block_ptr, perm=perm, row_ptr=np.array(row_ptr, dtype=np.int64), cols=np.array(cols, dtype=np.int32),
             vals=np.array(vals, dtype=np.float64), dinv=dinv, shift=shift, vals_bound=np.array(vbound, dtype=np.float64), dinv_bound=dbound,
             colours=colours)
    f["level_f"], f["level_b"], most = levels(block_ptr, f["row_ptr"], f["cols"])
    f["counts"] = np.array([nb, shifted, fallback, most], dtype=np.int64)
    return f


def levels(block_ptr, row_ptr, cols):
    """-> (LEVEL_F, LEVEL_B, the most levels of any block in either direction)"""
    n = len(row_ptr) - 1
    lf, lb = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for b in range(len(block_ptr) - 1):
        r0, r1 = int(block_ptr[b]), int(block_ptr[b + 1])
        for p in range(r0, r1):
            c = cols[row_ptr[p]:row_ptr[p + 1]]
            lf[p] = lf[r0 + c].max() + 1 if len(c) else 0
        for q in range(r1 - 1, r0 - 1, -1):
            c = cols[row_ptr[q]:row_ptr[q + 1]]
            if len(c):
                lb[r0 + c] = np.maximum(lb[r0 + c], lb[q] + 1)
    return lf, lb, int(max(lf.max(), lb.max())) + 1 if n else 0


def factor_matrix(f, vals=None, dinv=None):
    """L with its diagonal, block diagonal, in POSITION order (sparse CSC, sorted)"""
    n = len(f["row_ptr"]) - 1
    vals = f["vals"] if vals is None else vals
    dinv = f["dinv"] if dinv is None else dinv
    first = np.repeat(f["block_ptr"][:-1], np.diff(f["block_ptr"]))          # the block's first position, per position
    rows = np.repeat(np.arange(n), np.diff(f["row_ptr"]))
    strict = sp.csr_matrix((vals, (rows, first[rows] + f["cols"])), shape=(n, n))
    return (strict + sp.diags(1.0 / dinv)).tocsc()


class Solver:
    """z = P^T (L L^T)^-1 P r with compiled triangular solves (SuperLU on L in its natural order: nothing to eliminate)"""

    def __init__(self, f, vals=None, dinv=None):
        self.perm = f["perm"]
        self.L = factor_matrix(f, vals, dinv)
        self.lu = spla.splu(self.L, permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=False))
        assert (self.lu.perm_r == np.arange(self.L.shape[0])).all() and (self.lu.perm_c == np.arange(self.L.shape[0])).all()

    def __call__(self, r):
        z = np.empty_like(r)
        z[self.perm] = self.lu.solve(self.lu.solve(r[self.perm]), trans="T")
        return z


def apply(f, r, vals=None, dinv=None):
    return Solver(f, vals, dinv)(r)


def apply_longdouble(f, r, vals=None, dinv=None):
    """the apply by substitution in extended precision, multiplying by 1 / dinv's exact reciprocal: the reference of the bound"""
    vals = (f["vals"] if vals is None else vals).astype(np.longdouble)
    dinv = f["dinv"] if dinv is None else dinv
    ldiag = np.longdouble(1.0) / dinv.astype(np.longdouble)
    n = len(dinv)
    first = np.repeat(f["block_ptr"][:-1], np.diff(f["block_ptr"]))
    rp, cols = f["row_ptr"], f["cols"]
    x = r[f["perm"]].astype(np.longdouble)
    for p in range(n):
        lo, hi = rp[p], rp[p + 1]
        if hi > lo:
            x[p] -= vals[lo:hi] @ x[first[p] + cols[lo:hi]]
        x[p] /= ldiag[p]
    for q in range(n - 1, -1, -1):
        lo, hi = rp[q], rp[q + 1]
        x[q] /= ldiag[q]
        if hi > lo:
            x[first[q] + cols[lo:hi]] -= vals[lo:hi] * x[q]
    z = np.empty(n, dtype=np.longdouble)
    z[f["perm"]] = x
    return z


def apply_bound(f, r, vals=None, dinv=None):
    """componentwise: what a computed apply may be off by (see the head of the file), in the permuted numbering"""
    L = factor_matrix(f, vals, dinv)
    absL = abs(L).tocsc()
    M = (2 * sp.diags(absL.diagonal()) - absL).tocsc()             # the comparison matrix: |l_ii| on, -|l_ij| off the diagonal
    lu = spla.splu(M, permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=False))
    gamma = (int(np.diff(f["row_ptr"]).max(initial=0)) + 2) * EPS
    # the rows of L^T are the columns of L: the longest of either
    gamma = max(gamma, (int(np.bincount(absL.indices, minlength=1).max()) + 2) * EPS)
    y = lu.solve(np.abs(r[f["perm"]]))                             # |y^| <= M^-1 |b|
    e1 = gamma * lu.solve(absL @ y)                                # the forward solve's error
    w = lu.solve(y, trans="T")                                     # |z| <= M^-T M^-1 |b|
    e2 = lu.solve(e1, trans="T") + gamma * lu.solve(absL.T @ w, trans="T")
    out = np.empty_like(e2)
    out[f["perm"]] = e2 * (1 + 1e-6)                               # (the bound's own arithmetic and its second-order terms)
    return out


def pcg(A, b, solve, max_iter=1000, rtol=1e-10, x0=None, check_every=1):
    """The solve of ehyb_pcg_bic, iteration for iteration -> (x, iterations); solve: a Solver"""
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = b.copy() if x0 is None else b - A @ x0
    z = solve(r)
    p, rz, bb = z.copy(), r @ z, (b @ b) or 1.0
    it = 0
    while it < max_iter and (it % check_every or np.sqrt((r @ r) / bb) > rtol):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = solve(r)
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
        it += 1
    return x, it


def from_library(bic):
    """the arrays of a library object (E.Bic) as build returns them"""
    return {name: bic.array(name) for name in ("block_ptr", "perm", "row_ptr", "cols", "vals", "dinv", "level_f", "level_b", "shift", "counts")}


# ------------------------------------------------------------------ a matrix IC(0) breaks down on
def kershaw():
    """The 4 x 4 SPD matrix of Kershaw (1978): not an H-matrix, and IC(0) meets a negative pivot in its last row."""
    return np.array([[3.0, -2.0, 0.0, 2.0], [-2.0, 3.0, -2.0, 0.0], [0.0, -2.0, 3.0, -2.0], [2.0, 0.0, -2.0, 3.0]])


def five():
    """A 5 x 5 SPD matrix, not an H-matrix, whose graph has a triangle: IC(0) breaks down on it in the stored order and in the
    coloured one, as it stands and as the library's reordering leaves it (found by a search over small integer matrices with
    this restatement; the tests verify both again)."""
    return np.array([[3.0, -2, -1, 0, -1], [-2, 3, 2, -1, 0], [-1, 2, 3, 0, -2], [0, -1, 0, 3, 0], [-1, 0, -2, 0, 3]])


# ------------------------------------------------------------------ exact cases for the kernels
# dinv are powers of two, the entries of L and r small integers: every term of every row's sum is a multiple of one power of two,
# and exact_apply asserts that the magnitudes of a row's terms add up below 2^53 of them -- so every partial sum, in any order and
# with or without fused products, is exact and the exact solve is the only right answer.
SCALE = 200                   # the integers below stand for multiples of 2^-SCALE


def _solve_exact(block_ptr, row_ptr, cols, vals, dexp, x):
    """in place: x (Python ints, units of 2^-SCALE) through the forward and the backward solve; dexp: log2 of dinv"""
    n = len(dexp)
    first = np.repeat(block_ptr[:-1], np.diff(block_ptr)).tolist()
    rp, cl, vl = row_ptr.tolist(), cols.tolist(), [int(v) for v in vals]

    def scale(v, k):
        if k >= 0:
            return v << k
        assert v % (1 << -k) == 0, "the case leaves the exact range (denominator)"
        return v >> -k

    def check(terms):
        both = 0
        for t in terms:
            both |= abs(t)
        if both:
            unit = both & -both
            assert sum(abs(t) for t in terms) // unit < 2 ** 53, "the case leaves the exact range (width)"

    for p in range(n):
        lo, hi = rp[p], rp[p + 1]
        if hi > lo:
            terms = [x[p]] + [vl[e] * x[first[p] + cl[e]] for e in range(lo, hi)]
            check(terms)
            x[p] = terms[0] - sum(terms[1:])
        x[p] = scale(x[p], dexp[p])
    # backward, as the device does it: row p of L^T gathers the l_qp x_q of the q > p
    tcols = [[] for _ in range(n)]
    for q in range(n):
        for e in range(rp[q], rp[q + 1]):
            tcols[first[q] + cl[e]].append((q, vl[e]))
    for p in range(n - 1, -1, -1):
        if tcols[p]:
            terms = [x[p]] + [v * x[q] for q, v in tcols[p]]
            check(terms)
            x[p] = terms[0] - sum(terms[1:])
        x[p] = scale(x[p], dexp[p])
    return x


def exact_apply(block_ptr, row_ptr, cols, vals, dinv, R):
    """Z = (L L^T)^-1 R exactly, R (k, n) or (n,) of integers -> float64 of the same shape"""
    mant, ex = np.frexp(dinv)
    assert (mant == 0.5).all(), "dinv are powers of two"
    dexp = (ex - 1).tolist()
    R2 = np.atleast_2d(R)
    out = np.empty(R2.shape)
    for c in range(R2.shape[0]):
        assert (R2[c] == np.round(R2[c])).all()
        x = [int(v) << SCALE for v in R2[c]]
        x = _solve_exact(block_ptr, row_ptr, cols, vals, dexp, x)
        for i, v in enumerate(x):
            out[c, i] = float(v) * 2.0 ** -SCALE if abs(v) < 2 ** 1000 else np.nan
            assert int(out[c, i] * 2.0 ** SCALE) == v
    return out.reshape(np.shape(R))


def staged_factor(rng, lengths, stages=5, per_row=2):
    """A block-diagonal strictly lower L of the given block lengths with at most `stages` levels either way: row p takes up to
    per_row columns among the earlier positions q of its block with q % stages < p % stages.  Entries in +-{1, 2}, dinv in {1/2, 1,
    2}.  -> (block_ptr, row_ptr, cols, vals, dinv)"""
    block_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    row_ptr, cols, vals = [0], [], []
    for rows in lengths:
        for p in range(rows):
            cand = [q for q in range(max(0, p - 40), p) if q % stages < p % stages]
            if cand:
                take = sorted(set(rng.choice(cand, size=min(per_row, len(cand)), replace=False).tolist()))
                cols.extend(take)
                vals.extend(rng.choice([-2, -1, 1, 2], size=len(take)).tolist())
            row_ptr.append(len(cols))
    n = int(block_ptr[-1])
    dinv = 2.0 ** rng.integers(-1, 2, n)
    return block_ptr, np.array(row_ptr, dtype=np.int64), np.array(cols, dtype=np.int32), np.array(vals, dtype=np.float64), dinv


def small_ints(rng, shape, bits=4):
    return rng.integers(-(1 << bits), (1 << bits) + 1, shape).astype(np.float64)
