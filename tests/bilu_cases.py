"""The block ILU(0) preconditioner (bilu.cpp, and ehyb_bic.hip's apply on its streams) restated in numpy / scipy, the
right-preconditioned GMRES and BiCGSTAB around it, and the exact cases of the kernel tests.  No tests here (test_bilu_host.py,
test_gpu_bilu_kernels.py, test_gpu_bilu.py).

The restatement follows include/ehyb.h: the blocks and orders of ehyb_bic (bic_cases.py; the colouring on the pattern of
A_b + A_b^T), A_b with duplicates summed in stored order and the diagonal always in the pattern, row-wise IKJ ILU(0) -- in Python
floats, every product and difference rounded, k rising and j rising --, the pivot rule |u_ii| > 2^-26 s_i with s_i = sum |a_ij|,
the ladder alpha = 2^-10, 2^-8 .. 2^10 on A_b + alpha diag(s), the Jacobi form where no alpha works, and the two level arrays.
Everything is in the permuted numbering and reads the matrix as stored (raw CSR arrays: unsorted rows, duplicates, explicit
zeros), never a canonical form of it.

num: the arithmetic of the factorisation -- float, or np.longdouble for the reference the defect of (L U - A_b) is measured in."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import bic_cases as bc

EPS = bc.EPS
MAX_BLOCK = bc.MAX_BLOCK
SHIFTS = [2.0 ** k for k in range(-10, 11, 2)]
FALLBACK = -1.0
PIVOT_FLOOR = 2.0 ** -26
NAMES = ("block_ptr", "perm", "l_row_ptr", "l_cols", "l_vals", "u_row_ptr", "u_cols", "u_vals", "u_dinv", "level_f", "level_b", "shift", "counts")


# ------------------------------------------------------------------ the restatement
def block_rows_of(indptr, indices, data, r0, r1, pos):
    """A_b in local order -> per position p the merged row [(col, value)] with columns rising, duplicates summed in stored
    order, and the diagonal present (0.0 where none is stored)"""
    rows = [None] * (r1 - r0)
    for i in range(r0, r1):
        merged = {}
        for e in range(indptr[i], indptr[i + 1]):
            j = int(indices[e])
            if r0 <= j < r1:
                c = int(pos[j - r0])
                merged[c] = merged[c] + float(data[e]) if c in merged else float(data[e])
        p = int(pos[i - r0])
        merged.setdefault(p, 0.0)
        rows[p] = sorted(merged.items())
    return rows


def factor_block(rows, s, alpha, num=float):
    """IKJ ILU(0) of A_b + alpha diag(s) on the pattern -> list of dicts {col: value} holding l_ik (k < i), u_ii and u_ij (j > i),
    or None at a pivot the rule refuses"""
    W = []
    for i, row in enumerate(rows):
        w = {c: num(v) for c, v in row}
        if alpha != 0:
            w[i] = num(dict(row)[i]) + num(alpha) * num(s[i])
        for k, _ in row:
            if k >= i:
                break
            lik = w[k] / W[k][k]                    # (an accepted pivot is never zero: |u_kk| > 2^-26 s_k >= 0)
            w[k] = lik
            for j, ukj in W[k].items():
                if j > k and j in w:
                    with np.errstate(all="ignore"):
                        w[j] = w[j] - lik * ukj
        u = float(w[i])
        if not np.isfinite(u) or not abs(u) > PIVOT_FLOOR * s[i]:
            return None
        W.append(w)
    return W


def build(A, part_boundary, block_rows=0, order="stored", num=float, shifts=None):
    """the object of ehyb_bilu_create_host -> a dict of its arrays (NAMES) and "colours".  A: scipy CSR, read as stored.  shifts:
    the alpha of every block given (for the longdouble reference: the decisions of the float64 factor), FALLBACK included."""
    indptr, indices, data = A.indptr, A.indices, A.data
    n = A.shape[0]
    S = sp.csr_matrix((np.ones(len(indices)), indices.copy(), indptr.copy()), shape=A.shape)
    S = (S + S.T).tocsr()
    low = sp.tril(S, -1).tocsr()
    low.sort_indices()
    block_ptr = bc.blocks(part_boundary, block_rows)
    nb = len(block_ptr) - 1
    perm = np.empty(n, dtype=np.int32)
    lrp, lc, lv, urp, uc, uv = [0], [], [], [0], [], []
    udinv = np.empty(n, dtype=np.longdouble if num is not float else np.float64)
    shift, colours = np.zeros(nb), []
    shifted = fallback = 0
    for b in range(nb):
        r0, r1 = int(block_ptr[b]), int(block_ptr[b + 1])
        rows_n = r1 - r0
        if order == "stored":
            pos, ncol = np.arange(rows_n), None
        else:
            pos, ncol = bc.colour_positions(low, r0, r1)
        colours.append(ncol)
        perm[r0 + pos] = np.arange(r0, r1)
        rows = block_rows_of(indptr, indices, data, r0, r1, pos)
        s = []
        for row in rows:
            t = 0.0
            for _, v in row:
                t = t + abs(v)
            s.append(t)
        if shifts is not None:
            alpha = float(shifts[b])
            W = None if alpha == FALLBACK else factor_block(rows, s, alpha, num)
            assert alpha == FALLBACK or W is not None
        else:
            W, alpha = factor_block(rows, s, 0.0, num), 0.0
            if W is None:
                for alpha in SHIFTS:
                    W = factor_block(rows, s, alpha, num)
                    if W is not None:
                        break
        if W is None:
            alpha = FALLBACK
            fallback += 1
            for p, row in enumerate(rows):
                a = dict(row)[p]
                udinv[r0 + p] = 1.0 / a if a != 0 and np.isfinite(a) else 1.0
                lrp.append(len(lc))
                urp.append(len(uc))
        else:
            shifted += alpha != 0
            for p, w in enumerate(W):
                for c in sorted(w):
                    if c < p:
                        lc.append(c), lv.append(w[c])
                    elif c > p:
                        uc.append(c), uv.append(w[c])
                udinv[r0 + p] = num(1.0) / w[p]
                lrp.append(len(lc))
                urp.append(len(uc))
        shift[b] = alpha
    vt = np.longdouble if num is not float else np.float64
    f = dict(n=n, block_ptr=block_ptr, perm=perm, l_row_ptr=np.array(lrp, dtype=np.int64), l_cols=np.array(lc, dtype=np.int32),
             l_vals=np.array(lv, dtype=vt), u_row_ptr=np.array(urp, dtype=np.int64), u_cols=np.array(uc, dtype=np.int32),
             u_vals=np.array(uv, dtype=vt), u_dinv=udinv, shift=shift, colours=colours)
    f["level_f"], f["level_b"], most = levels(block_ptr, f["l_row_ptr"], f["l_cols"], f["u_row_ptr"], f["u_cols"])
    f["counts"] = np.array([nb, shifted, fallback, most], dtype=np.int64)
    return f


def levels(block_ptr, lrp, lc, urp, uc):
    """-> (LEVEL_F from L's rows, LEVEL_B from U's rows, the most levels of any block in either direction)"""
    n = len(lrp) - 1
    lf, lb = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for b in range(len(block_ptr) - 1):
        r0, r1 = int(block_ptr[b]), int(block_ptr[b + 1])
        for p in range(r0, r1):
            c = lc[lrp[p]:lrp[p + 1]]
            lf[p] = lf[r0 + c].max() + 1 if len(c) else 0
        for p in range(r1 - 1, r0 - 1, -1):
            c = uc[urp[p]:urp[p + 1]]
            lb[p] = lb[r0 + c].max() + 1 if len(c) else 0
    return lf, lb, int(max(lf.max(), lb.max())) + 1 if n else 0


def from_library(f):
    """the arrays of a library object (E.Bilu) as build returns them"""
    return {name: f.array(name) for name in NAMES}


def triangles(f):
    """(L with its unit diagonal, U with its diagonal 1 / u_dinv), block diagonal, in POSITION order (sparse CSC)"""
    n = len(f["u_dinv"])
    first = np.repeat(f["block_ptr"][:-1], np.diff(f["block_ptr"]))
    out = []
    for rp, cols, vals, diag in ((f["l_row_ptr"], f["l_cols"], f["l_vals"], np.ones(n)), (f["u_row_ptr"], f["u_cols"], f["u_vals"], 1.0 / f["u_dinv"])):
        rows = np.repeat(np.arange(n), np.diff(rp))
        strict = sp.csr_matrix((np.asarray(vals, dtype=np.float64), (rows, first[rows] + cols)), shape=(n, n))
        out.append((strict + sp.diags(np.asarray(diag, dtype=np.float64))).tocsc())
    return out


def _natural_lu(T):
    lu = spla.splu(T, permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=False))
    assert (lu.perm_r == np.arange(T.shape[0])).all() and (lu.perm_c == np.arange(T.shape[0])).all()
    return lu


class Solver:
    """z = P^T (L U)^-1 P r with compiled triangular solves (SuperLU on a triangle in its natural order: nothing to eliminate)"""

    def __init__(self, f):
        self.perm = f["perm"]
        L, U = triangles(f)
        self.l, self.u = _natural_lu(L), _natural_lu(U)

    def __call__(self, r):
        z = np.empty_like(r)
        z[self.perm] = self.u.solve(self.l.solve(r[self.perm]))
        return z


def apply_longdouble(f, r):
    """the apply by substitution in extended precision, dividing by the exact reciprocal of u_dinv: the reference of the bound"""
    n = len(f["u_dinv"])
    lv, uv = f["l_vals"].astype(np.longdouble), f["u_vals"].astype(np.longdouble)
    udiag = np.longdouble(1.0) / f["u_dinv"].astype(np.longdouble)
    first = np.repeat(f["block_ptr"][:-1], np.diff(f["block_ptr"]))
    x = r[f["perm"]].astype(np.longdouble)
    for p in range(n):
        lo, hi = f["l_row_ptr"][p], f["l_row_ptr"][p + 1]
        if hi > lo:
            x[p] -= lv[lo:hi] @ x[first[p] + f["l_cols"][lo:hi]]
    for p in range(n - 1, -1, -1):
        lo, hi = f["u_row_ptr"][p], f["u_row_ptr"][p + 1]
        if hi > lo:
            x[p] -= uv[lo:hi] @ x[first[p] + f["u_cols"][lo:hi]]
        x[p] /= udiag[p]
    z = np.empty(n, dtype=np.longdouble)
    z[f["perm"]] = x
    return z


def apply_bound(f, r):
    """componentwise: what a computed apply may be off by -- bic_cases.apply_bound (Higham, theorem 8.5 and lemma 8.8) with two
    different triangles: the forward solve's error goes through the backward one.  gamma = (longest row + 2) u."""
    L, U = triangles(f)
    absL, absU = abs(L).tocsc(), abs(U).tocsc()
    ML = (2 * sp.diags(absL.diagonal()) - absL).tocsc()
    MU = (2 * sp.diags(absU.diagonal()) - absU).tocsc()
    lul, luu = _natural_lu(ML), _natural_lu(MU)
    gamma = (int(max(np.diff(f["l_row_ptr"]).max(initial=0), np.diff(f["u_row_ptr"]).max(initial=0))) + 2) * EPS
    y = lul.solve(np.abs(r[f["perm"]]))
    e1 = gamma * lul.solve(absL @ y)
    w = luu.solve(y)
    e2 = luu.solve(e1) + gamma * luu.solve(absU @ w)
    out = np.empty_like(e2)
    out[f["perm"]] = e2 * (1 + 1e-6)
    return out


def defect(A, f):
    """max over the pattern of |(L U - A_b - alpha diag(s))_ij| / s_i, the products and sums in np.longdouble; fallback blocks are
    skipped.  -> (the figure, entries looked at)"""
    indptr, indices, data = A.indptr, A.indices, A.data
    worst, seen = 0.0, 0
    ld = np.longdouble
    for b in range(len(f["block_ptr"]) - 1):
        r0, r1 = int(f["block_ptr"][b]), int(f["block_ptr"][b + 1])
        alpha = float(f["shift"][b])
        if alpha == FALLBACK:
            continue
        pos = np.empty(r1 - r0, dtype=np.int64)
        pos[f["perm"][r0:r1] - r0] = np.arange(r1 - r0)
        rows = block_rows_of(indptr, indices, data, r0, r1, pos)
        Lr, Ur = [], []
        for p in range(r1 - r0):
            lo, hi = f["l_row_ptr"][r0 + p], f["l_row_ptr"][r0 + p + 1]
            Lr.append({int(c): ld(v) for c, v in zip(f["l_cols"][lo:hi], f["l_vals"][lo:hi])})
            Lr[p][p] = ld(1.0)
            lo, hi = f["u_row_ptr"][r0 + p], f["u_row_ptr"][r0 + p + 1]
            Ur.append({int(c): ld(v) for c, v in zip(f["u_cols"][lo:hi], f["u_vals"][lo:hi])})
            Ur[p][p] = ld(1.0) / ld(f["u_dinv"][r0 + p])
        for p, row in enumerate(rows):
            s = 0.0
            for _, v in row:
                s = s + abs(v)
            for c, a in row:
                want = ld(a) + (ld(alpha) * ld(s) if c == p and alpha != 0 else ld(0))
                got = ld(0)
                for k, lik in Lr[p].items():
                    ukc = Ur[k].get(c)
                    if ukc is not None:
                        got += lik * ukc
                if s > 0:
                    worst = max(worst, float(abs(got - want) / ld(s)))
                seen += 1
    return worst, seen


# ------------------------------------------------------------------ the solvers, step for step (include/ehyb.h)
def gmres(A, b, solve, x0=None, restart=30, passes=2, max_iter=1000, rtol=1e-10):
    """ehyb_gmres_bilu's rules: ehyb_gmres's (test_gpu_gmres.cpu_gmres) with z = solve(v_j) as the multiply's input and
    x += solve(sum y_i v_i) at a cycle's end.  -> (x, steps, relative residual, status)"""
    n = len(b)
    x = np.zeros(n) if x0 is None else x0.copy()
    bb = b @ b
    bb = 1.0 if bb == 0 else bb
    thr = rtol * rtol
    it = 0
    with np.errstate(all="ignore"):
        while True:
            r = b - A @ x
            rho = r @ r
            if not (np.isfinite(bb) and np.isfinite(rho)):
                return x, it, np.sqrt(rho / bb), "breakdown"
            if rho <= thr * bb:
                return x, it, np.sqrt(rho / bb), "converged"
            beta = np.sqrt(rho)
            V = [r / beta]
            gt = [beta]
            g, cs, sn = [], [], []
            R = np.zeros((restart, restart))
            status = None
            for j in range(min(restart, max_iter - it)):
                w = A @ solve(V[j])
                h = np.zeros(j + 2)
                Vm = np.array(V)
                for _ in range(passes):
                    c = Vm @ w
                    w = w - c @ Vm
                    h[:j + 1] += c
                h[j + 1] = hn = np.sqrt(w @ w)
                if not np.isfinite(h).all():
                    status = "breakdown"
                    break
                for i in range(j):
                    t = cs[i] * h[i] + sn[i] * h[i + 1]
                    h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1]
                    h[i] = t
                gamma = np.hypot(h[j], h[j + 1])
                if gamma == 0 or not np.isfinite(gamma):
                    status = "breakdown"
                    break
                cs.append(h[j] / gamma)
                sn.append(h[j + 1] / gamma)
                R[:j, j] = h[:j]
                R[j, j] = gamma
                gt.append(-sn[j] * gt[j])
                g.append(cs[j] * gt[j])
                it += 1
                rho = gt[j + 1] ** 2
                if rho <= thr * bb:
                    status = "converged"
                    break
                if hn == 0:
                    status = "breakdown"
                    break
                V.append(w / hn)
            J = len(g)
            if J:
                y = sla.solve_triangular(R[:J, :J], np.array(g))
                x = x + solve(y @ np.array(V[:J]))
            if status is not None:
                return x, it, np.sqrt(rho / bb), status
            if it >= max_iter:
                return x, it, np.sqrt(rho / bb), "max_iter"


def bicgstab(A, b, solve, x0=None, max_iter=1000, rtol=1e-10):
    """ehyb_bicgstab_bilu: the textbook right-preconditioned recurrences with ehyb_bicgstab's stop and breakdown rules.
    -> (x, iterations, relative residual, status)"""
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = b - A @ x
    rh = r.copy()
    p = r.copy()
    rho, rr, bb = rh @ r, r @ r, b @ b
    bb = bb if bb > 0 else 1.0
    thr = rtol * rtol
    rel = lambda: np.sqrt(rr / bb)                      # noqa: E731
    if not (np.isfinite(rr) and np.isfinite(bb)):
        return x, 0, rel(), "breakdown"
    if rr <= thr * bb:
        return x, 0, rel(), "converged"
    it = 0
    while it < max_iter:
        ph = solve(p)
        v = A @ ph
        rv = rh @ v
        with np.errstate(all="ignore"):
            alpha = rho / rv
        if not np.isfinite(rho) or rv == 0 or not np.isfinite(rv) or not np.isfinite(alpha):
            return x, it, rel(), "breakdown"
        s = r - alpha * v
        ss = s @ s
        if ss <= thr * bb:                              # half step
            x = x + alpha * ph
            rr = ss
            return x, it + 1, rel(), "converged"
        sh = solve(s)
        t = A @ sh
        ts, tt = t @ s, t @ t
        with np.errstate(all="ignore"):
            omega = ts / tt
        if tt == 0 or not np.isfinite(tt) or not np.isfinite(omega):
            return x, it, rel(), "breakdown"
        x = x + alpha * ph + omega * sh
        r = s - omega * t
        rho_new, rr = rh @ r, r @ r
        it += 1
        if rr <= thr * bb:
            return x, it, rel(), "converged"
        with np.errstate(all="ignore"):
            beta = (rho_new / rho) * (alpha / omega)
        if rho == 0 or not np.isfinite(rho) or omega == 0 or not np.isfinite(rho_new) or not np.isfinite(beta):
            return x, it, rel(), "breakdown"
        p = r + beta * (p - omega * v)
        rho = rho_new
    return x, it, rel(), "max_iter"


def jacobi(A):
    d = 1.0 / A.diagonal()
    return lambda v: d * v


# ------------------------------------------------------------------ exact cases for the kernels
# L and U hold dyadic values, 1 / u_ii are powers of two, r small integers: every term of every row's sum is a multiple of one
# power of two, and _ex asserts that the magnitudes of a row's terms add up below 2^53 of them -- so every partial sum, in any
# order and with or without fused products, is exact and the exact solve is the only right answer.
SCALE = 400                   # the integers below stand for multiples of 2^-SCALE


def _ex(terms):
    both = 0
    for t in terms:
        both |= abs(t)
    if both:
        unit = both & -both
        assert sum(abs(t) for t in terms) // unit < 2 ** 53, "the case leaves the exact range (width)"


def _times(v, x):
    """the dyadic float v times the scaled integer x, exactly"""
    num, den = float(v).as_integer_ratio()
    q, rem = divmod(num * x, den)
    assert rem == 0, "the case leaves the exact range (denominator)"
    return q


def exact_apply(block_ptr, lrp, lc, lv, urp, uc, uv, udinv, R):
    """Z = (L U)^-1 R exactly, R (k, n) or (n,) of integers -> float64 of the same shape"""
    mant, _ = np.frexp(udinv)
    assert (np.abs(mant) == 0.5).all(), "1 / u_ii are powers of two"
    n = len(udinv)
    first = np.repeat(block_ptr[:-1], np.diff(block_ptr)).tolist()
    lrp, lc, lv, urp, uc, uv = (np.asarray(a).tolist() for a in (lrp, lc, lv, urp, uc, uv))
    R2 = np.atleast_2d(R)
    out = np.empty(R2.shape)
    for col in range(R2.shape[0]):
        assert (R2[col] == np.round(R2[col])).all()
        x = [int(v) << SCALE for v in R2[col]]
        for p in range(n):
            if lrp[p + 1] > lrp[p]:
                terms = [x[p]] + [_times(lv[e], x[first[p] + lc[e]]) for e in range(lrp[p], lrp[p + 1])]
                _ex(terms)
                x[p] = terms[0] - sum(terms[1:])
        for p in range(n - 1, -1, -1):
            if urp[p + 1] > urp[p]:
                terms = [x[p]] + [_times(uv[e], x[first[p] + uc[e]]) for e in range(urp[p], urp[p + 1])]
                _ex(terms)
                x[p] = terms[0] - sum(terms[1:])
            x[p] = _times(udinv[p], x[p])
        for i, v in enumerate(x):
            out[col, i] = float(v) * 2.0 ** -SCALE
            assert int(out[col, i] * 2.0 ** SCALE) == v, "the answer is no double"
    return out.reshape(np.shape(R))


VALUES = [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]


def staged_pair(rng, lengths, stages=5, per_row_l=2, per_row_u=2, values=VALUES, reach=40):
    """Block-diagonal strict triangles of the given block lengths with at most `stages` levels either way, chosen independently:
    row p of L takes up to per_row_l columns among the earlier positions q of its block with q % stages < p % stages, row p of U
    up to per_row_u among the later ones with q % stages > p % stages (both within `reach`).  Dyadic entries, 1 / u_ii in
    {-1/2, 1/2, 1, 2}.  -> (block_ptr, l_row_ptr, l_cols, l_vals, u_row_ptr, u_cols, u_vals, u_dinv)"""
    block_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    out = []
    for lower, per_row in ((True, per_row_l), (False, per_row_u)):
        rp, cols, vals = [0], [], []
        for rows in lengths:
            for p in range(rows):
                if lower:
                    cand = [q for q in range(max(0, p - reach), p) if q % stages < p % stages]
                else:
                    cand = [q for q in range(p + 1, min(rows, p + 1 + reach)) if q % stages > p % stages]
                if cand and per_row:
                    take = sorted(set(rng.choice(cand, size=min(per_row, len(cand)), replace=False).tolist()))
                    cols.extend(take)
                    vals.extend(rng.choice(values, size=len(take)).tolist())
                rp.append(len(cols))
        out += [np.array(rp, dtype=np.int64), np.array(cols, dtype=np.int32), np.array(vals, dtype=np.float64)]
    n = int(block_ptr[-1])
    udinv = rng.choice([-0.5, 0.5, 1.0, 2.0], size=n)
    return (block_ptr, *out, udinv)


def empty_triangle(n):
    return np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)


def transpose_strict(block_ptr, rp, cols, vals):
    """the strict lower triangle (CSR, block-local columns) -> its transpose, a strict upper one of the same form"""
    n = len(rp) - 1
    first = np.repeat(block_ptr[:-1], np.diff(block_ptr))
    rows = np.repeat(np.arange(n), np.diff(rp))
    T = sp.csr_matrix((vals, (first[rows] + cols, rows)), shape=(n, n))
    T.sort_indices()
    trow = np.repeat(np.arange(n), np.diff(T.indptr))
    return T.indptr.astype(np.int64), (T.indices - first[trow]).astype(np.int32), T.data.copy()


small_ints = bc.small_ints
