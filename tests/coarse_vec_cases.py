"""The coarse space from near-null-space vectors (ehyb_coarse_create_host_vecs; coarse.cpp, ehyb_coarse.hip) restated in numpy,
a 3-D spring network whose null space is the six rigid-body modes, and exact cases for the two weighted kernels in the style of
coarse_cases.py.  No tests here (test_coarse_vec_host.py, test_gpu_coarse_vec_kernels.py, test_gpu_coarse_vec.py).

The restatement follows include/ehyb.h: build_P (per aggregate the columns of B in turn, modified Gram-Schmidt in two passes,
kept iff norm0 > 0 and at least 2^-20 of the column is left; the unknowns aggregate-major), prolongation (P as a sparse
matrix), coarse_matrix (E = P^T A P), apply (z = D^-1 r + P E^-1 P^T r) and pcg, which runs the loop of coarse_cases.pcg
with this file's apply in the place of that file's.  Everything is in the permuted numbering.

The exact cases.  W holds k / 4 with 1 <= |k| <= 7 in the kept columns and zeros in the dropped ones; r of restrict is wide
(26 bits) and so are r and C of prolong without a sum; where r.z is summed r has 12 bits and C as many as keep every whole slot
below 2^52 units at the largest size (18 less the bits of 7 nv).  Every sum's magnitudes are asserted below EXACT_LIMIT, so
every order of summation, fused or not, gives the same number.
"""
import numpy as np
import scipy.sparse as sp

import coarse_cases as kc
from exact_cases import EXACT_LIMIT
from solver_cases import STEP_GRID, Fx, inv_diag_fx, odd_ints, partials

MAX_VECS = 8                  # EHYB_COARSE_MAX_VECS
CUT = 2.0 ** -20              # EHYB_COARSE_VEC_CUT
AGG_ROWS = [1, 2, 63, 64, 65, 127, 128, 129, 257, 1000]   # rows per aggregate of scattered_aggregates, in turn
KERNEL_NV = [1, 3, 6, 8]
KERNEL_NAGG = 23              # two turns through AGG_ROWS and three more, as far as n allows


# ------------------------------------------------------------------ the restatement
def build_P(B, agg, nagg):
    """B (nv, n), agg (n,) -> (off (nagg + 1,) int32, W (nv, n)): the local bases of ehyb_coarse_create_host_vecs"""
    B = np.atleast_2d(np.asarray(B, dtype=np.float64))
    nv, n = B.shape
    W = np.zeros((nv, n))
    off = np.zeros(nagg + 1, dtype=np.int32)
    order = np.argsort(agg, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=nagg))])
    for a in range(nagg):
        rows = order[ptr[a]:ptr[a + 1]]
        kept = []
        for v in range(nv):
            t = B[v, rows].copy()
            norm0 = np.sqrt(t @ t)
            if not norm0 > 0:
                continue
            for _ in range(2):
                for q in kept:
                    t -= (q @ t) * q
            norm1 = np.sqrt(t @ t)
            if not norm1 >= CUT * norm0:
                continue
            kept.append(t / norm1)
        for j, q in enumerate(kept):
            W[j, rows] = q
        off[a + 1] = off[a] + len(kept)
    return off, W


def prolongation(agg, off, W):
    """P (n, nc): column off[a] + j holds W[j] on the rows of aggregate a"""
    nv, n = W.shape
    kept = np.diff(off)[agg]
    r, c, v = [], [], []
    for j in range(nv):
        rows = np.flatnonzero(j < kept)
        r.append(rows), c.append(off[agg[rows]] + j), v.append(W[j, rows])
    return sp.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(n, int(off[-1])))


def coarse_matrix(A, P):
    return np.asarray((P.T @ A @ P).todense())


def apply(r, dinv, P, einv):
    """z = D^-1 r + P E^-1 P^T r; dinv None: the identity"""
    return (r if dinv is None else dinv * r) + P @ (einv @ (P.T @ r))


def pcg(A, b, P, dinv=None, max_iter=1000, rtol=1e-10, x0=None, check_every=1, einv=None):
    """The loop of coarse_cases.pcg around this file's apply (einv None: numpy's inverse of P^T A P) -> (x, iterations)"""
    if einv is None:
        einv = np.linalg.inv(coarse_matrix(A, P))
    plain = kc.apply
    kc.apply = lambda r, d, _map, _einv: apply(r, d, P, einv)
    try:
        return kc.pcg(A, b, None, P.shape[1], dinv, max_iter=max_iter, rtol=rtol, x0=x0, check_every=check_every, einv=einv)
    finally:
        kc.apply = plain


# ------------------------------------------------------------------ a 3-D spring network
def spring_network(nx, ny, nz, shift, seed=0):
    """nx * ny * nz nodes on the unit lattice, three unknowns per node (node * 3 + component), a spring of stiffness uniform in
    [0.5, 1.5] along every axis edge and every face diagonal: K = sum of k d d^T blocks (d the unit vector of the spring) plus
    shift * I.  Without the shift the null space is the six rigid-body modes.  -> (K csr, coords (nodes, 3))"""
    rng = np.random.default_rng(seed)
    idx = np.arange(nx * ny * nz).reshape(nz, ny, nx)
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    coords = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1).astype(np.float64)
    steps = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1)]
    rows, cols, vals = [], [], []
    for dx, dy, dz in steps:
        def side(lo):
            return tuple(slice(max(0, -s if lo else s), size - max(0, s if lo else -s)) for s, size in ((dz, nz), (dy, ny), (dx, nx)))
        p, q = idx[side(True)].ravel(), idx[side(False)].ravel()
        d = np.array([dx, dy, dz], dtype=np.float64)
        d /= np.linalg.norm(d)
        k = rng.uniform(0.5, 1.5, len(p))
        for ca in range(3):
            for cb in range(3):
                w = k * d[ca] * d[cb]
                if not w.any():
                    continue
                for (u, v, s) in ((p, p, 1), (q, q, 1), (p, q, -1), (q, p, -1)):
                    rows.append(u * 3 + ca), cols.append(v * 3 + cb), vals.append(s * w)
    n = 3 * idx.size
    K = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    K.sum_duplicates()
    K = (K + K.T) * 0.5                                            # the two triangles were summed in different orders
    return (K + shift * sp.identity(n)).tocsr(), coords


# ------------------------------------------------------------------ exact cases of the two weighted kernels
def scattered_aggregates(n, seed=0, nagg=KERNEL_NAGG):
    """n rows in aggregates of AGG_ROWS rows in turn, as many (up to nagg) as n holds; what is left over goes to the aggregates of
    the largest kind present.  The rows of every aggregate are scattered over the whole index range.  -> (agg (n,) int32, nagg)"""
    size = []
    for a in range(nagg):
        if sum(size) + AGG_ROWS[a % len(AGG_ROWS)] > n:
            break
        size.append(AGG_ROWS[a % len(AGG_ROWS)])
    left = n - sum(size)
    big = [a for a in range(len(size)) if size[a] == max(size)]
    for k, a in enumerate(big):
        size[a] += left // len(big) + (1 if k < left % len(big) else 0)
    assert sum(size) == n and min(size) >= 1
    perm = np.random.default_rng(300 + seed).permutation(n)
    agg = np.empty(n, dtype=np.int32)
    agg[perm] = np.repeat(np.arange(len(size), dtype=np.int32), size)
    return agg, len(size)


def irregular_off(nagg, nv):
    """Kept columns per aggregate: even aggregates keep fewer than nv (nv - 1, half, and aggregate 2 none), odd ones every column,
    the last one fewer than nv -- as far as that leaves an unknown at all.  -> off (nagg + 1,) int32"""
    kept = np.full(nagg, nv, dtype=np.int64)
    kept[0::4] = max(nv - 1, 1)
    kept[2::4] = nv // 2
    if nagg > 2:
        kept[2] = 0
    kept[-1] = min(kept[-1], nv - 1)
    if kept.sum() == 0:
        kept[0] = 1
    return np.concatenate([[0], np.cumsum(kept)]).astype(np.int32)


def weights_fx(agg, off, nv, seed=0):
    """W: k / 4 with 1 <= |k| <= 7 in the kept columns of every row, zero in the dropped ones -> Fx with an (nv, n) mantissa"""
    rng = np.random.default_rng(400 + seed)
    n = len(agg)
    k = rng.integers(1, 8, (nv, n)) * rng.choice(np.array([-1, 1]), (nv, n))
    k[np.arange(nv)[:, None] >= np.diff(off)[agg][None, :]] = 0
    return Fx(k, 2)


def _ex(v, what="an intermediate"):
    assert v.peak() < EXACT_LIMIT, f"{what}: {v.peak():.3e} units, not exact in fp64"
    return v


def restrict_vec_case(agg, off, W, seed=0):
    """T[off[a] + j] = sum over the rows of a of W[j] r; r wide"""
    n, nc = len(agg), int(off[-1])
    r = Fx(odd_ints(np.random.default_rng(seed), n, 26), 3)
    t = np.zeros(nc, dtype=np.int64)
    for j in range(W.m.shape[0]):
        rows = np.flatnonzero(j < np.diff(off)[agg])
        at = off[agg[rows]] + j
        mag = np.bincount(at, weights=np.abs(W.m[j, rows] * r.m[rows]).astype(np.float64), minlength=nc)
        assert mag.max(initial=0) < EXACT_LIMIT, f"restrict: a sum's magnitudes add up to {mag.max():.3e} units"
        np.add.at(t, at, W.m[j, rows] * r.m[rows])
    return {"in": {"r": r}, "out": {"t": Fx(t, W.e + r.e)}}


def coarse_term(agg, off, W, c):
    """s[i] = sum over the kept columns j of W[j][i] C[off[agg[i]] + j] (Fx -> Fx), its magnitudes asserted"""
    kept, nc = np.diff(off)[agg], int(off[-1])
    s = np.zeros(len(agg), dtype=np.int64)
    mag = np.zeros(len(agg), dtype=np.int64)
    for j in range(W.m.shape[0]):
        term = np.where(j < kept, W.m[j] * c.m[np.minimum(off[agg] + j, nc - 1)], 0)
        s += term
        mag += np.abs(term)
    assert int(mag.max(initial=0)) < EXACT_LIMIT
    return Fx(s, W.e + c.e)


def prolong_vec_case(agg, off, W, with_dinv, summed, seed=0, grid=STEP_GRID):
    """z = D^-1 r + s; summed: the partials of r.z (r and C narrow), else r and C wide"""
    rng = np.random.default_rng(seed)
    n, nc, nv = len(agg), int(off[-1]), W.m.shape[0]
    dinv = inv_diag_fx(n) if with_dinv else None
    r = Fx(odd_ints(rng, n, 12 if summed else 26), 3)
    c = Fx(odd_ints(rng, nc, 18 - (7 * nv).bit_length() if summed else 30), 4 if summed else 6)
    z = _ex((r if dinv is None else _ex(r * dinv)) + coarse_term(agg, off, W, c))
    sums = {"rz": partials(r * z, grid, "coarse_prolong_vec rz")} if summed else {}
    return {"in": {"r": r, "c": c}, "dinv": dinv, "out": {"z": z}, "sums": sums}
