"""The two-level preconditioner (coarse.cpp, ehyb_coarse.hip) restated in numpy, and exact cases for its three kernels in
the style of solver_cases.py.  No tests here (test_coarse_host.py, test_gpu_coarse_kernels.py, test_gpu_coarse.py).

The restatement follows include/ehyb.h line for line: aggregate (growth, fragments, the automatic size, dof > 1), coarse_matrix
(E = P^T A P), apply (z = D^-1 r + P E^-1 P^T r) and pcg (the CG around it, the stopping test made every check_every iterations
as the device makes it).  Everything is in the permuted numbering: the matrix after ehyb_matrix_reorder.

The exact cases.  r of restrict and T of solve are wide scaled integers (26 bits), E^-1 holds small dyadic numbers (k / 4,
|k| <= 7, symmetric), inv_diag is the powers of two of solver_cases.inv_diag_fx; every sum's magnitudes are asserted to add up
below EXACT_LIMIT, so every order of summation gives the same number.  r of prolong cannot be wide where r.z is summed (its
term dinv r^2 is a square): 12 bits there, and C 18, so that the whole slot stays below 2^52 units at the largest size; with
rz = -1 (no sum) r and C are wide.
"""
import numpy as np
import scipy.sparse as sp

from exact_cases import EXACT_LIMIT
from solver_cases import STEP_GRID, Fx, dyadic, inv_diag_fx, odd_ints, partials  # noqa: F401

COARSE_MAX = 2048             # EHYB_COARSE_MAX
UNKNOWN_ROWS = [1, 2, 63, 64, 65, 127, 128, 129, 1000]   # rows per unknown of scattered_map, in turn
KERNEL_NC = [1, 3, 64, 65, 130]


# ------------------------------------------------------------------ the restatement
def default_agg_rows(n, dof=1):
    return max(128, -(-n * dof // 1536))


def aggregate(indptr, indices, part_boundary, agg_rows, dof=1, reorder_list=None):
    """ehyb_coarse_map -> (map (n,) int32, nc)"""
    n = len(indptr) - 1
    if agg_rows <= 0:
        agg_rows = default_agg_rows(n, dof)
    agg = np.full(n, -1, dtype=np.int64)
    count = 0
    for p in range(len(part_boundary) - 1):
        lo, hi = int(part_boundary[p]), int(part_boundary[p + 1])
        first, grown = count, []
        # growth: the seed is the lowest row not yet in an aggregate; breadth-first over the entries in stored order
        for seed in range(lo, hi):
            if agg[seed] >= 0:
                continue
            agg[seed] = count
            queue, head = [seed], 0
            while head < len(queue) and len(queue) < agg_rows:
                i = queue[head]
                head += 1
                for j in indices[indptr[i]:indptr[i + 1]].tolist():
                    if len(queue) >= agg_rows:
                        break
                    if lo <= j < hi and agg[j] < 0:
                        agg[j] = count
                        queue.append(j)
            grown.append(len(queue))
            count += 1
        # fragments: in order of rising size as grown, ties by number; judged by the size they have now
        for a in sorted(range(first, count), key=lambda a: (grown[a - first], a)):
            rows = np.flatnonzero(agg[lo:hi] == a) + lo
            if len(rows) == 0 or 4 * len(rows) >= agg_rows:
                continue
            cols = np.concatenate([indices[indptr[i]:indptr[i + 1]] for i in rows])
            cols = cols[(cols >= lo) & (cols < hi)]
            target = agg[cols]
            target = target[target != a]
            if len(target) == 0:
                continue                                        # no neighbour in the partition: it stays
            votes = np.bincount(target - first, minlength=count - first)
            agg[rows] = first + int(np.argmax(votes))           # (argmax: the lowest number among equals)
    _, agg = np.unique(agg, return_inverse=True)                # the survivors keep their order
    if dof > 1:
        old = np.empty(n, dtype=np.int64)
        old[np.asarray(reorder_list, dtype=np.int64)] = np.arange(n)    # reorder_list[old] = new
        _, agg = np.unique(agg * dof + old % dof, return_inverse=True)  # pairs that hold a row, in order of (aggregate, component)
    return agg.astype(np.int32), int(agg.max()) + 1 if n else 0


def prolongation(cmap, nc):
    n = len(cmap)
    return sp.csr_matrix((np.ones(n), (np.arange(n), cmap)), shape=(n, nc))


def coarse_matrix(A, cmap, nc):
    """E = P^T A P, dense"""
    P = prolongation(cmap, nc)
    return np.asarray((P.T @ A @ P).todense())


def transpose(cmap, nc):
    """ROW_PTR, ROWS: the rows of every unknown, rising"""
    rows = np.argsort(cmap, kind="stable").astype(np.int32)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(cmap, minlength=nc))]).astype(np.int32)
    return row_ptr, rows


def apply(r, dinv, cmap, einv):
    """z = D^-1 r + P E^-1 P^T r; dinv None: the identity"""
    t = np.bincount(cmap, weights=r, minlength=einv.shape[0])
    return (r if dinv is None else dinv * r) + (einv @ t)[cmap]


def pcg(A, b, cmap, nc, dinv=None, max_iter=1000, rtol=1e-10, x0=None, check_every=1, einv=None):
    """The solve of ehyb_pcg_coarse, iteration for iteration (einv None: numpy's inverse of this file's own E) -> (x, iterations)"""
    if einv is None:
        einv = np.linalg.inv(coarse_matrix(A, cmap, nc))
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = b.copy() if x0 is None else b - A @ x0
    z = apply(r, dinv, cmap, einv)
    p, rz, bb = z.copy(), r @ z, (b @ b) or 1.0
    it = 0
    while it < max_iter and (it % check_every or np.sqrt((r @ r) / bb) > rtol):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = apply(r, dinv, cmap, einv)
        rz, rz_old = r @ z, rz
        p = z + (rz / rz_old) * p
        it += 1
    return x, it


# ------------------------------------------------------------------ the freezing mix at full size (test_gpu_precond_full.py)
# The right-hand-side bank of test_gpu_solver_kernels.MIX_KINDS (cheb_cases.mix_bank, mix_x0) with the e of its "near" columns
# (b = A x*, x0 = x* + e u) chosen for this solver.  Relative residual per unit e on spd_matrix(1024, 921, 3000, 21) after 0, 2, 4,
# 6, 8 iterations, from pcg above with the library's own map and E^-1 (ehyb_coarse_map with the automatic agg_rows = 614:
# nc = 1735; the host object's arrays "map" and "Einv"), everything in the permuted numbering:
#   with inv_diag      3.40  0.359  0.120  0.0555  0.0304     a random b from x0 = 0 is at 7.0e-2 after 12
#   without            3.40  0.407  0.127  0.0585  0.0326                                   7.5e-2
# (the two "near" columns measured, u of columns 0 and 3, agree to two digits.)  MIX_E[with inv_diag] = the three e that cross
# MIX_RTOL = 1e-6 at check points 2, 4 and 6 (check_every = 2): each near the geometric middle of its interval,
# 1e-6 / sqrt(residual before * residual after), a factor of 1.4 to 3.1 from either edge.  With them pcg above stops the seven
# columns of the bank after 4, 0, 12, 2, 6, 4, 12 iterations, with inv_diag and without.  These numbers are measured from the
# restatement on the CPU, not from the device; no host test repeats them: the restatement alone takes 1.7 s for the bank, the
# matrix, its reordering and the host object another 2 s, and the slowest host test of this solver takes 0.5 s.
MIX_E = {True: (9e-7, 4.8e-6, 1.2e-5), False: (8.5e-7, 4.4e-6, 1.2e-5)}


def near_singular_grid(nx, ny, seed, shift):
    """test_gpu_cg.spd_matrix's construction with extra = 0 and the diagonal = row sum + shift"""
    rng = np.random.default_rng(seed)
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    r = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel(), rng.integers(0, n, 0)])
    c = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel(), rng.integers(0, n, 0)])
    v = -rng.uniform(0.5, 1.5, len(r))
    A = sp.coo_matrix((np.concatenate([v, v]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    d = np.asarray(abs(A).sum(axis=1)).ravel() + shift
    return (A + sp.diags(d)).tocsr()


def spd_on_the_pattern(A, shift):
    """An SPD matrix on the pattern of a symmetric A (the generators' values are indefinite): -|a_ij| off the diagonal, the
    diagonal = the row's sum of magnitudes + shift.  Its near-null vector is the constant, which the per-component constants of
    dof > 1 contain."""
    off = -abs(sp.csr_matrix(A))
    off.setdiag(0.0)
    off.eliminate_zeros()
    d = np.asarray(abs(off).sum(axis=1)).ravel() + shift
    return (off + sp.diags(d)).tocsr()


# ------------------------------------------------------------------ exact cases of the three kernels
def _ex(v, what="an intermediate"):
    assert v.peak() < EXACT_LIMIT, f"{what}: {v.peak():.3e} units, not exact in fp64"
    return v


def scattered_map(n, nc, seed=0):
    """A map of n rows onto nc unknowns that hold UNKNOWN_ROWS rows in turn (as far as n allows; what is left over goes to the
    unknowns of the largest kind, or to the last one), their rows scattered over the whole index range.  None: n < nc."""
    if n < nc or nc < 1:
        return None
    want = [UNKNOWN_ROWS[u % len(UNKNOWN_ROWS)] for u in range(nc)]
    size, left = [], n
    for u, w in enumerate(want):
        size.append(max(1, min(w, left - (nc - 1 - u))))
        left -= size[-1]
    big = [u for u in range(nc) if want[u] == max(want)] or [nc - 1]
    for k, u in enumerate(big):
        size[u] += left // len(big) + (1 if k < left % len(big) else 0)
    assert sum(size) == n and min(size) >= 1
    perm = np.random.default_rng(100 + seed).permutation(n)
    cmap = np.empty(n, dtype=np.int32)
    cmap[perm] = np.repeat(np.arange(nc, dtype=np.int32), size)
    return cmap


def einv_fx(nc, seed=0):
    """E^-1 of the kernel tests: k / 4 with |k| <= 7, symmetric, no zero -> Fx with an (nc, nc) mantissa"""
    rng = np.random.default_rng(200 + seed)
    k = rng.integers(1, 8, (nc, nc)) * rng.choice(np.array([-1, 1]), (nc, nc))
    k = np.tril(k) + np.tril(k, -1).T
    return Fx(k, 2)


def group_sums(terms, cmap, nc, what):
    """per unknown the sum of the terms of its rows (Fx -> Fx); the magnitudes of every sum stay below EXACT_LIMIT"""
    mag = np.bincount(cmap, weights=np.abs(terms.m).astype(np.float64), minlength=nc)
    assert mag.max(initial=0) < EXACT_LIMIT, f"{what}: a sum's magnitudes add up to {mag.max():.3e} units"
    out = np.zeros(nc, dtype=np.int64)
    np.add.at(out, cmap, terms.m)
    return Fx(out, terms.e)


def restrict_case(n, cmap, nc, seed=0):
    """T[u] = sum of r over the rows of u; r wide"""
    r = Fx(odd_ints(np.random.default_rng(seed), n, 26), 3)
    return {"in": {"r": r}, "out": {"t": group_sums(r, cmap, nc, "restrict")}}


def solve_case(nc, seed=0):
    """C = E^-1 T; T wide"""
    einv = einv_fx(nc, seed)
    t = Fx(odd_ints(np.random.default_rng(seed), nc, 26), 3)
    assert int((np.abs(einv.m) @ np.abs(t.m)).max()) < EXACT_LIMIT
    return {"einv": einv, "in": {"t": t}, "out": {"c": Fx(einv.m @ t.m, einv.e + t.e)}}


def prolong_case(n, cmap, nc, with_dinv, summed, seed=0, grid=STEP_GRID):
    """z = D^-1 r + C[map]; summed: the partials of r.z (r and C narrow), else r and C wide"""
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    r = Fx(odd_ints(rng, n, 12 if summed else 26), 3)
    c = Fx(odd_ints(rng, nc, 18 if summed else 30), 6)
    z = _ex((r if dinv is None else _ex(r * dinv)) + Fx(c.m[cmap], c.e))
    sums = {"rz": partials(r * z, grid, "coarse_prolong rz")} if summed else {}
    return {"in": {"r": r, "c": c}, "dinv": dinv, "out": {"z": z}, "sums": sums}
