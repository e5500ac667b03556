"""Inputs and the CPU yardstick for ehyb_lobpcg.  No tests here (test_lobpcg_host.py, test_gpu_lobpcg_kernels.py, test_gpu_lobpcg.py).

lap_grid, start_block, numpy_rr and cpu_lobpcg: the Laplacian-like test matrix, the start block and a numpy restatement of the
solver's rules (include/ehyb.h), to which the device is compared and which test_lobpcg_host.py holds against numpy.linalg.eigvalsh.
The restatement applies the TRUE preconditioner: for a coarse object its MAP and EINV host arrays, z = inv_diag o r + P E^-1 P^T r.
count_spread runs it once as it is and five times with G and H perturbed by symmetric relative noise of 4e-16: an iteration count
moves only where a residual sits within rounding of its threshold, and the spread says by how much.

gram_case, resid_case: inputs for the two kernels of ehyb_lobpcg.hip whose every output is ONE number in fp64 whatever the order of
summation, built with the machinery of solver_cases.py / gmres_cases.py (odd integers, power-of-two inv_diag, small dyadic scalars).
The Gram matrices sum n products of two 12-bit integers: below 2^24 n < 2^41 for the largest n.  A residual is AX - theta X with
11-bit AX, 10-bit X and theta in eighths of magnitude <= 3/2: a multiple of 1/8 below 2^12, its square a multiple of 1/64 below
2^24, and the n squares add up below 2^24 n units of 1/64 -- far below 2^53 for every n here."""
import numpy as np

import gmres_cases as gc
from eigsh_cases import sym_grid
from exact_cases import EXACT_LIMIT
from solver_cases import inv_diag_fx, odd_ints

MAX_BLOCK = 8
RANK_CUT = 2.0 ** -40


def lap_grid(nx, ny, seed):
    """sym_grid(nx, ny, seed, plant=False) with its diagonal replaced by minus the off-diagonal row sum plus 1e-3: a weighted grid
    Laplacian shifted just off singular, whose lowest modes are the smooth ones an aggregate coarse space removes"""
    A = sym_grid(nx, ny, seed, plant=False).tolil()
    off = np.asarray(A.sum(axis=1)).ravel() - A.diagonal()
    A.setdiag(-off + 1e-3)
    return A.tocsr()


def start_block(n, nb):
    """the start block of the header, (nb, n): x_ij = ((h & 2047) - 1023.5) / 1024 with the 32-bit hash of row i and column j"""
    i = np.arange(n, dtype=np.uint64)[None, :]
    j = np.arange(nb, dtype=np.uint64)[:, None]
    m = np.uint64(0xFFFFFFFF)
    h = ((i + np.uint64(1)) * np.uint64(2654435761) + (j + np.uint64(1)) * np.uint64(40503)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & m
    h ^= h >> np.uint64(13)
    return ((h & np.uint64(2047)).astype(np.float64) - 1023.5) / 1024.0


class RRError(ValueError):
    pass


def mirror(M):
    """the symmetric matrix of the upper triangle"""
    return np.triu(M) + np.triu(M, 1).T


def numpy_rr(G, H, nb):
    """ehyb_lobpcg_rr's rules with numpy.linalg.eigh for the two dense problems -> (theta (nb,), Y (mc, nb), rank)"""
    G, H = mirror(np.asarray(G, dtype=np.float64)), mirror(np.asarray(H, dtype=np.float64))
    mc = G.shape[0]
    g = G.diagonal()
    if not (np.isfinite(G).all() and np.isfinite(H).all()) or (g < 0).any():
        raise RRError("a non-finite entry or a negative diagonal")
    keep = np.flatnonzero(g > 0)
    if len(keep) < nb:
        raise RRError("rank")
    d = 1.0 / np.sqrt(g[keep])
    Gs = d[:, None] * G[np.ix_(keep, keep)] * d[None, :]
    np.fill_diagonal(Gs, 1.0)
    sigma, U = np.linalg.eigh(Gs)
    sel = sigma > RANK_CUT * sigma[-1]
    rank = int(sel.sum())
    if rank < nb:
        raise RRError("rank")
    Q = d[:, None] * U[:, sel] / np.sqrt(sigma[sel])[None, :]
    theta, Z = np.linalg.eigh(mirror(Q.T @ (H[np.ix_(keep, keep)] @ Q)))
    Y = np.zeros((mc, nb))
    Y[keep] = Q @ Z[:, :nb]
    return theta[:nb].copy(), Y, rank


def preconditioner(inv_diag=None, coarse_map=None, coarse_einv=None):
    """T of the header as a function of a vector: the two-level one with a map and E^-1, Jacobi with inv_diag alone, else None"""
    if coarse_map is not None:
        nc = coarse_einv.shape[0]
        dd = 1.0 if inv_diag is None else inv_diag
        return lambda r: dd * r + (coarse_einv @ np.bincount(coarse_map, weights=r, minlength=nc))[coarse_map]
    if inv_diag is not None:
        return lambda r: inv_diag * r
    return None


def cpu_lobpcg(A, nev, block=0, T=None, X0=None, max_iter=500, tol=1e-8, anorm=0.0, noise=None):
    """ehyb_lobpcg's rules in numpy.  T: a function of a vector (preconditioner()) or None.  noise: a numpy Generator -- G and H of
    every Rayleigh-Ritz step are multiplied entrywise by 1 + 4e-16 u with a symmetric u in [-1, 1).
    -> (evals (nev,), X (nev, n), info) with info = {"nconv", "iters", "multiplies", "resid", "status", "orth"}; status "ok" or
    "breakdown" (then nconv = 0); orth = the largest max |X^T X - I| seen at a residual step."""
    n = A.shape[0]
    nb = nev if block == 0 else block
    assert 1 <= nev <= nb <= MAX_BLOCK and nb <= n
    info = {"nconv": 0, "iters": 0, "multiplies": nb, "resid": np.full(nev, np.nan), "status": "breakdown", "orth": 0.0}

    def ritz(S, AS):
        G, H = S @ S.T, S @ AS.T
        if noise is not None:
            u = mirror(noise.uniform(-1.0, 1.0, G.shape))
            G, H = G * (1.0 + 4e-16 * u), H * (1.0 + 4e-16 * u)
        return numpy_rr(G, H, nb)

    with np.errstate(all="ignore"):
        X = start_block(n, nb) if X0 is None else np.array(X0, dtype=np.float64).reshape(nb, n)
        AX = (A @ X.T).T
        try:
            theta, Y, _ = ritz(X, AX)
        except RRError:
            return np.full(nev, np.nan), np.zeros((nev, n)), info
        X, AX = Y.T @ X, Y.T @ AX
        Pd = AP = None
        it = 0
        while True:
            R = AX - theta[:, None] * X
            res = np.sqrt((R * R).sum(axis=1))
            info["iters"] = it
            if not (np.isfinite(res).all() and np.isfinite(theta).all()):
                return np.full(nev, np.nan), np.zeros((nev, n)), info
            info["orth"] = max(info["orth"], np.abs(X @ X.T - np.eye(nb)).max())
            nrm = max(np.abs(theta).max(), anorm)
            conv = res <= tol * nrm
            nconv = 0
            while nconv < nev and conv[nconv]:
                nconv += 1
            if nconv == nev or it == max_iter:
                break
            active = np.flatnonzero(~conv)
            W = R[active] if T is None else np.array([T(r) for r in R[active]])
            AW = (A @ W.T).T
            info["multiplies"] += len(active)
            S = np.vstack([X, W] if Pd is None else [X, Pd, W])
            AS = np.vstack([AX, AW] if Pd is None else [AX, AP, AW])
            try:
                theta, Y, _ = ritz(S, AS)
            except RRError:
                return np.full(nev, np.nan), np.zeros((nev, n)), info
            Yp = Y.copy()
            Yp[:nb] = 0.0
            X, AX, Pd, AP = Y.T @ S, Y.T @ AS, Yp.T @ S, Yp.T @ AS
            it += 1
    info.update(nconv=nconv, resid=res[:nev].copy(), status="ok")
    return theta[:nev].copy(), X[:nev].copy(), info


def count_spread(A, nev, runs=5, **kw):
    """-> (min, max, plain): the restatement's iteration counts over the plain run and `runs` runs with noise"""
    plain = cpu_lobpcg(A, nev, **kw)[2]
    counts = [plain["iters"]] + [cpu_lobpcg(A, nev, noise=np.random.default_rng(100 + k), **kw)[2]["iters"] for k in range(runs)]
    return min(counts), max(counts), plain


# ------------------------------------------------------------------ one launch at a time, exactly
GRAM_SIZES = [1, 63, 64, 65, 1000, 4097, 70001]
GRAM_COLS = [1, 2, 8, 9, 16, 17, 24]
RESID_COLS = [1, 3, 8]
ACTIVE = ["all", "none", "first", "last", "alternate"]


def gram_case(n, mc, seed=0):
    """S and AS: mc columns of 12-bit odd integers each.  -> S, AS (mc, n) float64 and G = S S^T, H = S AS^T from the int64 products,
    H's lower triangle the mirror of its upper one (the kernel computes s_i . (A s)_j for i <= j)"""
    rng = np.random.default_rng(seed)
    S = np.array([odd_ints(rng, n, 12) for _ in range(mc)], dtype=np.int64).reshape(mc, n)
    AS = np.array([odd_ints(rng, n, 12) for _ in range(mc)], dtype=np.int64).reshape(mc, n)
    assert n * (1 << 24) < EXACT_LIMIT
    G, H = S @ S.T, S @ AS.T
    H = np.triu(H) + np.triu(H, 1).T
    assert (G == G.T).all()
    return {"S": S.astype(np.float64), "AS": AS.astype(np.float64), "G": G.astype(np.float64), "H": H.astype(np.float64)}


def active_mask(nb, which):
    return {"all": (1 << nb) - 1, "none": 0, "first": 1, "last": 1 << (nb - 1), "alternate": sum(1 << c for c in range(0, nb, 2))}[which]


def resid_case(n, nb, which, with_dinv, seed=0):
    """R_c = AX_c - theta_c X_c in eighths, res2_c = R_c . R_c in 64ths, W = inv_diag o R over the active columns, packed.
    -> X, AX (nb, n), theta (nb,), dinv (n,) or None, mask, res2 (nb,), W (na, n), all float64 and exact"""
    rng = np.random.default_rng(seed)
    X = np.array([odd_ints(rng, n, 10) for _ in range(nb)], dtype=np.int64).reshape(nb, n)
    AX = np.array([odd_ints(rng, n, 11) for _ in range(nb)], dtype=np.int64).reshape(nb, n)
    th = [gc.DYADICS[(3 * c + seed) % len(gc.DYADICS)] for c in range(nb)]
    th8 = np.array([int(t * 8) for t in th], dtype=np.int64)
    assert all(t * 8 == int(t * 8) for t in th)
    R8 = 8 * AX - th8[:, None] * X                                    # in eighths
    assert np.abs(R8).max(initial=0) < 1 << 15 and n * (1 << 30) < EXACT_LIMIT
    mask = active_mask(nb, which)
    cols = [c for c in range(nb) if mask >> c & 1]
    dinv = inv_diag_fx(n).f("inv_diag") if with_dinv else None
    R = R8.astype(np.float64) / 8.0
    W = R[cols] * (dinv[None, :] if with_dinv else 1.0)
    return {"X": X.astype(np.float64), "AX": AX.astype(np.float64), "theta": np.array([gc.exact(t) for t in th]), "dinv": dinv, "mask": mask,
            "res2": (R8 * R8).sum(axis=1).astype(np.float64) / 64.0, "W": W.reshape(len(cols), n)}
