"""Inputs and the CPU yardstick for ehyb_lobpcg_gen, the solver for K x = lambda M x.  No tests here (test_lobpcg_gen_host.py,
test_gpu_lobpcg_gen_kernels.py, test_gpu_lobpcg_gen.py).

mass_grid: a mass matrix on the grid of eigsh_cases.sym_grid, and its lumped form.  cpu_lobpcg_gen: lobpcg_cases.cpu_lobpcg with
the third image BS = M S carried through every rotation (a lumped mass, a 1-D array, is applied where S is read), the unchanged
numpy_rr on G = S^T BS and H = S^T AS, the residual AX - theta BX and the threshold tol max(bnorm max |theta|, anorm).

gram_b_case, resid_b_case: exact-integer inputs in the manner of lobpcg_cases.gram_case / resid_case.  Stored form: BS (BX) is a
third set of odd integers, independent of S (X), so that a kernel reading S for BS shows.  Lumped form: m takes the values 1, 2, 4
-- every product m s is exact, and a kernel that applies m twice or not at all shows at every row where m != 1 -- and S is
narrowed to 11 bits: a term of G is below 4 * 2^22, and n of them stay below EXACT_LIMIT (asserted)."""
import numpy as np
import scipy.sparse as sp

import gmres_cases as gc
import lobpcg_cases as lc
from exact_cases import EXACT_LIMIT
from solver_cases import inv_diag_fx, odd_ints


def mass_grid(nx, ny, seed):
    """-> (M csr, lumped): rho = U(0.5, 2) on the diagonal and min(rho_i, rho_j) / 8 on every edge of the nx x ny grid (numbered as
    sym_grid).  A row has at most four edges of at most rho_i / 8 each: strictly diagonally dominant with a positive diagonal,
    hence SPD.  lumped = the row sums."""
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    rho = np.random.default_rng(1000 + seed).uniform(0.5, 2.0, n)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [rho]
    for a, b in ((idx[:, 1:].ravel(), idx[:, :-1].ravel()), (idx[1:, :].ravel(), idx[:-1, :].ravel())):
        w = np.minimum(rho[a], rho[b]) / 8.0
        rows += [a, b]
        cols += [b, a]
        vals += [w, w]
    M = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    M.sort_indices()
    return M, np.asarray(M.sum(axis=1)).ravel()


def mass_dense(M):
    return np.diag(M) if np.ndim(M) == 1 else M.toarray()


def cpu_lobpcg_gen(A, M, nev, block=0, T=None, X0=None, max_iter=500, tol=1e-8, anorm=0.0, bnorm=0.0, noise=None):
    """ehyb_lobpcg_gen's rules in numpy.  M: a sparse matrix (consistent) or a 1-D array (lumped).  Everything else as
    lobpcg_cases.cpu_lobpcg -> (evals, X, info), info["orth"] = the largest max |X M X^T - I| seen, info["mass_multiplies"]."""
    n = A.shape[0]
    nb = nev if block == 0 else block
    assert 1 <= nev <= nb <= lc.MAX_BLOCK and nb <= n
    lumped = np.ndim(M) == 1
    bn = 1.0 if bnorm == 0 else bnorm
    mass = (lambda V: V * M[None, :]) if lumped else (lambda V: (M @ V.T).T)
    info = {"nconv": 0, "iters": 0, "multiplies": nb, "mass_multiplies": 0 if lumped else nb, "resid": np.full(nev, np.nan),
            "status": "breakdown", "orth": 0.0}

    def ritz(S, AS, BS):
        G, H = S @ BS.T, S @ AS.T
        if noise is not None:
            u = lc.mirror(noise.uniform(-1.0, 1.0, G.shape))
            G, H = G * (1.0 + 4e-16 * u), H * (1.0 + 4e-16 * u)
        return lc.numpy_rr(G, H, nb)

    with np.errstate(all="ignore"):
        X = lc.start_block(n, nb) if X0 is None else np.array(X0, dtype=np.float64).reshape(nb, n)
        AX, BX = (A @ X.T).T, mass(X)
        try:
            theta, Y, _ = ritz(X, AX, BX)
        except lc.RRError:
            return np.full(nev, np.nan), np.zeros((nev, n)), info
        X, AX, BX = Y.T @ X, Y.T @ AX, Y.T @ BX
        Pd = AP = BP = None
        it = 0
        while True:
            R = AX - theta[:, None] * BX
            res = np.sqrt((R * R).sum(axis=1))
            info["iters"] = it
            if not (np.isfinite(res).all() and np.isfinite(theta).all()):
                return np.full(nev, np.nan), np.zeros((nev, n)), info
            info["orth"] = max(info["orth"], np.abs(X @ BX.T - np.eye(nb)).max())
            nrm = max(bn * np.abs(theta).max(), anorm)
            conv = res <= tol * nrm
            nconv = 0
            while nconv < nev and conv[nconv]:
                nconv += 1
            if nconv == nev or it == max_iter:
                break
            active = np.flatnonzero(~conv)
            W = R[active] if T is None else np.array([T(r) for r in R[active]])
            AW, BW = (A @ W.T).T, mass(W)
            info["multiplies"] += len(active)
            info["mass_multiplies"] += 0 if lumped else len(active)
            S = np.vstack([X, W] if Pd is None else [X, Pd, W])
            AS = np.vstack([AX, AW] if Pd is None else [AX, AP, AW])
            BS = np.vstack([BX, BW] if Pd is None else [BX, BP, BW])
            try:
                theta, Y, _ = ritz(S, AS, BS)
            except lc.RRError:
                return np.full(nev, np.nan), np.zeros((nev, n)), info
            Yp = Y.copy()
            Yp[:nb] = 0.0
            X, AX, BX, Pd, AP, BP = Y.T @ S, Y.T @ AS, Y.T @ BS, Yp.T @ S, Yp.T @ AS, Yp.T @ BS
            it += 1
    info.update(nconv=nconv, resid=res[:nev].copy(), status="ok")
    return theta[:nev].copy(), X[:nev].copy(), info


def count_spread_gen(A, M, nev, runs=5, **kw):
    """-> (min, max, plain): the restatement's iteration counts over the plain run and `runs` runs with noise, as count_spread"""
    plain = cpu_lobpcg_gen(A, M, nev, **kw)[2]
    counts = [plain["iters"]] + [cpu_lobpcg_gen(A, M, nev, noise=np.random.default_rng(100 + k), **kw)[2]["iters"] for k in range(runs)]
    return min(counts), max(counts), plain


# ------------------------------------------------------------------ one launch at a time, exactly
GRAM_SIZES = [1, 63, 64, 65, 127, 128, 129, 1000, 4097, 70001]
GRAM_COLS = [1, 8, 9, 17, 24]
RESID_SIZES = [1, 64, 257, 2 * gc.S + 3]
MASS_VALUES = np.array([1, 2, 4], dtype=np.int64)


def mass_ints(n):
    """m in {1, 2, 4}, varying with the index and not with the period of a tile, a wave or a grid stride"""
    i = np.arange(n, dtype=np.int64)
    return MASS_VALUES[(i * 5 + i // 7 + i // 128) % 3]


def gram_b_case(n, mc, lumped, seed=0):
    """-> S, AS, BS (mc, n), m (n,) or None, G = S BS^T and H = S AS^T from the int64 products, the lower triangles the mirrors of
    the upper ones (the kernel computes s_i . (B s)_j and s_i . (A s)_j for i <= j), all float64 and exact"""
    rng = np.random.default_rng(seed)
    ints = lambda bits: np.array([odd_ints(rng, n, bits) for _ in range(mc)], dtype=np.int64).reshape(mc, n)   # noqa: E731
    if lumped:
        S, AS, m = ints(11), ints(12), mass_ints(n)
        BS = S * m[None, :]
        assert n * 4 * (1 << 22) < EXACT_LIMIT and n * (1 << 23) < EXACT_LIMIT
    else:
        S, AS, BS, m = ints(12), ints(12), ints(12), None
        assert n * (1 << 24) < EXACT_LIMIT
    G, H = S @ BS.T, S @ AS.T
    assert np.abs(G).max() < EXACT_LIMIT and np.abs(H).max() < EXACT_LIMIT
    G, H = np.triu(G) + np.triu(G, 1).T, np.triu(H) + np.triu(H, 1).T
    f = lambda a: None if a is None else a.astype(np.float64)   # noqa: E731
    return {"S": f(S), "AS": f(AS), "BS": f(BS), "m": f(m), "G": f(G), "H": f(H)}


def resid_b_case(n, nb, which, with_dinv, lumped, seed=0):
    """R_c = AX_c - theta_c BX_c in eighths, res2_c = R_c . R_c in 64ths, W = inv_diag o R over the active columns, packed.  BX: 10-bit
    odd integers of its own, or m o X.  |R8| < 2^14 + 12 * 2^12 < 2^16, a square below 2^32, n of them below EXACT_LIMIT (asserted).
    -> X, AX, BX (nb, n), m (n,) or None, theta (nb,), dinv (n,) or None, mask, res2 (nb,), W (na, n), all float64 and exact"""
    rng = np.random.default_rng(seed)
    ints = lambda bits: np.array([odd_ints(rng, n, bits) for _ in range(nb)], dtype=np.int64).reshape(nb, n)   # noqa: E731
    X, AX = ints(10), ints(11)
    m = mass_ints(n) if lumped else None
    BX = X * m[None, :] if lumped else ints(10)
    th = [gc.DYADICS[(3 * c + seed) % len(gc.DYADICS)] for c in range(nb)]
    th8 = np.array([int(t * 8) for t in th], dtype=np.int64)
    assert all(t * 8 == int(t * 8) for t in th)
    R8 = 8 * AX - th8[:, None] * BX                                   # in eighths
    assert np.abs(R8).max(initial=0) < 1 << 16 and n * (1 << 32) < EXACT_LIMIT
    mask = lc.active_mask(nb, which)
    cols = [c for c in range(nb) if mask >> c & 1]
    dinv = inv_diag_fx(n).f("inv_diag") if with_dinv else None
    R = R8.astype(np.float64) / 8.0
    W = R[cols] * (dinv[None, :] if with_dinv else 1.0)
    f = lambda a: None if a is None else a.astype(np.float64)   # noqa: E731
    return {"X": f(X), "AX": f(AX), "BX": f(BX), "m": f(m), "theta": np.array([gc.exact(t) for t in th]), "dinv": dinv, "mask": mask,
            "res2": (R8 * R8).sum(axis=1).astype(np.float64) / 64.0, "W": W.reshape(len(cols), n)}
