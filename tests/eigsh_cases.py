"""Inputs and the CPU yardstick for ehyb_eigsh.  No tests here (test_eigsh_host.py, test_gpu_eigsh_kernels.py, test_gpu_eigsh.py).

sym_grid and cpu_eigsh: the test matrices and a numpy restatement of the solver's rules (include/ehyb.h), to which the device is
compared and which test_eigsh_host.py holds against numpy.linalg.eigvalsh.

rotate_case, next_case, first_case, scale_case: inputs for the three kernels of ehyb_eigsh.hip whose every output is ONE number in
fp64 whatever the order of summation, built with the machinery of solver_cases.py / gmres_cases.py (Fx scaled integers, planted
partials).  The rotation sums up to 65 products of a 12-bit odd integer and a small dyadic number: every partial sum in every
order is an integer of a few units of 2^-5 far below 2^52.  beta = 3 * 2^k is an exact root that is no power of two and
w = beta v is built backwards from v, so w / beta is a true division with an exact quotient."""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

import gmres_cases as gc
import solver_cases as sc
from exact_cases import EXACT_LIMIT
from solver_cases import Fx, _ex, odd_ints

MAX_BASIS, MAX_NEV = 64, 16
PLANT_UP = (40, 33, 27, 22, 18, 15)
PLANT_DOWN = (30, 25, 21, 17, 14, 12)


def sym_grid(nx, ny, seed, plant=True):
    """A weighted 5-point graph Laplacian on an nx x ny grid (edge weights U(0.5, 1.5)) plus a random positive diagonal U(0.1, 1).
    plant: six diagonal entries raised by PLANT_UP and six lowered by PLANT_DOWN, at twelve distinct random places -- the matrix is
    then indefinite with well-separated ends."""
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    diag = np.zeros(n)
    for a, b in ((idx[:, 1:].ravel(), idx[:, :-1].ravel()), (idx[1:, :].ravel(), idx[:-1, :].ravel())):
        w = -rng.uniform(0.5, 1.5, len(a))
        rows += [a, b]
        cols += [b, a]
        vals += [w, w]
        np.add.at(diag, a, -w)
        np.add.at(diag, b, -w)
    diag += rng.uniform(0.1, 1.0, n)
    if plant:
        where = rng.choice(n, len(PLANT_UP) + len(PLANT_DOWN), replace=False)
        diag[where[:len(PLANT_UP)]] += PLANT_UP
        diag[where[len(PLANT_UP):]] -= PLANT_DOWN
    rows.append(np.arange(n))
    cols.append(np.arange(n))
    vals.append(diag)
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    return A


def planted_diagonal(n, seed):
    """the planted entries of sym_grid alone, as a diagonal to add to another symmetric matrix"""
    rng = np.random.default_rng(seed)
    d = np.zeros(n)
    where = rng.choice(n, len(PLANT_UP) + len(PLANT_DOWN), replace=False)
    d[where[:len(PLANT_UP)]] += PLANT_UP
    d[where[len(PLANT_UP):]] -= PLANT_DOWN
    return d


def resolve_basis(nev, basis, n):
    """-> (m, keep) by the rule of the header"""
    b = min(max(2 * nev + 1, 20), MAX_BASIS) if basis == 0 else basis
    m = min(b, n)
    return m, nev + max(m - nev, 0) // 2


def start_vector(n):
    return 1.0 + (np.arange(n) % 7) / 8.0


def cpu_eigsh(A, nev, which="LA", basis=0, max_restarts=300, tol=1e-10, scale=None, v0=None):
    """ehyb_eigsh's rules in numpy.  -> (evals (found,), X (found, n), info) with info = {"found", "nconv", "multiplies",
    "restarts", "resid", "status"}; status "ok" or "breakdown" (then found = nconv = 0)."""
    n = A.shape[0]
    m, keep = resolve_basis(nev, basis, n)
    sc_ = np.ones(n) if scale is None else np.asarray(scale, dtype=np.float64)
    info = {"found": 0, "nconv": 0, "multiplies": 0, "restarts": 0, "resid": np.zeros(0), "status": "breakdown"}
    w = start_vector(n) if v0 is None else np.asarray(v0, dtype=np.float64).copy()
    with np.errstate(all="ignore"):
        ww = w @ w
        if not np.isfinite(ww) or not ww > 0:
            return np.zeros(0), np.zeros((0, n)), info
        V = np.zeros((m + 1, n))
        V[0] = w / np.sqrt(ww)
        T = np.zeros((m, m))
        k = mult = restarts = 0
        while True:
            J, beta, invariant = m, 0.0, False
            for j in range(k, m):
                w = sc_ * (A @ (sc_ * V[j]))
                mult += 1
                h = np.zeros(j + 1)
                for _ in range(2):
                    c = V[:j + 1] @ w
                    w = w - c @ V[:j + 1]
                    h += c
                b2 = w @ w
                if not (np.isfinite(h).all() and np.isfinite(b2) and np.isfinite(h @ h + b2)):
                    info["multiplies"] = mult - 1
                    info["restarts"] = restarts
                    return np.zeros(0), np.zeros((0, n)), info
                T[:j + 1, j] = h
                T[j, :j + 1] = h
                if b2 <= 2.0 ** -90 * (h @ h + b2):
                    J, beta, invariant = j + 1, 0.0, True
                    break
                beta = np.sqrt(b2)
                V[j + 1] = w / beta
            theta, Y = np.linalg.eigh(T[:J, :J])
            order = np.argsort(-theta, kind="stable") if which == "LA" else np.argsort(theta, kind="stable")
            theta, Y = theta[order], Y[:, order]
            res = np.abs(beta * Y[J - 1])
            want = min(nev, J)
            nrm = np.abs(theta).max()
            nconv = 0
            while nconv < want and res[nconv] <= tol * nrm:
                nconv += 1
            if nconv == want or invariant or restarts == max_restarts:
                break
            kk = min(keep, J - 1)
            last = V[J].copy()
            V[:kk] = Y[:, :kk].T @ V[:J]
            V[kk] = last
            T[:] = 0.0
            T[np.arange(kk), np.arange(kk)] = theta[:kk]
            k = kk
            restarts += 1
    info.update(found=want, nconv=nconv, multiplies=mult, restarts=restarts, resid=res[:want].copy(), status="ok")
    return theta[:want].copy(), Y[:, :want].T @ V[:J], info


# ------------------------------------------------------------------ one launch at a time, exactly
ROTATE_SHAPES = [(1, 1), (2, 1), (8, 8), (9, 9), (21, 15), (65, 1), (64, 41), (65, 64)]
NEXT_J = [0, 1, 7, 8, 31, 63]


def rotate_case(n, mc, kc, seed=0):
    """dst[:, c] = sum_l Y[l, c] src[:, l]: columns of 12-bit odd integers times 2^-(l mod 3), Y small dyadic numbers (eighths) with
    some zeros.  In units of 2^-5 every term is an integer and the magnitudes of a whole sum stay far below 2^52, so every order of
    summation, fused or not, gives one number -- and so does the float64 matrix product that states the expected result.
    -> src (mc, n), Y (mc, kc), dst (kc, n) as float64"""
    rng = np.random.default_rng(seed)
    src = np.array([v.f("src") for v in gc.basis(rng, n, mc, 12)]).reshape(mc, n)
    Y = np.array([[gc.exact(gc.DYADICS[(3 * l + 5 * c + seed) % len(gc.DYADICS)]) if (l + 2 * c + seed) % 5 else 0.0 for c in range(kc)]
                  for l in range(mc)])
    assert (src * 4 == np.round(src * 4)).all() and (Y * 8 == np.round(Y * 8)).all()
    assert (np.abs(Y).T @ np.abs(src)).max(initial=0.0) * 32 < EXACT_LIMIT
    return {"src": src, "Y": Y, "dst": Y.T @ src}


def next_case(n, j, with_scale, seed=0, k=1, h0=None):
    """step j >= 0: h planted in Hessenberg copy 1, beta = 3 * 2^k; v_{j+1} = w / beta, z = scale o v_{j+1}"""
    rng = np.random.default_rng(seed)
    scale = sc.inv_diag_fx(n) if with_scale else None
    beta = 3 * Fraction(2) ** k
    h = [gc.DYADICS[(i + seed) % len(gc.DYADICS)] * 4 for i in range(j + 1)]
    if h0 is not None:
        h[0] = Fraction(h0)
    v = Fx(odd_ints(rng, n, 26), 2)
    return {"j": j, "scale": scale, "h": [gc.exact(x) for x in h], "ww": beta * beta, "beta": gc.exact(beta), "w": _ex(gc.fx_of(beta) * v),
            "v": v, "z": v if scale is None else _ex(v * scale)}


def scale_case(n, seed=0):
    rng = np.random.default_rng(seed)
    scale = sc.inv_diag_fx(n)
    w = Fx(odd_ints(rng, n, 30), 4)
    return {"scale": scale, "w": w, "out": _ex(w * scale)}
