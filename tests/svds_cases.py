"""Inputs and the CPU yardstick for ehyb_svds.  No tests here (test_svds_host.py, test_gpu_svds_kernels.py, test_gpu_svds.py).

cpu_svds restates the solver's rules (include/ehyb.h, the ehyb_svds block) in numpy: Golub-Kahan-Lanczos bidiagonalisation with
full two-sided reorthogonalisation and a thick restart with Ritz vectors; the device is compared to it and test_svds_host.py holds
it against dense singular values.  systems() are the inputs of both: the matrices of lsqr_cases.py and a few small ones on which a
cycle ends early (a collapse).  trace: cpu_svds appends the deciding ratio of every half step, so that a test can assert that no
decision is near the threshold.

next_case, start_case: inputs for svds_next_kernel whose every output is ONE number in fp64, built with the machinery of
eigsh_cases.next_case: alpha and beta are 3 * 2^k, an exact root that is no power of two, w = beta v is built backwards from v so
that w / beta is a true division with an exact quotient, and h (g) is planted in Hessenberg copy 1."""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

import eigsh_cases as ec
import gmres_cases as gc
import lsqr_cases as lc
from solver_cases import Fx, _ex, odd_ints

MAX_BASIS, MAX_NSV = 64, 16
COLLAPSE = 2.0 ** -90
NEXT_J = [0, 1, 7, 8, 31, 63]
LEFT, RIGHT = 0, 1


def cpu_svds(A, nsv, basis=0, max_restarts=300, tol=1e-10, v0=None, trace=None):
    """ehyb_svds's rules in numpy on a SQUARE (padded) scipy matrix.  -> (s (found,), U (found, n), V (found, n), info) with info =
    {"found", "nconv", "multiplies", "restarts", "resid", "status", "collapse"}; status "ok" or "breakdown" (then found = nconv = 0);
    collapse None, "left" or "right".  trace: a list that receives (side, j, ratio) of every half step that had something to decide."""
    A = A.tocsr()
    At = A.T.tocsr()
    n = A.shape[0]
    m, keep = ec.resolve_basis(nsv, basis, n)
    info = {"found": 0, "nconv": 0, "multiplies": 0, "restarts": 0, "resid": np.zeros(0), "status": "breakdown", "collapse": None}
    none = (np.zeros(0), np.zeros((0, n)), np.zeros((0, n)), info)
    w = ec.start_vector(n) if v0 is None else np.asarray(v0, dtype=np.float64).copy()
    with np.errstate(all="ignore"):
        ww = w @ w
        if not np.isfinite(ww) or not ww > 0:
            return none
        P, Q = np.zeros((m + 1, n)), np.zeros((m, n))
        P[0] = w / np.sqrt(ww)
        B = np.zeros((m, m))
        k = mult = restarts = 0

        def ortho(w, basis_rows):
            h = np.zeros(len(basis_rows))
            for _ in range(2):
                c = basis_rows @ w
                w = w - c @ basis_rows
                h += c
            return w, h

        while True:
            J, Jl, beta, collapse = m, m, 0.0, None
            for j in range(k, m):
                # the left half
                w, h = ortho(A @ P[j], Q[:j])
                a2 = w @ w
                if not (np.isfinite(h).all() and np.isfinite(a2) and np.isfinite(h @ h + a2)):
                    info.update(multiplies=mult, restarts=restarts)
                    return none
                mult += 1
                B[:j, j] = h
                if trace is not None and h @ h + a2 > 0:
                    trace.append((LEFT, j, a2 / (h @ h + a2)))
                if a2 <= COLLAPSE * (h @ h + a2):
                    J, Jl, beta, collapse = j + 1, j, 0.0, "left"
                    break
                B[j, j] = np.sqrt(a2)
                Q[j] = w / B[j, j]
                # the right half
                w, g = ortho(At @ Q[j], P[:j + 1])
                b2 = w @ w
                if not (np.isfinite(g).all() and np.isfinite(b2) and np.isfinite(g @ g + b2)):
                    info.update(multiplies=mult, restarts=restarts)
                    return none
                mult += 1
                if trace is not None:
                    trace.append((RIGHT, j, b2 / (g @ g + b2)))
                if b2 <= COLLAPSE * (g @ g + b2):
                    J, Jl, beta, collapse = j + 1, j + 1, 0.0, "right"
                    break
                beta = np.sqrt(b2)
                P[j + 1] = w / beta
            if Jl == 0:                                     # a zero matrix (A p_0 = 0)
                info.update(multiplies=mult, restarts=restarts, status="ok", collapse=collapse)
                return none
            X, sig, Yt = np.linalg.svd(B[:Jl, :J], full_matrices=False)
            Y = Yt.T
            res = np.abs(beta * X[Jl - 1])
            want = min(nsv, Jl)
            nconv = 0
            while nconv < want and res[nconv] <= tol * sig[0]:
                nconv += 1
            if nconv == want or collapse or restarts == max_restarts:
                break
            kk = min(keep, J - 1)
            last = P[J].copy()
            P[:kk] = Y[:, :kk].T @ P[:J]
            P[kk] = last
            Q[:kk] = X[:, :kk].T @ Q[:Jl]
            B[:] = 0.0
            B[np.arange(kk), np.arange(kk)] = sig[:kk]
            k = kk
            restarts += 1
    info.update(found=want, nconv=nconv, multiplies=mult, restarts=restarts, resid=res[:want].copy(), status="ok", collapse=collapse)
    return sig[:want].copy(), X[:, :want].T @ Q[:Jl], Y[:, :want].T @ P[:J], info


# ------------------------------------------------------------------ the systems
def wide(seed=9636):
    """random 7 x 30, density 0.4: rank 7.  The Krylov space of the right vectors is p_0 plus the row space, dimension 8, and A p_7
    lies in the span of q_0 .. q_6: a left collapse at j = 7 (15 multiplies).  Its transpose ends one half step later by the
    restatement's (and the issue's) count: the alpha of step 7 is rounding noise, but noise of relative size 2^-26, far ABOVE the
    collapse threshold of 2^-45 -- the rule is a net for exact cases --, so q_7 is written and the right half collapses (16
    multiplies).  The seed is the first of 30,000 tried at which every deciding ratio of both runs is above 2^-60 or below
    2^-100 (test_svds_host.py asserts it): a typical seed leaves that alpha^2 ratio between 2^-95 and 2^-64."""
    rng = np.random.default_rng(seed)
    return sp.random(7, 30, density=0.4, random_state=rng, data_rvs=lambda k: rng.uniform(-1, 1, k)).tocsr()


def repeated_diagonal():
    """diag(5, 5, 4, 3, 2, 1, 1, .5, .1 x 8): ten distinct values among sixteen -- a right collapse with J = 10"""
    return sp.diags(np.r_[5.0, 5.0, 4.0, 3.0, 2.0, 1.0, 1.0, 0.5, np.full(8, 0.1)]).tocsr()


def systems():
    """name -> dict(A: square (padded) csr, nsv, basis, expect: (multiplies, restarts, collapse) of the restatement at tol 1e-10,
    found: what a collapse leaves, None = nsv)"""
    T = lc.tall()
    W = wide()
    out = {
        "convection-4": dict(A=lc.convection(), nsv=4, basis=0, expect=(408, 23, None)),
        "convection-1": dict(A=lc.convection(), nsv=1, basis=0, expect=(300, 13, None)),
        "convection-8-24": dict(A=lc.convection(), nsv=8, basis=24, expect=(464, 26, None)),
        "tall-6": dict(A=lc.padded(T), nsv=6, basis=0, expect=(208, 12, None)),
        "tall-T-6": dict(A=lc.padded(T.T.tocsr()), nsv=6, basis=0, expect=(208, 12, None)),
        "tall-16-40": dict(A=lc.padded(T), nsv=16, basis=40, expect=(320, 10, None)),
        "wide-7x30": dict(A=lc.padded(W), nsv=3, basis=0, expect=(15, 0, "left")),
        "wide-T": dict(A=lc.padded(W.T.tocsr()), nsv=3, basis=0, expect=(16, 0, "right")),
        "repeated-diagonal": dict(A=repeated_diagonal(), nsv=3, basis=0, expect=(20, 0, "right")),
        "identity": dict(A=sp.identity(10, format="csr"), nsv=2, basis=0, expect=(2, 0, "right"), found=1),
        "zero": dict(A=sp.csr_matrix((6, 6)), nsv=1, basis=0, expect=(1, 0, "left"), found=0),
    }
    return out


COLLAPSE_SYSTEMS = ("wide-7x30", "wide-T", "repeated-diagonal", "identity", "zero")


# ------------------------------------------------------------------ one launch at a time, exactly
def next_case(n, side, j, seed=0, k=1, h0=None):
    """side LEFT, step j: h_0 .. h_{j-1} planted in Hessenberg copy 1, alpha = 3 * 2^k; q_j = w / alpha.
    side RIGHT, step j: g_0 .. g_j planted, beta = 3 * 2^k; p_{j+1} = w / beta.  -> the count of planted coefficients as "count",
    the column that is written as "column"."""
    rng = np.random.default_rng(seed)
    count = j if side == LEFT else j + 1
    norm = 3 * Fraction(2) ** k
    h = [gc.DYADICS[(i + seed) % len(gc.DYADICS)] * 4 for i in range(count)]
    if h0 is not None:
        h[0] = Fraction(h0)
    v = Fx(odd_ints(rng, n, 26), 2)
    return {"side": side, "j": j, "count": count, "column": j if side == LEFT else j + 1, "h": [gc.exact(x) for x in h], "ww": norm * norm,
            "norm": gc.exact(norm), "w": _ex(gc.fx_of(norm) * v), "v": v}


def start_case(n, seed=0):
    """side RIGHT, j = -1: beta = 3/2 into gt[0], p_0 = w / beta"""
    c = gc.first_case(n, False, seed=seed)
    return {"ww": c["ww"], "norm": c["beta"], "w": c["w"], "v": c["v"]}
