"""What the tests of ehyb_lsqr share.  No tests here (test_lsqr_host.py, test_gpu_lsqr_kernels.py, test_gpu_lsqr.py).

cpu_lsqr restates the device's recurrences, stop rules and breakdown rules (include/ehyb.h, the ehyb_lsqr block) in numpy, with
the Lanczos vectors stored unnormalised as the device stores them.  systems() builds the six test systems, every one with 1,440
rows once padded square.

The second half holds inputs for the six vector kernels of ehyb_lsqr.hip whose every output is ONE number in fp64 -- the
counterpart of minres_cases.py, built with the machinery of solver_cases.py (Fx scaled integers, planted partials, exact partial
sums).  A kernel forms every scalar itself, sums from the 512 planted partials of a slot and the rotations from the planted state
copy, so the cases choose them such that every root, quotient and hypot is exact or a single correctly rounded operation:
  alpha^2, beta^2, beta'^2, alpha'^2 are squares of dyadic numbers (9/4, 25/16, 4, 1/4 ...), so the roots are exact and
    alpha / beta, beta' / alpha are small dyadics or one rounded division; t is built backwards (t = alpha * (...)) so that
    t / alpha comes out exact although alpha (3/2, 5/4) is no power of two;
  the update's rotations are (3, 4, 5) triples times powers of two: rhobar1 = hypot(rhobar, damp) and rho = hypot(rhobar1, beta')
    are exact, cs, sn, phi / rho and theta / rho are restated operation by operation in fp64 (update_scalars), and x' =
    fma(phi / rho, w, x), w' = fma(-theta / rho, w, V / alpha') are each ONE rounding of an exact sum, formed here in integer
    arithmetic (w, x and V / alpha' kept to 8 bits so that the sum fits an int64).
"""
import math
from fractions import Fraction

import numpy as np

import solver_cases as sc
from solver_cases import Fx, STEP_GRID, _ex, odd_ints, partials

NX, NY = 40, 36                       # 1,440 rows
N = NX * NY
M_COLS = 600                          # columns of the over-determined system

STATE = ("rhobar", "phibar", "cs2", "sn2", "z", "xxnorm", "res2", "anorm2", "rnorm", "arnorm", "xnorm", "bnorm")


# ------------------------------------------------------------------ the restatement
def stop_test(st, atol, btol):
    """lsqr_stop of ehyb_lsqr.hip on a state dict: 1, 2 or 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = atol * np.sqrt(st["anorm2"])
        if st["rnorm"] <= t * st["xnorm"] + btol * st["bnorm"]:
            return 1
        if st["arnorm"] <= t * st["rnorm"]:
            return 2
    return 0


def cpu_lsqr(A, b, x0=None, damp=0.0, atol=1e-10, btol=1e-10, max_iter=1000, iterates=None):
    """The device's recurrences, stop and breakdown rules in numpy on a SQUARE (padded) scipy matrix.
    -> (x, info) with info as ehyb_lsqr_info; iterates: a list that receives x after every update."""
    A = A.tocsr()
    At = A.T.tocsr()
    x = np.zeros_like(b, dtype=np.float64) if x0 is None else np.array(x0, dtype=np.float64)

    def info(istop, it, st):
        return {"istop": istop, "iters": it, "rnorm": st["rnorm"], "arnorm": st["arnorm"], "anorm": float(np.sqrt(st["anorm2"])),
                "xnorm": st["xnorm"]}

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        U = b - A @ x
        b2, bb = U @ U, b @ b
        nan = dict.fromkeys(STATE, np.nan)
        if not (np.isfinite(bb) and np.isfinite(b2)):
            return x, info(-1, 0, nan)
        beta = np.sqrt(b2)
        a2 = 0.0
        V = np.zeros_like(x)
        if b2 > 0:
            V = (At @ U) / beta
            a2 = V @ V
            if not np.isfinite(a2):
                return x, info(-1, 0, nan)
        alpha = np.sqrt(a2)
        st = dict(rhobar=alpha, phibar=beta, cs2=-1.0, sn2=0.0, z=0.0, xxnorm=0.0, res2=0.0, anorm2=0.0, rnorm=beta,
                  arnorm=alpha * beta, xnorm=0.0, bnorm=beta)
        if b2 == 0 or a2 == 0:
            return x, info(0, 0, st)
        w = V / alpha
        it = 0
        while it < max_iter:
            stop = stop_test(st, atol, btol)
            if stop:
                return x, info(stop, it, st)
            if not (np.isfinite(a2) and a2 > 0 and np.isfinite(b2) and b2 > 0 and np.isfinite(alpha / beta)):
                return x, info(-1, it, st)
            U = (A @ V) / alpha - (alpha / beta) * U
            b2n = U @ U
            if not (np.isfinite(b2n) and b2n >= 0):
                return x, info(-1, it, st)
            beta_n = np.sqrt(b2n)
            a2n = 0.0
            if b2n > 0:
                if not np.isfinite(beta_n / alpha):
                    return x, info(-1, it, st)
                V = (At @ U) / beta_n - (beta_n / alpha) * V
                a2n = V @ V
            alpha_n = np.sqrt(a2n)
            rhobar1 = np.hypot(st["rhobar"], damp)
            cs1, sn1 = st["rhobar"] / rhobar1, damp / rhobar1
            psi, phibar1 = sn1 * st["phibar"], cs1 * st["phibar"]
            rho = np.hypot(rhobar1, beta_n)
            cs, sn = rhobar1 / rho, beta_n / rho
            theta, phi, phibar_n = sn * alpha_n, cs * phibar1, sn * phibar1
            tau = sn * phi
            t1, t2 = phi / rho, theta / rho
            if not (np.isfinite(a2n) and a2n >= 0 and np.isfinite(rho) and rho > 0 and np.isfinite(t1) and np.isfinite(t2)):
                return x, info(-1, it, st)
            delta, gbar = st["sn2"] * rho, -st["cs2"] * rho
            rhs = phi - delta * st["z"]
            zbar = rhs / gbar
            gamma = np.hypot(gbar, theta)
            zn = rhs / gamma
            res2n = st["res2"] + psi * psi
            x = x + t1 * w
            if a2n > 0:
                w = V / alpha_n - t2 * w
            st = dict(rhobar=-cs * alpha_n, phibar=phibar_n, cs2=gbar / gamma, sn2=theta / gamma, z=zn, xxnorm=st["xxnorm"] + zn * zn,
                      res2=res2n, anorm2=st["anorm2"] + a2 + b2n + damp * damp, rnorm=np.sqrt(phibar_n * phibar_n + res2n),
                      arnorm=alpha_n * abs(tau), xnorm=np.sqrt(st["xxnorm"] + zbar * zbar), bnorm=st["bnorm"])
            alpha, beta, a2, b2 = alpha_n, beta_n, a2n, b2n
            it += 1
            if iterates is not None:
                iterates.append(x.copy())
        stop = stop_test(st, atol, btol)
        return x, info(stop if stop else 7, it, st)


# ------------------------------------------------------------------ the six systems
def padded(A):
    """the m x n scipy matrix padded with empty rows or columns to max(m, n) square"""
    import scipy.sparse as sp

    m, n = A.shape
    s = max(m, n)
    A = A.tocoo()
    return sp.csr_matrix((A.data, (A.row, A.col)), shape=(s, s))


def pad_vector(v, s):
    out = np.zeros(s)
    out[:len(v)] = v
    return out


def convection(nx=NX, ny=NY):
    """5-point convection-diffusion stencil: diagonal 2.5 + 2.5, x-couplings -1 -+ 0.4, y-couplings -1: square, unsymmetric"""
    import scipy.sparse as sp

    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    west, east = (idx[:, 1:].ravel(), idx[:, :-1].ravel()), (idx[:, :-1].ravel(), idx[:, 1:].ravel())
    south, north = (idx[1:, :].ravel(), idx[:-1, :].ravel()), (idx[:-1, :].ravel(), idx[1:, :].ravel())
    r = np.concatenate([np.arange(n), west[0], east[0], south[0], north[0]])
    c = np.concatenate([np.arange(n), west[1], east[1], south[1], north[1]])
    v = np.concatenate([np.full(n, 5.0), np.full(len(west[0]), -1.4), np.full(len(east[0]), -0.6), -np.ones(len(south[0])),
                        -np.ones(len(north[0]))])
    return sp.csr_matrix((v, (r, c)), shape=(n, n))


def tall(seed=11):
    """1,440 x 600: random entries of density 0.008 in (-1, 1) plus an identity block on top: full column rank"""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    R = sp.random(N, M_COLS, density=0.008, random_state=rng, data_rvs=lambda k: rng.uniform(-1, 1, k))
    return (R + sp.eye(N, M_COLS)).tocsr()


def systems():
    """name -> dict(A: the rectangular matrix, Asq: padded square, b: padded, damp, shape).  (a) square unsymmetric, (b) tall and
    inconsistent, (c) the same damped, (d) its transpose (minimum norm), (e) a diagonal of 2 and -0.5, (f) zero b."""
    import scipy.sparse as sp

    rng = np.random.default_rng(5)
    out = {}
    A = convection()
    out["a"] = dict(A=A, b=A @ np.sin(np.arange(N) * 0.01) + 0.1, damp=0.0)
    T = tall()
    bt = rng.uniform(-1, 1, N)
    out["b"] = dict(A=T, b=bt, damp=0.0)
    out["c"] = dict(A=T, b=bt, damp=0.5)
    out["d"] = dict(A=T.T.tocsr(), b=rng.uniform(-1, 1, M_COLS), damp=0.0)
    D = sp.diags(np.where(np.arange(N) % 3 == 0, -0.5, 2.0)).tocsr()
    out["e"] = dict(A=D, b=rng.uniform(-1, 1, N), damp=0.0)
    out["f"] = dict(A=A, b=np.zeros(N), damp=0.0)
    for s in out.values():
        s["shape"] = s["A"].shape
        s["Asq"] = padded(s["A"])
        s["b"] = pad_vector(s["b"], N)
        assert s["Asq"].shape == (N, N)
    return out


# ------------------------------------------------------------------ exact cases for the step kernels
def fx_of(fr):
    """the dyadic Fraction as an Fx scalar"""
    fr = Fraction(fr)
    e = fr.denominator.bit_length() - 1
    assert fr.denominator == 1 << e, f"{fr} is not dyadic"
    return sc.dyadic(fr.numerator, e)


def planted_total(fr):
    """(integer total, e) of a slot whose sum is the dyadic Fraction fr"""
    f = fx_of(fr)
    return f.m, f.e


def lsqr_init_case(n, seed=0, grid=STEP_GRID):
    """U = b - t; partials of U.U and b.b (both squared: 13-bit numbers)"""
    c = sc.cg_init_case(n, False, seed + 90, grid)
    return {"in": {"b": c["in"]["b"], "t": c["in"]["q"]}, "out": {"u": c["out"]["r"]},
            "sums": {"beta2": c["sums"]["rr"], "bb": c["sums"]["bb"]}}


# cur -> beta_1 (start), alpha_1 (wstart): not powers of two, so the divisions are true ones
START = {0: Fraction(3, 2), 1: Fraction(5, 4)}


def lsqr_start_case(n, which, seed=0, grid=STEP_GRID):
    """V = t / beta_1, partials of V.V (V is squared: 13 bits); t = beta_1 V is built backwards"""
    rng = np.random.default_rng(seed)
    beta = START[which]
    v = Fx(odd_ints(rng, n, 13), 3)
    return {"in": {"t": _ex(fx_of(beta) * v)}, "beta2": beta * beta, "out": {"v": v}, "sums": {"alpha2": partials(v * v, grid, "lsqr_start alpha2")}}


def lsqr_wstart_case(n, which, seed=0):
    """w = V / alpha_1; V = alpha_1 w is built backwards, w is wide"""
    rng = np.random.default_rng(seed)
    alpha = START[which]
    w = Fx(odd_ints(rng, n, 26), 2)
    return {"in": {"v": _ex(fx_of(alpha) * w)}, "alpha2": alpha * alpha, "out": {"w": w}}


# cur -> (alpha, beta, beta') of ustep and (alpha, beta', -) of vstep: the divisor of t, and the ratio that multiplies the old vector
PAIR = {0: (Fraction(3, 2), Fraction(4)), 1: (Fraction(5, 4), Fraction(1, 2))}


def lsqr_pair_case(n, cur, seed=0, grid=STEP_GRID):
    """ustep and vstep are one formula: new = t / d - (d' / e) old, partials of new.new, where for ustep d = alpha, d' / e =
    alpha / beta and for vstep d = beta', d' / e = beta' / alpha.  d = PAIR[cur][0], e = PAIR[cur][1]; the ratio d / e is
    dyadic (3/8, 5/2).  new is squared (13 bits), old is wide; t = d (new + (d / e) old) is built backwards."""
    rng = np.random.default_rng(seed)
    d, e = PAIR[cur]
    ratio = fx_of(d / e)
    new = Fx(odd_ints(rng, n, 13), 3)
    old = Fx(odd_ints(rng, n, 26), 1)
    t = _ex(fx_of(d) * _ex(new + _ex(ratio * old)))
    return {"in": {"t": t, "old": old}, "d2": d * d, "e2": e * e, "out": {"new": new}, "sums": {"new2": partials(new * new, grid, "lsqr pair new2")}}


# The update's planted scalars.  cur -> rhobar, damp, beta', alpha', phibar, cs2, sn2, z, xxnorm, res2, anorm2, alpha^2:
# (rhobar, damp, rhobar1) and (rhobar1, beta', rho) are (3, 4, 5)-triples times powers of two (damp = 0 in the second set)
UPDATE = {
    0: dict(rhobar=Fraction(9, 4), damp=Fraction(3), beta_n=Fraction(5), alpha_n=Fraction(3, 2), phibar=Fraction(2), cs2=Fraction(-3, 4),
            sn2=Fraction(1, 2), z=Fraction(5, 8), xxnorm=Fraction(7, 4), res2=Fraction(3, 16), anorm2=Fraction(11, 2), alpha2=Fraction(9, 4)),
    1: dict(rhobar=Fraction(-3, 2), damp=Fraction(0), beta_n=Fraction(2), alpha_n=Fraction(5, 4), phibar=Fraction(-4), cs2=Fraction(1, 2),
            sn2=Fraction(-1, 2), z=Fraction(-3, 8), xxnorm=Fraction(1, 4), res2=Fraction(0), anorm2=Fraction(3), alpha2=Fraction(25, 16)),
}


def update_scalars(cur, lucky=None):
    """Every scalar of the update kernel for the planted set `cur`, restated operation by operation in fp64 as the kernel's source
    states them.  lucky: None, "beta" (beta' = 0: alpha' taken as 0) or "alpha" (alpha' = 0)."""
    p = {k: float(v) for k, v in UPDATE[cur].items()}
    beta2_n, alpha2_n = UPDATE[cur]["beta_n"] ** 2, UPDATE[cur]["alpha_n"] ** 2
    if lucky == "beta":
        beta2_n, alpha2_n = Fraction(0), Fraction(7)           # the alpha'^2 slot holds something stale: it must not be used
        p["beta_n"] = p["alpha_n"] = 0.0
    elif lucky == "alpha":
        alpha2_n = Fraction(0)
        p["alpha_n"] = 0.0
    f = np.float64
    rhobar, damp, beta_n, alpha_n, phibar = f(p["rhobar"]), f(p["damp"]), f(p["beta_n"]), f(p["alpha_n"]), f(p["phibar"])
    rhobar1 = f(math.hypot(rhobar, damp))
    assert Fraction(float(rhobar1)) ** 2 == UPDATE[cur]["rhobar"] ** 2 + UPDATE[cur]["damp"] ** 2, "hypot must be exact"
    cs1, sn1 = rhobar / rhobar1, damp / rhobar1
    psi, phibar1 = sn1 * phibar, cs1 * phibar
    rho = f(math.hypot(rhobar1, beta_n))
    assert Fraction(float(rho)) ** 2 == Fraction(float(rhobar1)) ** 2 + Fraction(float(beta_n)) ** 2, "hypot must be exact"
    cs, sn = rhobar1 / rho, beta_n / rho
    theta, phi, phibar_n = sn * alpha_n, cs * phibar1, sn * phibar1
    tau = sn * phi
    t1, t2 = phi / rho, theta / rho
    delta, gbar = f(p["sn2"]) * rho, -f(p["cs2"]) * rho
    fma = _fma
    rhs = fma(-delta, f(p["z"]), phi)
    zbar = rhs / gbar
    gamma = f(math.hypot(gbar, theta))
    zn = rhs / gamma
    res2n = fma(psi, psi, f(p["res2"]))
    new = dict(rhobar=-cs * alpha_n, phibar=phibar_n, cs2=gbar / gamma, sn2=theta / gamma, z=zn, xxnorm=fma(zn, zn, f(p["xxnorm"])), res2=res2n,
               anorm2=fma(damp, damp, (f(p["anorm2"]) + f(p["alpha2"])) + f(float(beta2_n))), rnorm=np.sqrt(fma(phibar_n, phibar_n, res2n)),
               arnorm=alpha_n * abs(tau), xnorm=np.sqrt(fma(zbar, zbar, f(p["xxnorm"]))), bnorm=777.0)
    state = {k: p[k] for k in ("rhobar", "phibar", "cs2", "sn2", "z", "xxnorm", "res2", "anorm2")}
    state.update(rnorm=1e300, arnorm=1e300, xnorm=0.0, bnorm=777.0)          # the update does not look at the first three
    return {"state": state, "state_new": {k: float(v) for k, v in new.items()}, "damp": float(damp), "t1": float(t1), "t2": float(t2),
            "alpha2": UPDATE[cur]["alpha2"], "beta2_n": beta2_n, "alpha2_n": alpha2_n, "alpha_n": Fraction(p["alpha_n"]), "gamma": float(gamma)}


def _fma(a, b, c):
    """a * b + c rounded once, for finite fp64 arguments, by exact rational arithmetic"""
    return np.float64(float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))))


def _fma_vec(scalar, m, units, addend):
    """fl(scalar * m + addend) per element, m and addend int64 arrays of 8 bits in units of 2^-units: ONE rounding of the exact
    sum, formed in rational arithmetic once per distinct (m, addend) pair (at most 2^16 of them) -> float64 array"""
    assert (np.abs(m) < 256).all() and (np.abs(addend) < 256).all()
    keys, inverse = np.unique((m + 256) * 512 + (addend + 256), return_inverse=True)
    s, unit = Fraction(float(scalar)), Fraction(1, 1 << units)
    table = np.array([float(s * (int(k) // 512 - 256) * unit + (int(k) % 512 - 256) * unit) for k in keys], dtype=np.float64)
    return table[inverse] if len(keys) else np.zeros(0)


def lsqr_update_case(n, cur, lucky=None, seed=0):
    """x' = fma(phi / rho, w, x); alpha' > 0: w' = fma(-theta / rho, w, V / alpha').  w, x and V / alpha' are 8-bit integers (in
    units of 1/4) so that each fma is one rounding of an exact int64 sum; V = alpha' (V / alpha') is built backwards."""
    rng = np.random.default_rng(seed)
    S = update_scalars(cur, lucky)
    w, x, va = odd_ints(rng, n, 8), odd_ints(rng, n, 8), odd_ints(rng, n, 8)
    out = {"x": _fma_vec(S["t1"], w, 2, x)}
    ins = {"w": Fx(w, 2), "x": Fx(x, 2)}
    if S["alpha2_n"] > 0 and S["beta2_n"] > 0:
        out["w"] = _fma_vec(-S["t2"], w, 2, va)
        ins["v"] = _ex(fx_of(S["alpha_n"]) * Fx(va, 2))
    return {"in": ins, "scalars": S, "out": out}
