"""Inputs for the four vector kernels of ehyb_minres.hip whose every output is ONE number in fp64 -- the counterpart of
solver_cases.py, built with its machinery (Fx scaled integers, planted partials, exact partial sums).  No tests here
(test_minres_cases.py, test_gpu_minres_kernels.py).

The scalars.  A kernel forms every scalar itself: sums from the 512 planted partials of a slot, the rotation from the planted
state copy.  They are chosen so that every quotient and every root is exact:
  beta^2 is a square times a power of four (9/4, 25/16), so beta = sqrt(beta^2) is 3/2 or 5/4 -- not a power of two: q / beta
    and M^-1 ra / beta are true divisions, and the vectors are built backwards (q = beta * (...)) so that they come out exact;
  z.q = beta^3 c, so that alpha = z.q / beta^2 = beta c and alpha / beta = c, a small dyadic (3/8, -5/4);
  beta_old makes beta / beta_old dyadic (3/4, 5/2); beta_old = 0 is the first iteration;
  the state (cs, sn, dbar) is dyadic and gives delta = cs dbar + sn alpha and gbar = sn dbar - cs alpha exactly.
Two kinds of rotation, because cs' = gbar / gamma and sn' = beta_new / gamma cannot both be dyadic unless one of them is 0:
  "last":  beta_new = 0, gamma = |gbar|, cs' = +-1, sn' = 0, phi = +-phibar.  Everything is dyadic: wide vectors, the whole
           update exact in integer arithmetic.  (It is also the update after which the next dot kernel must set "converged".)
  "triple": (gbar, beta_new, gamma) = (3, 4, 5) times a power of two.  gamma is an exact root, cs' = fl(3/5) and sn' = fl(4/5)
           are correctly rounded quotients of 53 bits, phi = cs' phibar with phibar a power of two.  x' = fma(phi, w', x) is then
           ONE rounding of phi w' + x: w' and x are kept to 8 bits so that the exact sum fits in an int64, whose conversion to
           fp64 is that rounding.  v, wa, wb and ra stay wide.
"""
import math
from fractions import Fraction

import numpy as np

import solver_cases as sc
from solver_cases import Fx, STEP_GRID, _ex, _z, dyadic, inv_diag_fx, odd_ints, partials

STATE = ("dbar", "eps", "phibar", "cs", "sn", "beta_old")


def fx_of(fr):
    """the dyadic Fraction as an Fx scalar"""
    fr = Fraction(fr)
    e = fr.denominator.bit_length() - 1
    assert fr.denominator == 1 << e, f"{fr} is not dyadic"
    return dyadic(fr.numerator, e)


def planted_total(fr):
    """(integer total, e) of a slot whose sum is the dyadic Fraction fr"""
    f = fx_of(fr)
    return f.m, f.e


# cur -> beta, c = alpha / beta, beta_old
LANCZOS = {0: (Fraction(3, 2), Fraction(3, 8), Fraction(2)), 1: (Fraction(5, 4), Fraction(-5, 4), Fraction(1, 2))}


def scalars_of(cur):
    beta, c, beta_old = LANCZOS[cur]
    return {"beta": beta, "beta2": beta * beta, "zq": beta ** 3 * c, "alpha": beta * c, "ab": c, "beta_old": beta_old, "bo": beta / beta_old}


def minres_init_case(n, with_dinv, seed=0, grid=STEP_GRID):
    """r = b - q, z = M^-1 r; partials of r.z and of b.M^-1 b"""
    c = sc.cg_init_case(n, with_dinv, seed + 70, grid)
    bb = c["in"]["b"] * _z(c["in"]["b"], c["dinv"])
    prod = {"beta2": c["products"]["rz"], "bb": bb}
    return {"in": c["in"], "dinv": c["dinv"], "out": {"r": c["out"]["r"], "z": c["out"]["p"]},
            "sums": {"beta2": c["sums"]["rz"], "bb": partials(bb, grid, "minres_init bb")}, "products": prod}


def minres_dot_case(n, seed=0, grid=STEP_GRID):
    c = sc.dot_case(n, seed + 71, grid)
    return {"in": {"z": c["in"]["p"], "q": c["in"]["q"]}, "dinv": None, "out": {}, "sums": {"zq": c["sums"]["pq"]},
            "products": {"zq": c["products"]["pq"]}}


def minres_lanczos_case(n, cur, with_dinv, first, seed=0, grid=STEP_GRID):
    """r_new = q / beta - (alpha / beta) ra - (beta / beta_old) rb over rb (first: no rb term, rb is an output only);
    z = M^-1 r_new; partials of r_new.z.  r_new is squared, so it holds 13-bit numbers; ra, rb and q are wide."""
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    S = scalars_of(cur)
    r_new = Fx(odd_ints(rng, n, 13), 3)
    ra, rb = Fx(odd_ints(rng, n, 26)), Fx(odd_ints(rng, n, 26), 1)
    t = r_new + _ex(fx_of(S["ab"]) * ra)                       # q / beta - (alpha / beta) ra, the inner fma
    if not first:
        _ex(r_new + _ex(fx_of(S["bo"]) * rb))                  # what the inner fma leaves
        t = _ex(t + _ex(fx_of(S["bo"]) * rb))
    q = _ex(fx_of(S["beta"]) * t)
    z = _z(r_new, dinv)
    prod = {"beta2_new": r_new * z}
    ins = {"q": q, "ra": ra}
    if not first:
        ins["rb"] = rb
    return {"in": ins, "dinv": dinv, "scalars": S, "first": first, "out": {"rb": r_new, "z": z},
            "sums": {"beta2_new": partials(prod["beta2_new"], grid, "minres_lanczos beta2_new")}, "products": prod}


# cur -> cs, sn, eps, phibar of the planted state copy; kind -> cur -> (gbar, beta_new)
ROTATION = {0: (Fraction(-3, 4), Fraction(1, 2), Fraction(5, 8), Fraction(1, 2)), 1: (Fraction(1, 2), Fraction(-1, 2), Fraction(-3, 8), Fraction(2))}
TARGET = {"last": {0: (Fraction(3, 2), Fraction(0)), 1: (Fraction(-5, 4), Fraction(0))},
          "triple": {0: (Fraction(3, 2), Fraction(2)), 1: (Fraction(-3), Fraction(4))}}


def rotation_of(cur, kind):
    """every scalar of the update kernel for (cur, kind): the planted ones and, restated step by step with the kernel's
    roundings, the ones it forms.  The planted ones are dyadic Fractions; cs_new, sn_new, phi and phibar_new are floats."""
    S = scalars_of(cur)
    cs, sn, eps, phibar = ROTATION[cur]
    gbar, beta_new = TARGET[kind][cur]
    alpha = S["alpha"]
    dbar = (gbar + cs * alpha) / sn
    delta = cs * dbar + sn * alpha
    g2 = gbar * gbar + beta_new * beta_new
    gamma = Fraction(math.isqrt(g2.numerator), math.isqrt(g2.denominator))
    assert gamma * gamma == g2 and sn * dbar - cs * alpha == gbar, "gamma must be an exact root"
    for v in (dbar, delta, gamma):
        fx_of(v)
    cs_new, sn_new = float(gbar) / float(gamma), float(beta_new) / float(gamma)         # IEEE divisions, as the kernel's
    phi, phibar_new = cs_new * float(phibar), sn_new * float(phibar)                    # phibar is a power of two: exact scalings
    assert phibar > 0 and phibar.numerator & (phibar.numerator - 1) == 0 and phibar.denominator & (phibar.denominator - 1) == 0
    S.update(cs=cs, sn=sn, eps=eps, phibar=phibar, dbar=dbar, gbar=gbar, beta_new=beta_new, beta2_new=beta_new * beta_new, delta=delta,
             gamma=gamma, cs_new=cs_new, sn_new=sn_new, phi=phi, phibar_new=phibar_new)
    S["state"] = {"dbar": float(dbar), "eps": float(eps), "phibar": float(phibar), "cs": float(cs), "sn": float(sn), "beta_old": 777.0}
    S["state_new"] = {"dbar": float(-cs * beta_new), "eps": float(sn * beta_new), "phibar": phibar_new, "cs": cs_new, "sn": sn_new,
                      "beta_old": float(S["beta"])}
    return S


def minres_update_case(n, cur, with_dinv, kind, seed=0):
    """v = M^-1 ra / beta; w_new = (v - eps wb - delta wa) / gamma over wb; x += phi w_new.  Built backwards from w_new:
    v = gamma w_new + eps wb + delta wa, ra = beta v / M^-1."""
    rng = np.random.default_rng(seed)
    dinv = inv_diag_fx(n) if with_dinv else None
    S = rotation_of(cur, kind)
    wa, wb = Fx(odd_ints(rng, n, 26)), Fx(odd_ints(rng, n, 26), 1)
    if kind == "last":
        w_new, x = Fx(odd_ints(rng, n, 26), 2), Fx(odd_ints(rng, n, 30))
        x_new = (x + _ex(fx_of(Fraction(S["phi"])) * w_new)).f("x")
    else:
        w_new, x = Fx(odd_ints(rng, n, 8)), Fx(odd_ints(rng, n, 8))
        # phi = m * 2^-e with m of 53 bits; phi w' + x as an int64 in units of 2^-e, then ONE rounding: the conversion
        m, e = Fraction(S["phi"]).numerator, Fraction(S["phi"]).denominator.bit_length() - 1
        assert Fraction(S["phi"]).denominator == 1 << e and abs(m) < 2 ** 53 and e <= 54
        total = w_new.m * np.int64(m) + x.m * (np.int64(1) << e)
        assert abs(m) * 255 + (255 << e) < 2 ** 63
        x_new = np.ldexp(total.astype(np.float64), -e)
    t = _ex(fx_of(S["gamma"]) * w_new)                             # the numerator of w_new
    t = _ex(t + _ex(fx_of(S["delta"]) * wa))                       # ... before the delta fma
    v = _ex(t + _ex(fx_of(S["eps"]) * wb))
    ra = _ex(fx_of(S["beta"]) * v)
    if dinv is not None:
        ra = _ex(ra * Fx(64 // dinv.m, 3))                         # / M^-1: the powers of two 2^3 .. 2^-3
        _ex(ra * dinv)
    return {"in": {"ra": ra, "wa": wa, "wb": wb, "x": x}, "dinv": dinv, "scalars": S, "kind": kind,
            "out": {"wb": w_new, "x": x_new}, "sums": {}, "products": {}}
