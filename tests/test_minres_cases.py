"""minres_cases.py checked on the CPU: the scalars a kernel forms from what a case plants are exactly the intended ones (restated
with Fractions and IEEE operations), every case's outputs are what the kernel's formulas give on its inputs -- evaluated in
rational arithmetic, with the one rounding of x' = fma(phi, w', x) made explicitly --, the sums are the sums of their terms,
and the width rule of solver_cases.py holds: what a kernel reads and sums cannot pass through fp32 unnoticed."""
import math
from fractions import Fraction

import numpy as np
import pytest

import minres_cases as mc
import solver_cases as sc

SMALL = [1, 257, 1000]


def fr(v):
    return v.fractions() if isinstance(v, sc.Fx) else [Fraction(float(a)) for a in v]


def test_the_planted_scalars_give_the_intended_quotients_and_roots():
    for cur in (0, 1):
        S = mc.scalars_of(cur)
        beta2, zq = float(S["beta2"]), float(S["zq"])
        assert Fraction(math.sqrt(beta2)) == S["beta"] and S["beta"].numerator not in (1, 2, 4)      # an exact root, not a power of two
        alpha = zq / beta2
        assert Fraction(alpha) == S["alpha"] and Fraction(alpha / math.sqrt(beta2)) == S["ab"]
        assert Fraction(math.sqrt(beta2) / float(S["beta_old"])) == S["bo"]
        for kind in ("last", "triple"):
            R = mc.rotation_of(cur, kind)
            cs, sn, dbar = float(R["cs"]), float(R["sn"]), float(R["dbar"])
            beta_new = math.sqrt(float(R["beta2_new"]))
            assert Fraction(beta_new) == R["beta_new"]
            assert Fraction(cs * dbar + sn * alpha) == R["delta"]
            gbar = sn * dbar - cs * alpha
            assert Fraction(gbar) == R["gbar"]
            gamma = math.sqrt(gbar * gbar + beta_new * beta_new)
            assert Fraction(gamma) == R["gamma"] and gamma > 0
            assert (gbar / gamma, beta_new / gamma) == (R["cs_new"], R["sn_new"])
            if kind == "triple":                                                                 # a Pythagorean triple, 3 : 4 : 5
                assert sorted(abs(Fraction(v) / R["gamma"] * 5) for v in (R["gbar"], R["beta_new"])) == [3, 4]
                assert Fraction(R["cs_new"]).denominator > 2 ** 40 and Fraction(R["phi"]).denominator > 2 ** 40
            else:
                assert R["beta_new"] == 0 and abs(R["cs_new"]) == 1.0 and R["sn_new"] == 0.0 and R["phibar_new"] == 0.0


@pytest.mark.parametrize("n", SMALL)
def test_init_and_dot_cases(n):
    for with_dinv in (False, True):
        c = mc.minres_init_case(n, with_dinv, seed=n)
        d = fr(c["dinv"]) if with_dinv else [Fraction(1)] * n
        b, q = fr(c["in"]["b"]), fr(c["in"]["q"])
        r = [bi - qi for bi, qi in zip(b, q)]
        assert r == fr(c["out"]["r"]) and [ri * di for ri, di in zip(r, d)] == fr(c["out"]["z"])
        assert sum(ri * ri * di for ri, di in zip(r, d)) == sum(fr(c["sums"]["beta2"]))
        assert sum(bi * bi * di for bi, di in zip(b, d)) == sum(fr(c["sums"]["bb"]))
    c = mc.minres_dot_case(n, seed=n)
    assert sum(a * b for a, b in zip(fr(c["in"]["z"]), fr(c["in"]["q"]))) == sum(fr(c["sums"]["zq"]))


@pytest.mark.parametrize("n", SMALL)
def test_lanczos_cases(n):
    for cur in (0, 1):
        for with_dinv in (False, True):
            for first in (False, True):
                c = mc.minres_lanczos_case(n, cur, with_dinv, first, seed=n + cur)
                S = c["scalars"]
                d = fr(c["dinv"]) if with_dinv else [Fraction(1)] * n
                q, ra = fr(c["in"]["q"]), fr(c["in"]["ra"])
                rb = [Fraction(0)] * n if first else fr(c["in"]["rb"])
                assert ("rb" in c["in"]) == (not first)
                rn = [qi / S["beta"] - S["ab"] * ai - (0 if first else S["bo"]) * bi for qi, ai, bi in zip(q, ra, rb)]
                assert rn == fr(c["out"]["rb"]) and [ri * di for ri, di in zip(rn, d)] == fr(c["out"]["z"])
                assert sum(ri * ri * di for ri, di in zip(rn, d)) == sum(fr(c["sums"]["beta2_new"]))


@pytest.mark.parametrize("n", SMALL)
def test_update_cases(n):
    for cur in (0, 1):
        for with_dinv in (False, True):
            for kind in ("last", "triple"):
                c = mc.minres_update_case(n, cur, with_dinv, kind, seed=n + cur)
                S = c["scalars"]
                d = fr(c["dinv"]) if with_dinv else [Fraction(1)] * n
                ra, wa, wb, x = (fr(c["in"][k]) for k in ("ra", "wa", "wb", "x"))
                wn = [(ri * di / S["beta"] - S["eps"] * bi - S["delta"] * ai) / S["gamma"] for ri, di, ai, bi in zip(ra, d, wa, wb)]
                assert wn == fr(c["out"]["wb"])
                exact = [Fraction(S["phi"]) * wi + xi for wi, xi in zip(wn, x)]
                assert [Fraction(float(v)) for v in exact] == fr(c["out"]["x"])                  # float(Fraction): correctly rounded
                if kind == "triple":
                    assert any(Fraction(float(v)) != v for v in exact) or n < 3, "the rounding of x' must be exercised"


@pytest.mark.parametrize("n", [S for S in sc.SIZES if S > 0])
def test_every_size_builds_and_keeps_the_width_rule(n):
    """building a case asserts its exactness (Fx.f, partials, _ex); here the width rule on top: every vector a kernel reads is
    wide (more than 24 significant bits) in at least half of its elements, or its products are -- but for the vectors whose
    square is summed, and the 8-bit w' and x of the triple update, where arithmetic forces it (the module docstrings)."""
    assert sc.asserted_walk(n)
    c = mc.minres_lanczos_case(n, n & 1, True, False, seed=n % 83)
    for name in ("q", "ra", "rb"):
        assert sc.wide_share(c["in"][name].m) >= 0.5, name
    assert sc.wide_share(c["products"]["beta2_new"].m) >= 0.5
    c = mc.minres_update_case(n, n & 1, True, "last", seed=n % 83)
    for name in ("ra", "wa", "wb", "x"):
        assert sc.wide_share(c["in"][name].m) >= 0.5, name
    assert sc.wide_share(c["out"]["wb"].m) >= 0.5
    c = mc.minres_update_case(n, n & 1, True, "triple", seed=n % 83)
    for name in ("ra", "wa", "wb"):
        assert sc.wide_share(c["in"][name].m) >= 0.5, name
    c = mc.minres_init_case(n, True, seed=n % 97)
    assert sc.wide_share(c["products"]["beta2"].m) >= 0.5 and sc.wide_share(c["products"]["bb"].m) >= 0.5
    c = mc.minres_dot_case(n, seed=n % 89)
    assert sc.wide_share(c["products"]["zq"].m) >= 0.5
