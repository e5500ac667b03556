"""The two vector kernels of the Chebyshev preconditioner one launch at a time, bit for bit (ehyb_cheb_start_step,
ehyb_cheb_step; K = 1), on the exact cases of cheb_cases.py: with and without inv_diag, with the r.z sum going to either
slot or nowhere (rz = -1: the slot array must come back untouched), at sizes that cover every profile of unrolled and tail
trips of the kernels' index walk.  Guards as in test_gpu_solver_kernels.py: PAD doubles of SENTINEL behind every vector, every
slot entry that is not written unchanged, inputs unchanged.  No tolerance appears in this file."""
import pytest

import cheb_cases as cc
from test_gpu_solver_kernels import Bench, cg_layout  # noqa: F401  (cg_layout: a fixture)

pytestmark = pytest.mark.gpu

COEF = cc.C0[0] / 2.0 ** cc.C0[1]
A, B = (num / 2.0 ** lg for num, lg in cc.A_B)


def test_the_coefficients_are_the_dyadic_ones():
    assert (COEF, A, B) == (0.375, 0.375, -1.25)


@pytest.mark.parametrize("n", cc.SIZES)
def test_cheb_start_step(E, gpu, cg_layout, n):  # noqa: F811
    cc.asserted_walk(n)
    L = cg_layout
    for with_dinv in (False, True):
        c = cc.start_case(n, with_dinv, seed=n % 97)
        assert c["coef"].f() == COEF
        for rz in (-1, 0, 1):
            b = Bench(E, n, L["slots"]).vecs(c["in"]).vec("d").vec("z")
            if with_dinv:
                b.vec("dinv", c["dinv"])
            b.call("ehyb_cheb_start_step", "r", "dinv" if with_dinv else None, COEF, "d", "z", "slots", rz)
            b.expect(f"cheb start n={n} inv_diag={with_dinv} rz={rz}", c["out"], {} if rz < 0 else {L["rz0"] + 2 * rz: c["sums"]["rz"]})


@pytest.mark.parametrize("n", cc.SIZES)
def test_cheb_step(E, gpu, cg_layout, n):  # noqa: F811
    cc.asserted_walk(n)
    L = cg_layout
    for with_dinv in (False, True):
        c = cc.step_case(n, with_dinv, seed=n % 89)
        assert (c["a"].f(), c["b"].f()) == (A, B)
        for rz in (-1, 0, 1):
            for in_place in ((False, True) if rz == (1 if with_dinv else -1) else (False,)):
                b = Bench(E, n, L["slots"]).vecs(c["in"])
                if not in_place:
                    b.vec("w_out")
                if with_dinv:
                    b.vec("dinv", c["dinv"])
                w_out = "w_in" if in_place else "w_out"
                b.call("ehyb_cheb_step", "w_in", "t", "dinv" if with_dinv else None, A, B, w_out, "d", "z", "r", "slots", rz)
                # r, t and (unless it is w_out) w_in come back unchanged: expect() compares every vector it was not given
                b.expect(f"cheb step n={n} inv_diag={with_dinv} rz={rz} in place={in_place}",
                         {w_out: c["out"]["w_out"], "d": c["out"]["d"], "z": c["out"]["z"]},
                         {} if rz < 0 else {L["rz0"] + 2 * rz: c["sums"]["rz"]})
