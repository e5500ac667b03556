"""gmres_cases.py is self-consistent: plain fp64 arithmetic on the cases' inputs -- in the kernels' order and in another one, fused
or not makes no difference to exact values -- gives the cases' outputs bit for bit, the partials have the layout of the pair
walk, and the vectors a kernel reads are wide where the arithmetic allows it."""
from fractions import Fraction

import numpy as np
import pytest

import gmres_cases as gc
import solver_cases as sc
from solver_cases import S, STEP_GRID, THREADS

SMALL = [0, 1, 65, 257, 2 * 512 + 3]


def test_sizes_and_counts_cover_the_walk_and_the_register_groups():
    assert {0, 1, 63, 64, 65, 255, 256, 257, 131073} <= set(gc.SIZES) and S + 1 == 131073
    assert max(gc.SIZES) > 2 * S and max(gc.SIZES) % 2 == 1            # a second trip of the pair walk, and a pair of one
    assert gc.COUNTS == [1, 2, 8, 9, 31, 65]


def test_pair_partials_is_the_pair_walk():
    n, grid = 2 * 3 * THREADS * 2 + 5, 3
    terms = sc.Fx(np.arange(1, n + 1, dtype=np.int64))
    want = np.zeros(grid, dtype=np.int64)
    stride = grid * THREADS
    for blk in range(grid):
        for t in range(THREADS):
            p = blk * THREADS + t
            while 2 * p < n:
                want[blk] += terms.m[2 * p] + (terms.m[2 * p + 1] if 2 * p + 1 < n else 0)
                p += stride
    assert np.array_equal(gc.pair_partials(terms, grid).m, want)


@pytest.mark.parametrize("n", SMALL)
def test_dots_and_update(n):
    for count in (1, 9):
        c = gc.dots_case(n, count, seed=n)
        w = c["w"].f("w")
        for v, part in zip(c["V"], c["sums"]):
            prod = v.f("v") * w
            assert float(prod.sum()) == float(prod[::-1].sum()) == float(part.f("c").sum())
        assert sc.wide_share(c["w"].m) == 1.0
        for last in (0, 1):
            c = gc.update_case(n, count, last, seed=n + 1)
            w = c["w"].f("w").copy()
            for ci, v in zip(c["c"], c["V"]):
                w = w - float(ci) * v.f("v")
            assert np.array_equal(w, c["w_new"].f("w_new"))
            if last:
                assert float((w * w).sum()) == float(c["ww"].f("ww").sum())


@pytest.mark.parametrize("j", [0, 1, 2, 9, 63])
def test_next(j):
    c = gc.next_case(65, j, True, seed=j)
    h = list(c["h"]) + [float(np.sqrt(float(c["ww"])))]
    assert h[-1] ** 2 == float(c["ww"]) and Fraction(h[-1]).numerator % 3 == 0      # an exact root, not a power of two
    for i in range(j):
        cs, sn = c["rot"][i]
        h[i], h[i + 1] = cs * h[i] + sn * h[i + 1], -sn * h[i] + cs * h[i + 1]
    gamma = float(np.hypot(h[j], h[j + 1]))
    assert h[:j] + [gamma] == c["R"] and (h[j] / gamma, h[j + 1] / gamma) == (c["cs"], c["sn"])
    assert (-c["sn"] * c["gt"], c["cs"] * c["gt"]) == (c["gt_next"], c["g"]) and c["rho"] == c["gt_next"] ** 2
    assert np.array_equal(c["w"].f("w") / h[j + 1], c["v"].f("v")) and sc.wide_share(c["v"].m) == 1.0
    assert np.array_equal(c["v"].f("v") * c["dinv"].f("dinv"), c["z"].f("z"))
    f = gc.first_case(65, True, seed=j)
    assert f["beta"] ** 2 == float(f["ww"]) and np.array_equal(f["w"].f("w") / f["beta"], f["v"].f("v"))


@pytest.mark.parametrize("J", [1, 2, 9, 64])
def test_solve_x(J):
    c = gc.solve_x_case(65, J, True, seed=J)
    R, g = np.array(c["R"]), list(c["g"])
    y = [0.0] * J
    for i in reversed(range(J)):
        y[i] = g[i] / R[i][i]
        for k in range(i):
            g[k] = g[k] - R[k][i] * y[i]
    assert y == [float(v) for v in c["y"]]
    acc = np.zeros(65)
    for yi, v in zip(y, c["V"]):
        acc = acc + yi * v.f("v")
    assert np.array_equal(c["x"].f("x") + acc * c["dinv"].f("dinv"), c["x_new"].f("x_new"))
    assert all(Fraction(R[i][i]).numerator not in (1, -1) or abs(R[i][i]) == 2.0 or abs(R[i][i]) == 0.5 for i in range(J))
    assert any(abs(Fraction(R[i][i]).numerator) != 1 for i in range(J))            # true divisions among them
