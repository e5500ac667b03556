"""The helpers of solver_cases.py, checked without a GPU: the walk that chose the sizes, the integer reference against
fractions.Fraction on small inputs, and the exactness precondition of every construction at every size of the list."""
from fractions import Fraction

import numpy as np
import pytest

import solver_cases as sc


def test_the_size_list_covers_the_walk():
    seen = set()
    for n in sc.SIZES:
        seen |= sc.walk_profile(n, sc.STEP_GRID)
    assert seen >= sc.WANTED_PROFILES, sc.WANTED_PROFILES - seen
    assert sorted(sc.WALK) == sorted(sc.SIZES) and all(sc.asserted_walk(n) == sc.WALK[n] for n in sc.SIZES)
    # what the suite ran before this layer existed: one element per thread at most
    for n in (9900, 12000, 30000):
        assert sc.walk_profile(n, sc.solver_grid(n)) == {(0, 0), (0, 1)}, n
    assert sc.walk_profile(943695, sc.solver_grid(943695)) == {(1, 3), (2, 0)}
    assert sc.solver_grid(0) == 1 and sc.solver_grid(256) == 1 and sc.solver_grid(257) == 2 and sc.solver_grid(10 ** 7) == 512
    assert sc.S == 131072 and sc.solver_grid(sc.S) == sc.STEP_GRID


def test_walk_profile_against_the_loops_written_out():
    for n, grid in [(0, 1), (1, 1), (255, 1), (256, 1), (1025, 1), (2048, 2), (5000, 2), (7 * 512 + 1, 2), (4 * 512, 2)]:
        stride, seen = grid * sc.THREADS, set()
        for first in range(stride):
            i, unrolled, tail = first, 0, 0
            while i + 3 * stride < n:
                unrolled, i = unrolled + 1, i + 4 * stride
            while i < n:
                tail, i = tail + 1, i + stride
            seen.add((unrolled, tail))
        assert sc.walk_profile(n, grid) == seen, (n, grid)


def fr(v):
    return v.fractions()


def partials_by_hand(terms, grid):
    out = [Fraction(0)] * grid
    for i, t in enumerate(terms):
        out[(i % (grid * sc.THREADS)) // sc.THREADS] += t
    return out


def scalar(case, num, den):
    return Fraction(case["scalars"][num][0], case["scalars"][den][0])


def check(case, out, sums, grid):
    """out: name -> list of Fraction, sums: name -> list of Fraction terms; compared with the case's integer reference"""
    assert set(out) == set(case["out"]) and set(sums) == set(case["sums"])
    for k, want in out.items():
        assert fr(case["out"][k]) == want or (len(want) == 0 and len(case["out"][k].m) == 0), k
        assert [Fraction(v) for v in case["out"][k].f(k).tolist()] == want, k       # the float64 it is turned into
    for k, terms in sums.items():
        got = case["sums"][k]
        assert len(got.m) == grid and fr(got) == partials_by_hand(terms, grid), k
        assert [Fraction(v) for v in got.f(k).tolist()] == partials_by_hand(terms, grid), k


SMALL = [(0, 1), (1, 1), (257, 1), (700, 2), (2300, 2), (4 * 512 + 3, 2)]


@pytest.mark.parametrize("n,grid", SMALL)
@pytest.mark.parametrize("with_dinv", [False, True])
def test_reference_against_fractions(n, grid, with_dinv):
    d = fr(sc.inv_diag_fx(n)) if with_dinv else [Fraction(1)] * n
    assert all(v in [Fraction(2) ** k for k in range(-3, 4)] for v in d)

    for make in (sc.cg_init_case, sc.bicg_init_case):
        c = make(n, with_dinv, seed=3, grid=grid)
        b, q = fr(c["in"]["b"]), fr(c["in"]["q"])
        r = [bi - qi for bi, qi in zip(b, q)]
        z = [ri * di for ri, di in zip(r, d)]
        rr, bb = [ri * ri for ri in r], [bi * bi for bi in b]
        if make is sc.cg_init_case:
            check(c, {"r": r, "p": z}, {"rz": [ri * zi for ri, zi in zip(r, z)], "rr": rr, "bb": bb}, grid)
        else:
            check(c, {"r": r, "rh": r, "p": z}, {"rho": rr, "rr": rr, "bb": bb}, grid)

    c = sc.dot_case(n, seed=4, grid=grid)
    check(c, {}, {"pq": [a * b for a, b in zip(fr(c["in"]["p"]), fr(c["in"]["q"]))]}, grid)

    c = sc.bicg_dot2_case(n, seed=5, grid=grid)
    t, s = fr(c["in"]["t"]), fr(c["in"]["sv"])
    check(c, {}, {"ts": [a * b for a, b in zip(t, s)], "tt": [a * a for a in t]}, grid)

    for cur in (0, 1):
        c = sc.cg_update_case(n, cur, with_dinv, seed=6, grid=grid)
        alpha = scalar(c, "rz", "pq")
        assert alpha == Fraction(*{0: (3, 8), 1: (-5, 4)}[cur]) == fr(c["alpha"])[0]
        x = [xi + alpha * pi for xi, pi in zip(fr(c["in"]["x"]), fr(c["in"]["p"]))]
        r = [ri - alpha * qi for ri, qi in zip(fr(c["in"]["r"]), fr(c["in"]["q"]))]
        check(c, {"x": x, "r": r}, {"rz": [ri * ri * di for ri, di in zip(r, d)], "rr": [ri * ri for ri in r]}, grid)

        c = sc.cg_direction_case(n, cur, with_dinv, seed=7)
        beta = scalar(c, "rz_new", "rz")
        assert beta == fr(c["beta"])[0] and beta.denominator in (4, 8)
        check(c, {"p": [ri * di + beta * pi for ri, di, pi in zip(fr(c["in"]["r"]), d, fr(c["in"]["p"]))]}, {}, grid)

        c = sc.bicg_s_case(n, cur, with_dinv, seed=8, grid=grid)
        alpha = scalar(c, "rho", "rv")
        s = [ri - alpha * vi for ri, vi in zip(fr(c["in"]["r"]), fr(c["in"]["v"]))]
        check(c, {"sv": s, "sh": [si * di for si, di in zip(s, d)]}, {"ss": [si * si for si in s]}, grid)

        c = sc.bicg_direction_case(n, cur, with_dinv, seed=9)
        alpha, omega = scalar(c, "rho", "rv"), scalar(c, "ts", "tt")
        beta = scalar(c, "rho_new", "rho") * (alpha / omega)
        assert (alpha, omega) == (Fraction(3, 8), Fraction(3, 4)) and beta == fr(c["beta"])[0] == Fraction(sc.DIRECTION_RATIO[cur], 4)
        sv = c["scalars"]
        assert sc.bicg_beta_rounded(sv["rho_new"][0], sv["rho"][0], sv["rv"][0], sv["ts"][0], sv["tt"][0]) == float(beta)
        p = [ri * di + beta * (pi - omega * vi * di) for ri, vi, pi, di in zip(fr(c["in"]["r"]), fr(c["in"]["v"]), fr(c["in"]["p"]), d)]
        check(c, {"p": p}, {}, grid)

        if with_dinv:
            continue                # the two update kernels take no preconditioner
        c = sc.bicg_update_case(n, cur, seed=10, grid=grid)
        alpha, omega = scalar(c, "rho", "rv"), scalar(c, "ts", "tt")
        assert alpha == fr(c["alpha"])[0] and omega == fr(c["omega"])[0] == Fraction(*{0: (-5, 4), 1: (3, 4)}[cur])
        i = {k: fr(v) for k, v in c["in"].items()}
        x = [xi + alpha * pi + omega * hi for xi, pi, hi in zip(i["x"], i["p"], i["sh"])]
        r = [si - omega * ti for si, ti in zip(i["sv"], i["t"])]
        check(c, {"x": x, "r": r}, {"rho": [a * b for a, b in zip(i["rh"], r)], "rr": [a * a for a in r]}, grid)

        c = sc.bicg_half_case(n, cur, seed=11, grid=grid)
        alpha = scalar(c, "rho", "rv")
        i = {k: fr(v) for k, v in c["in"].items()}
        check(c, {"x": [xi + alpha * pi for xi, pi in zip(i["x"], i["p"])], "r": i["sv"]}, {"rr": [a * a for a in i["sv"]]}, grid)


def all_cases(n):
    """(kernel name, case) for every construction, with the preconditioner where the kernel takes one (the larger values)"""
    yield "cg_init", sc.cg_init_case(n, True)
    yield "cg_init", sc.cg_init_case(n, False)
    yield "cg_dot", sc.dot_case(n)
    yield "bicg_init", sc.bicg_init_case(n, True)
    yield "bicg_dot2", sc.bicg_dot2_case(n)
    for cur in (0, 1):
        yield "cg_update", sc.cg_update_case(n, cur, True)
        yield "cg_direction", sc.cg_direction_case(n, cur, True)
        yield "bicg_s", sc.bicg_s_case(n, cur, True)
        yield "bicg_update", sc.bicg_update_case(n, cur)
        yield "bicg_update_half", sc.bicg_half_case(n, cur)
        yield "bicg_direction", sc.bicg_direction_case(n, cur, True)


@pytest.mark.parametrize("n", sc.SIZES)
def test_precondition_and_width_at_every_size(n):
    """Building a case asserts that every value and every slot's magnitudes stay below EXACT_LIMIT; on top of that: every
    vector turns into float64 exactly, at least half of every vector read and of every product summed is wide (half
    rounded down where two vectors take turns by index), and the exceptions are the listed ones and no others."""
    for name, c in all_cases(n):
        for group, length in (("in", n), ("out", n), ("sums", sc.STEP_GRID)):
            for k, v in c[group].items():
                f = v.f(f"{name} {k}")
                assert len(f) == length and np.array_equal(f * 2.0 ** v.e, v.m.astype(np.float64)), (name, group, k)
        for k, v in c["products"].items():
            total = int(np.abs(v.m).sum())
            assert total < sc.EXACT_LIMIT, (name, k, total)
            assert (sc.significant_bits(v.m) > 24).sum() >= n // 2, (name, k, "products too narrow for fp32 to show")
        for k, v in c["in"].items():
            wide = int((sc.significant_bits(v.m) > 24).sum())
            if (name, k) in sc.NARROW_BY_NECESSITY:
                assert wide == 0, (name, k)
            else:
                assert wide >= n // 2, (name, k, wide)
        for num, den in c.get("scalars", {}).values():
            parts = sc.plant(num)
            assert int(parts.sum()) == num and den == 1 and (parts > 0).sum() > 100 and (parts < 0).sum() > 100
            assert len(set(np.abs(parts).tolist())) > 400 and np.abs(parts).max() > 1000 * np.median(np.abs(parts))


def test_planted_slots_and_probes():
    for total in (0, 3, -5 * sc.ODD_C, 2 ** 51 - 1):
        slot = sc.planted_slot(total, seed=total % 7)
        assert np.isnan(slot[sc.STEP_GRID:]).all() and len(slot) == sc.MAX_GRID
        assert sum(Fraction(v) for v in slot[:sc.STEP_GRID].tolist()) == total
        assert sc.in_order_sum(slot) == float(total) == sc.in_order_sum(slot[sc.STEP_GRID - 1::-1])
    assert sc.planted_slot(3, e=2)[:sc.STEP_GRID].sum() == 0.75
    for r, p in sc.DIVISION_PROBES:
        assert abs(r) < 2 ** 52 and abs(p) < 2 ** 52
        q = Fraction(r, p)
        assert q.denominator & (q.denominator - 1), "a dyadic quotient probes nothing"
        assert sc.rounded_quotient(r, p) == r / p == float(q) and Fraction(r / p) != q
    # three roundings, in the order of the source: not the same as one rounding of the exact value
    assert sc.bicg_beta_rounded(1, 3, 7, 11, 13) == (1 / 3) * ((3 / 7) / (11 / 13))


def test_width_helpers():
    assert sc.significant_bits([0, 1, -1, 6, 2 ** 24, 2 ** 24 + 1, -(2 ** 40 + 2 ** 10)]).tolist() == [0, 1, 1, 2, 1, 25, 31]
    assert sc.wide_share(np.array([2 ** 25 + 1, 3])) == 0.5
    v = sc.odd_ints(np.random.default_rng(0), 1000, 13)
    assert (v % 2 != 0).all() and (np.abs(v) >= 2 ** 12).all() and (np.abs(v) < 2 ** 13).all() and (v < 0).any() and (v > 0).any()
    assert (np.float32(v.astype(np.float64) ** 2) != v.astype(np.float64) ** 2).mean() > 0.5     # the squares do not fit fp32
