"""svds_next_kernel one launch at a time through ehyb_svds_next_step, bit for bit, on the inputs of svds_cases.py: every output is
one number in fp64, so the basis, the vector, every slot and every double of the tail is compared exactly (up to the sign of zero).
No tolerance appears in this file.

The guards are those of test_gpu_gmres_kernels.py, whose Bench is used: pads of sentinels behind the vector, behind the basis and
behind the tail; whatever the kernel does not name keeps its sentinel -- the other columns of the basis, R but for column j (left),
gt but for entry j + 1 (right), both Hessenberg copies; inputs come back unchanged; for an odd n the padding element of every
column holds the sentinel.

Sizes: 1, 2, 7, 8 and the three around 1024 (one workgroup's pairs are 512 elements: several workgroups, an odd tail), and
2 S + 3 = 262,147, one pair and one single element past a whole stride of the pair walk at 512 workgroups."""
import numpy as np
import pytest

import gmres_cases as gc
import solver_cases as sc
import svds_cases as sv
import test_gpu_gmres_kernels as gk
from solver_cases import MAX_GRID
from test_gpu_gmres_kernels import layout  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, BREAKDOWN = gk.RUNNING, gk.CONVERGED, gk.BREAKDOWN
ITERS = gk.ITERS
LEFT, RIGHT = sv.LEFT, sv.RIGHT
SMALL = [1, 2, 7, 8, 1023, 1024, 1025]
WRAP = 2 * sc.S + 3
assert WRAP > 2 * sc.STEP_GRID * sc.THREADS


def bench(E, L, n, side, j, seed, status=RUNNING, extra=1, **kw):
    """the basis with the written column and `extra` behind it, all sentinels; w; alpha^2 or beta^2 planted; h or g planted"""
    c = sv.next_case(n, side, j, seed=seed, **kw)
    b = gk.Bench(E, L, n, status=status).vec("w", c["w"]).basis([], c["column"] + 1 + extra)
    b.plant(L["slot_ww"], c["ww"], seed=3)
    b.tail("h_at", c["h"], offset=L["h_stride"])
    return c, b


def args(b, side, j):
    return (b.ld, "V", "w", "slots", side, j)


def written(L, c, norm=None):
    """what the launch writes into the tail when the multiply counts: column j of R with alpha (left), beta (right)"""
    norm = c["norm"] if norm is None else norm
    if c["side"] == LEFT:
        return {("r_at", c["j"] * L["r_stride"]): c["h"] + [norm]}
    return {("gt_at", c["j"] + 1): norm}


def cases():
    out = [(n, side, j) for n in SMALL for side in (LEFT, RIGHT) for j in sv.NEXT_J]
    return out + [(WRAP, side, j) for side in (LEFT, RIGHT) for j in (0, 8, 63)]


@pytest.mark.parametrize("n,side,j", cases(), ids=[f"n{n}-{'left' if s == LEFT else 'right'}-j{j}" for n, s, j in cases()])
def test_next_step(E, gpu, layout, n, side, j):  # noqa: F811
    """left: R[0 .. j-1, j] = h, R[j, j] = alpha, q_j = w / alpha; right: gt[j + 1] = beta, p_{j+1} = w / beta; the counter; the
    status stays"""
    c, b = bench(E, layout, n, side, j, n % 79 + j + 7 * side)
    b.call("ehyb_svds_next_step", *args(b, side, j))
    b.expect(f"next n={n} side={side} j={j}", columns={c["column"]: c["v"]}, tail=written(layout, c), flags=(RUNNING, ITERS + 1))


@pytest.mark.parametrize("n", SMALL + [WRAP])
def test_next_step_normalises_the_start_vector(E, gpu, layout, n):  # noqa: F811
    """side 1, j = -1: beta = 3/2 into gt[0], p_0 = w / beta; the counter stays"""
    c = sv.start_case(n, seed=n % 73)
    b = gk.Bench(E, layout, n).vec("w", c["w"]).basis([], 2)
    b.plant(layout["slot_ww"], c["ww"], seed=4)
    b.call("ehyb_svds_next_step", *args(b, RIGHT, -1))
    b.expect(f"start n={n}", columns={0: c["v"]}, tail={("gt_at", 0): c["norm"]})


@pytest.mark.parametrize("side", [LEFT, RIGHT], ids=["left", "right"])
def test_the_collapse_rule_on_both_sides_of_its_threshold(E, gpu, layout, side):  # noqa: F811
    """c_0 = 3 * 2^45 and w.w = 9: c.c + w.w rounds to 9 * 2^90, so w.w <= 2^-90 (c.c + w.w) holds with equality: the multiply counts,
    the column (left) and a zero norm are written, the status is converged, no vector moves.  One ulp more of c_0: w.w is below the
    threshold, the same.  One ulp less: c.c rounds to 9 * 2^90 - 2^41, w.w is above the threshold by 2^-49 of it, the step goes on."""
    L, n, j = layout, 257, 1 if side == LEFT else 0
    h0 = 3.0 * 2.0 ** 45
    above, below = float(np.nextafter(h0, np.inf)), float(np.nextafter(h0, 0.0))
    assert 9.0 <= 2.0 ** -90 * (h0 * h0 + 9.0) and 9.0 <= 2.0 ** -90 * (above * above + 9.0) and not 9.0 <= 2.0 ** -90 * (below * below + 9.0)
    for what, value in (("at equality", h0), ("one ulp inside", above)):
        c, b = bench(E, L, n, side, j, 5, k=0, h0=value)
        assert c["norm"] == 3.0 and c["h"] == [value]
        b.call("ehyb_svds_next_step", *args(b, side, j))
        b.expect(f"collapse {what}", tail=written(L, c, norm=0.0), flags=(CONVERGED, ITERS + 1))
    c, b = bench(E, L, n, side, j, 5, k=0, h0=below)
    b.call("ehyb_svds_next_step", *args(b, side, j))
    b.expect("one ulp outside", columns={c["column"]: c["v"]}, tail=written(L, c), flags=(RUNNING, ITERS + 1))
    # w.w = 0 behind eight columns: a collapse whatever the coefficients hold
    c, b = bench(E, L, n, side, 8, 6)
    b.slot(L["slot_ww"], sc.planted_slot(0, seed=2))
    b.call("ehyb_svds_next_step", *args(b, side, 8))
    b.expect("w.w = 0", tail=written(L, c, norm=0.0), flags=(CONVERGED, ITERS + 1))


def test_a_zero_matrix_collapses_in_the_first_left_half(E, gpu, layout):  # noqa: F811
    """left, j = 0: no coefficients, w.w = 0 <= 2^-90 * 0: R[0, 0] = 0, the multiply counts, converged"""
    L = layout
    c, b = bench(E, L, 257, LEFT, 0, 2)
    b.slot(L["slot_ww"], sc.planted_slot(0, seed=1))
    b.call("ehyb_svds_next_step", *args(b, LEFT, 0))
    b.expect("A p_0 = 0", tail=written(L, c, norm=0.0), flags=(CONVERGED, ITERS + 1))


def test_next_breaks_down_on_a_non_finite_quantity(E, gpu, layout):  # noqa: F811
    """a NaN or an infinity in h (left) or g (right), a NaN in w.w: the status, and nothing else -- the basis and the tail keep their
    sentinels, the counter stays.  At the start: a zero or non-finite norm."""
    L, n, j = layout, 257, 7
    nan_slot = sc.planted_slot(0, seed=1) + np.where(np.arange(MAX_GRID) == 3, np.nan, 0.0)
    for side in (LEFT, RIGHT):
        for what in ("nan-c", "inf-c", "nan-ww", "last-c"):
            c, b = bench(E, L, n, side, j, 5)
            if what == "nan-ww":
                b.slot(L["slot_ww"], nan_slot)
            else:                                             # "last-c": the last coefficient the side reads (h_{j-1}, g_j)
                b.tail("h_at", np.inf if what == "inf-c" else np.nan, offset=L["h_stride"] + (c["count"] - 1 if what == "last-c" else 2))
            b.call("ehyb_svds_next_step", *args(b, side, j))
            b.expect(f"breakdown {what} side {side}", flags=(BREAKDOWN, ITERS))
    # the left half does not read h_j: a NaN there (the right half's g_j of the step before) is not its business
    c, b = bench(E, L, n, LEFT, j, 5)
    b.tail("h_at", np.nan, offset=L["h_stride"] + j)
    b.call("ehyb_svds_next_step", *args(b, LEFT, j))
    after = b.host["slots"]
    b.expect("h_j is not read by the left half", columns={c["column"]: c["v"]}, tail=written(L, c), flags=(RUNNING, ITERS + 1))
    assert np.isnan(after[b.tail_at + L["h_at"] + L["h_stride"] + j])
    for what, slot in (("zero", sc.planted_slot(0, seed=2)), ("nan", nan_slot)):
        c = sv.start_case(n, seed=1)
        b = gk.Bench(E, L, n).vec("w", c["w"]).basis([], 1).slot(L["slot_ww"], slot)
        b.call("ehyb_svds_next_step", *args(b, RIGHT, -1))
        b.expect(f"start vector with a {what} norm", flags=(BREAKDOWN, ITERS))


@pytest.mark.parametrize("status", [CONVERGED, BREAKDOWN], ids=["converged", "breakdown"])
def test_next_returns_at_once_when_the_status_is_set(E, gpu, layout, status):  # noqa: F811
    """the inputs of the value tests, on which the step would write: with the status set nothing moves"""
    L = layout
    for n in (257, WRAP):
        for side in (LEFT, RIGHT):
            c, b = bench(E, L, n, side, 8, 6, status=status)
            b.call("ehyb_svds_next_step", *args(b, side, 8))
            b.expect(f"next side {side} with status {status}")
        c = sv.start_case(n, seed=2)
        b = gk.Bench(E, L, n, status=status).vec("w", c["w"]).basis([], 1).plant(L["slot_ww"], c["ww"], seed=4)
        b.call("ehyb_svds_next_step", *args(b, RIGHT, -1))
        b.expect(f"start with status {status}")
