"""What ehyb_bilu launches, one launch at a time.

The apply (ehyb_bic_apply_kernel on the streams of an L / U pair) on raw objects (ehyb_bilu_create_raw), bit for bit against the
exact solve of bilu_cases.exact_apply.  The data are dyadic -- the entries of L and U in +-{1/2, 1, 2}, 1 / u_ii powers of two
(of either sign), r small integers, every row's terms checked by exact_apply to add up below 2^53 units -- so the exact solve is
the only right answer (up to the sign of a zero) whatever the order of a sum and whether or not a product is fused.  Block
lengths 1, 2, round the wave, 1025 and the LDS ceiling, several blocks a launch, levels from 1 to `rows`, rows of 0, 1, 63, 64, 65
and 200 entries in either triangle independently of the other, k = 1 .. max_k and one more with a frozen column, padded leading
dimensions.  With U = L^T and equal diagonals the result is Bic.raw's apply bit for bit: the stream builder did not change IC.

The two GMRES launches ehyb_gmres_bilu adds -- the back substitution writing the combination instead of x, and x += z -- through
ehyb_bilu_gmres_combine_step / _add_step with the bench of test_gpu_gmres_kernels.py: every vector, its pad, every slot and the tail
compared exactly."""
import numpy as np
import pytest

import bic_cases as bc
import bilu_cases as lc
import gmres_cases as gc
from solver_cases import SENTINEL
from test_gpu_gmres_kernels import ITERS, Bench, layout  # noqa: F401 (layout: a fixture)

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def equal(z, want):
    """as numbers: the exact solve knows no sign of zero, the device's (0 - 0) * dinv has one"""
    return z.shape == want.shape and np.array_equal(z, want)


def check(E, case, R, ld=None, what="", **kw):
    """one object, two launches: both the exact result; -> the object"""
    f = E.Bilu.raw(*case)
    want = lc.exact_apply(*case, R)
    z = f.apply(R, ld=ld, **kw)
    pad = f.last_pad
    again = f.apply(R, ld=ld, **kw)
    nbytes, entries, threads = f.stream_info
    g = lc.from_library(f)
    print(f"{what}: n {f.n}, {f.blocks} blocks, levels forward {g['level_f'].max() + 1} backward {g['level_b'].max() + 1}, max_k {f.max_k}, {threads} threads, "
          f"{entries} entries in {nbytes} bytes; max |z| {np.abs(want).max():.3g}")
    assert entries == len(case[2]) + len(case[5])
    assert equal(z, want), (what, int((z != want).sum()), np.flatnonzero((z != want).ravel())[:5])
    assert same_bits(again, z), what
    assert np.isnan(pad).all(), "nothing is written between the columns"
    return f


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 1025])
def test_one_block(E, gpu, rows):
    rng = np.random.default_rng(rows)
    case = lc.staged_pair(rng, [rows], per_row_l=2, per_row_u=3)
    f = check(E, case, lc.small_ints(rng, rows), what=f"one block of {rows} rows")
    assert f.max_k == 4 and f.levels <= 5


def test_the_lds_ceiling(E, gpu):
    """20480 rows: 160 KiB of dynamic LDS, one column a launch.  L couples every row to the one four before it and U to the one
    four behind it, in stages of 5: short chains, every row touched in both directions."""
    n = lc.MAX_BLOCK
    rng = np.random.default_rng(1)
    case = lc.staged_pair(rng, [n], per_row_l=1, per_row_u=1, reach=4)
    R = lc.small_ints(rng, (2, n), bits=6)
    f = check(E, case, R, what="the LDS ceiling, k = 2 in two passes")
    assert f.max_k == 1 and f.stream_info[2] == 1024 and len(case[2]) > n // 2 and len(case[5]) > n // 2


@pytest.mark.parametrize("lower,upper", [(True, True), (True, False), (False, True)], ids=["both", "lower", "upper"])
def test_a_chain_of_as_many_levels_as_rows(E, gpu, lower, upper):
    """bidiagonal: every row waits for its neighbour -- 300 levels of one row each, in both directions or in one (the other
    triangle empty: one level)"""
    n = 300
    rng = np.random.default_rng(2)
    chain_l = (np.concatenate([[0], np.arange(n)]).astype(np.int64), np.arange(n - 1, dtype=np.int32), rng.choice([-1.0, 1.0], n - 1))
    chain_u = (np.concatenate([np.arange(n), [n - 1]]).astype(np.int64), np.arange(1, n, dtype=np.int32), rng.choice([-1.0, 1.0], n - 1))
    udinv = 2.0 ** (np.array([1, -1, 0])[np.arange(n) % 3])        # (the products along the chain stay near 1)
    case = (np.array([0, n]), *(chain_l if lower else lc.empty_triangle(n)), *(chain_u if upper else lc.empty_triangle(n)), udinv)
    f = check(E, case, lc.small_ints(rng, (3, n)), what="a chain")
    assert f.levels == 300
    assert np.array_equal(f.array("level_f"), np.arange(n) if lower else np.zeros(n)) and np.array_equal(f.array("level_b"), np.arange(n)[::-1] if upper else np.zeros(n))


def long_rows_case(rng, lengths_l, lengths_u, pad=300):
    """one block: `pad` rows without entries, then one row per length of lengths_l reading that many of the first rows (L), and
    in front of another `pad` rows one row per length of lengths_u reading that many of the last rows (U).  Two levels a side."""
    nl, nu = len(lengths_l), len(lengths_u)
    n = nu + pad + nl + pad
    lrp, lcols, urp, ucols = [0], [], [0], []
    for p in range(n):
        if nu + pad <= p < nu + pad + nl:
            lcols += list(range(nu, nu + lengths_l[p - nu - pad]))          # among the rows nu .. nu + pad: no entries in L
        lrp.append(len(lcols))
        if p < nu:
            ucols += list(range(n - lengths_u[p], n))                       # among the last pad rows: no entries in U
        urp.append(len(ucols))
    lvals, uvals = rng.choice([-1.0, 1.0, 0.5, -2.0], len(lcols)), rng.choice([-1.0, 1.0, -0.5, 2.0], len(ucols))
    return (np.array([0, n]), np.array(lrp, dtype=np.int64), np.array(lcols, dtype=np.int32), lvals, np.array(urp, dtype=np.int64),
            np.array(ucols, dtype=np.int32), uvals, rng.choice([0.5, 1.0, -2.0], n))


@pytest.mark.parametrize("which", ["both", "lower", "upper"])
def test_rows_of_0_1_63_64_65_and_200_entries_in_either_triangle(E, gpu, which):
    """rows round the lane group and longer than any (200 entries: several passes of a 64-lane group), in L, in U, or in both, the
    other triangle's rows of the same positions empty"""
    rng = np.random.default_rng(8)
    lengths = [0, 1, 63, 64, 65, 200]
    case = long_rows_case(rng, lengths if which != "upper" else [0] * 6, lengths[::-1] if which != "lower" else [0] * 6)
    f = check(E, case, lc.small_ints(rng, (2, len(case[-1]))), what=f"long rows, {which}")
    g = lc.from_library(f)
    assert sorted(np.diff(g["l_row_ptr"]).tolist())[-6:] == (sorted(lengths) if which != "upper" else [0] * 6)
    assert sorted(np.diff(g["u_row_ptr"]).tolist())[-6:] == (sorted(lengths) if which != "lower" else [0] * 6)
    assert g["level_f"].max() == (1 if which != "upper" else 0) and g["level_b"].max() == (1 if which != "lower" else 0)


def test_700_blocks_of_mixed_lengths(E, gpu):
    """more workgroups than two rounds of the 256 CUs, launched most expensive first; lengths 1 .. 90 in no order"""
    rng = np.random.default_rng(5)
    lengths = rng.integers(1, 91, 700)
    lengths[[0, 350, 699]] = (1, 90, 2)
    case = lc.staged_pair(rng, lengths.tolist())
    n = int(lengths.sum())
    assert n % 64 != 0
    f = check(E, case, lc.small_ints(rng, (2, n)), what="700 blocks")
    assert f.blocks == 700 and f.stream_info[2] == 64


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_k_columns_with_padded_leading_dimensions(E, gpu, k):
    """ldr, ldz > n; k = 5 goes in passes of four and one; column j is the one-column apply of R[j] bit for bit"""
    rng = np.random.default_rng(6)
    lengths = [65, 130, 7, 300]
    n = sum(lengths)
    case = lc.staged_pair(rng, lengths, per_row_l=3, per_row_u=1)
    R = lc.small_ints(rng, (5, n))[:k]
    f = check(E, case, R, ld=n + 13, what=f"k = {k}")
    assert f.max_k == 4
    Z = f.apply(R, ld=n + 13)
    for j in range(k):
        assert same_bits(Z[j], f.apply(R[j])), j


def test_a_frozen_column_is_left_as_it_was(E, gpu):
    rng = np.random.default_rng(7)
    lengths = [65, 130, 7, 300]
    n = sum(lengths)
    case = lc.staged_pair(rng, lengths)
    f = E.Bilu.raw(*case)
    R = lc.small_ints(rng, (5, n))
    want = lc.exact_apply(*case, R)
    Z0 = rng.uniform(-1, 1, (5, n))
    for flags in ([1, 0, 1, 1, 0], [0, 0, 0, 0, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]):
        Z = f.apply(R, ld=n + 3, active=flags, Z0=Z0)
        for j, on in enumerate(flags):
            assert equal(Z[j], want[j]) if on else same_bits(Z[j], Z0[j]), (flags, j)
        assert np.isnan(f.last_pad).all()


@pytest.mark.parametrize("rows,max_k", [(5121, 3), (10241, 1)])
def test_the_block_lengths_that_lower_max_k(E, gpu, rows, max_k):
    """four columns in passes of max_k: a long block of short rows beside a short one"""
    rng = np.random.default_rng(rows)
    case = lc.staged_pair(rng, [rows, 77], per_row_l=1, per_row_u=1)
    f = check(E, case, lc.small_ints(rng, (4, rows + 77)), ld=rows + 80, what=f"a block of {rows} rows")
    assert f.max_k == max_k


@pytest.mark.parametrize("lengths", [[1], [64, 65, 2], [1025, 7, 300]], ids=["1", "64-65-2", "1025-7-300"])
def test_with_u_the_transpose_of_l_it_is_the_ic_apply(E, gpu, lengths):
    """U = L^T and equal diagonals (ones: ILU's forward solve does not scale, so only a unit diagonal makes the two the same
    operator): Bic.raw(L, ones) applies (L L^T)^-1 through the streams Bilu.raw(L, L^T, ones) builds, and gives the same bits, the
    same stream sizes and the same levels.  With another diagonal ILU scales in the backward solve alone: against the exact solve."""
    rng = np.random.default_rng(9)
    bp, rp, cols, vals, dinv = bc.staged_factor(rng, lengths)
    n = int(bp[-1])
    ut = lc.transpose_strict(bp, rp, cols, vals)
    R = lc.small_ints(rng, (3, n))
    ones = np.ones(n)
    ic, ilu = E.Bic.raw(bp, rp, cols, vals, ones), E.Bilu.raw(bp, rp, cols, vals, *ut, ones)
    z = ic.apply(R)
    assert same_bits(z, ilu.apply(R)) and equal(z, bc.exact_apply(bp, rp, cols, vals, ones, R))
    assert ic.stream_info == ilu.stream_info
    assert np.array_equal(ic.array("level_f"), ilu.array("level_f")) and np.array_equal(ic.array("level_b"), ilu.array("level_b"))
    # a diagonal: IC scales a row in both solves, ILU in the backward one alone
    ilu2 = E.Bilu.raw(bp, rp, cols, vals, *ut, dinv)
    assert equal(ilu2.apply(R), lc.exact_apply(bp, rp, cols, vals, *ut, dinv, R))


# ------------------------------------------------------------------ the two launches of ehyb_gmres_bilu's cycle end
ADD_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 131073]


@pytest.mark.parametrize("n", ADD_SIZES)
def test_add_step(E, gpu, layout, n):
    """x += z where the cycle counted a step, whatever the status; one rounding per element, so numpy's sum is the answer"""
    rng = np.random.default_rng(n)
    for status, J in ((0, 1), (1, 30), (2, 64)):
        z, x = rng.standard_normal(n) * 2.0 ** rng.integers(-30, 30, n), rng.standard_normal(n)
        b = Bench(E, layout, n, status=status, iters=ITERS + J, cycle=ITERS).vec("z", z).vec("x", x)
        b.call("ehyb_bilu_gmres_add_step", "z", "x", "slots")
        b.expect(f"add n={n} J={J}", {"x": x + z})


def test_add_without_a_counted_step_writes_nothing(E, gpu, layout):
    n = 257
    rng = np.random.default_rng(1)
    for iters, cycle in ((ITERS, ITERS), (ITERS, ITERS + 2), (ITERS + 65, ITERS)):
        b = Bench(E, layout, n, iters=iters, cycle=cycle).vec("z", rng.standard_normal(n)).vec("x", rng.standard_normal(n))
        b.call("ehyb_bilu_gmres_add_step", "z", "x", "slots")
        b.expect(f"add iters={iters} cycle={cycle}")


@pytest.mark.parametrize("J", [1, 9, 64])
@pytest.mark.parametrize("n", ADD_SIZES)
def test_combine_step(E, gpu, layout, n, J):
    """R y = g, comb = V y over the J steps counted since the cycle start: solve_x's case without inv_diag, whose x_new - x is the
    combination exactly (the case asserts every sum on the way exact)"""
    L = layout
    c = gc.solve_x_case(n, J, False, seed=n % 71 + J)
    comb = (c["x_new"] - c["x"]).f("comb")
    b = Bench(E, L, n, status=1, iters=ITERS + J, cycle=ITERS).vec("comb").basis(c["V"], J)
    b.tail("g_at", c["g"])
    for col in range(J):
        b.tail("r_at", [c["R"][i][col] for i in range(col + 1)], offset=col * L["r_stride"])
    b.call("ehyb_bilu_gmres_combine_step", b.ld, "V", "comb", "slots")
    b.expect(f"combine n={n} J={J}", {"comb": comb})


def test_combine_without_a_counted_step_writes_nothing(E, gpu, layout):
    n = 257
    c = gc.solve_x_case(n, 3, False, seed=1)
    b = Bench(E, layout, n, iters=ITERS, cycle=ITERS).vec("comb").basis(c["V"], 3)
    b.call("ehyb_bilu_gmres_combine_step", b.ld, "V", "comb", "slots")
    b.expect("combine without a step")
    assert (b.dev["comb"].download() == SENTINEL).all()
