"""ehyb_bic_apply_kernel one launch at a time, on raw objects (ehyb_bic_create_raw), bit for bit against the exact solve of
bic_cases.exact_apply.  The data are dyadic -- dinv powers of two, the entries of L and r small integers, every row's terms
checked by exact_apply to add up below 2^53 units -- so the exact solve is the only right answer whatever the order of a sum and
whether or not a product is fused.  Block lengths round the wave and the workgroup, the LDS ceiling, a chain of 300 levels, a
level wider than the workgroup feeding one row longer than any lane group, an empty L, more blocks than two rounds of the 256
CUs, k = 1 .. 5 with padded leading dimensions, an inactive column, and the block lengths at which ehyb_bic_max_k falls to 3, 2
and 1.  Every launch is compared with the exact result and with a second launch."""
import numpy as np
import pytest

import bic_cases as bc

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check(E, factor, R, ld=None, what="", **kw):
    """one object, two launches: both the exact result; -> the object"""
    bp, rp, cols, vals, dinv = factor
    f = E.Bic.raw(bp, rp, cols, vals, dinv)
    want = bc.exact_apply(bp, rp, cols, vals, dinv, R)
    z = f.apply(R, ld=ld, **kw)
    pad = f.last_pad
    again = f.apply(R, ld=ld, **kw)
    nbytes, entries, threads = f.stream_info
    print(f"{what}: n {f.n}, {f.blocks} blocks, {f.levels} levels, max_k {f.max_k}, {threads} threads, {entries} entries in {nbytes} bytes; "
          f"max |z| {np.abs(want).max():.3g}")
    assert entries == 2 * len(cols)
    assert same_bits(z, want), (what, int((z != want).sum()), np.flatnonzero((z != want).ravel())[:5])
    assert same_bits(again, want), what
    assert np.isnan(pad).all(), "nothing is written between the columns"
    return f


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1025])
def test_one_block(E, gpu, rows):
    rng = np.random.default_rng(rows)
    factor = bc.staged_factor(rng, [rows])
    f = check(E, factor, bc.small_ints(rng, rows), what=f"one block of {rows} rows")
    assert f.max_k == 4 and f.levels <= 5


def test_the_lds_ceiling(E, gpu):
    """20480 rows: 160 KiB of dynamic LDS, one column a launch; L is diagonal, so every row only scales"""
    n = bc.MAX_BLOCK
    rng = np.random.default_rng(1)
    dinv = 2.0 ** rng.integers(-3, 4, n)
    factor = (np.array([0, n]), np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), dinv)
    R = bc.small_ints(rng, (2, n), bits=10)
    f = check(E, factor, R, what="the LDS ceiling, k = 2 in two passes")
    assert f.max_k == 1 and f.levels == 1 and f.stream_info[2] == 1024
    assert same_bits(f.apply(R[1]), R[1] * dinv * dinv)


def test_a_chain_of_300_levels(E, gpu):
    """bidiagonal: every row waits for the one before it, forward and backward: 300 levels of one row each"""
    n = 300
    rng = np.random.default_rng(2)
    rp = np.concatenate([[0], np.arange(n)]).astype(np.int64)
    cols = np.arange(n - 1, dtype=np.int32)
    vals = rng.choice([-1.0, 1.0], n - 1)
    dinv = 2.0 ** (np.array([1, -1, 0])[np.arange(n) % 3])        # (the products along the chain stay near 1)
    f = check(E, (np.array([0, n]), rp, cols, vals, dinv), bc.small_ints(rng, (3, n)), what="a chain")
    assert f.levels == 300 and np.array_equal(f.array("level_f"), np.arange(n)) and np.array_equal(f.array("level_b"), np.arange(n)[::-1])


def test_a_level_wider_than_the_workgroup_and_a_row_longer_than_any_group(E, gpu):
    """2500 independent rows, then one row that depends on all of them: forward a level of 2500 rows in several rounds and a row
    of 2500 entries summed by 64 lanes in 40 passes; backward the same entries as a column, one entry per row"""
    w = 2500
    n = w + 1
    rng = np.random.default_rng(3)
    rp = np.concatenate([np.zeros(n, dtype=np.int64), [w]])
    cols = np.arange(w, dtype=np.int32)
    vals = rng.choice([-3.0, -1.0, 1.0, 3.0], w)
    dinv = 2.0 ** rng.integers(-1, 2, n)
    f = check(E, (np.array([0, n]), rp, cols, vals, dinv), bc.small_ints(rng, (4, n)), what="a wide level and a long row")
    assert f.levels == 2 and f.stream_info[2] < w and f.max_k == 4


def test_an_empty_factor(E, gpu):
    """no entries at all: every row at level 0, in three blocks; n is not a multiple of 64"""
    rng = np.random.default_rng(4)
    n = 64 + 65 + 200
    dinv = 2.0 ** rng.integers(-2, 3, n)
    factor = (np.array([0, 64, 129, n]), np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), dinv)
    f = check(E, factor, bc.small_ints(rng, n), what="an empty L")
    assert f.levels == 1 and not f.array("level_f").any() and not f.array("level_b").any()


def test_700_blocks_of_mixed_lengths(E, gpu):
    """more workgroups than two rounds of the 256 CUs, launched most expensive first; lengths 1 .. 90 in no order"""
    rng = np.random.default_rng(5)
    lengths = rng.integers(1, 91, 700)
    lengths[[0, 350, 699]] = (1, 90, 2)
    factor = bc.staged_factor(rng, lengths.tolist())
    n = int(lengths.sum())
    assert n % 64 != 0
    f = check(E, factor, bc.small_ints(rng, (2, n)), what="700 blocks")
    assert f.blocks == 700 and f.stream_info[2] == 64


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_k_columns_with_padded_leading_dimensions(E, gpu, k):
    """ldr, ldz > n; k = 5 goes in passes of four and one; column j is the one-column apply of R[j] bit for bit"""
    rng = np.random.default_rng(6)
    lengths = [65, 130, 7, 300]
    n = sum(lengths)
    assert n % 64 != 0
    factor = bc.staged_factor(rng, lengths)
    R = bc.small_ints(rng, (5, n))[:k]
    f = check(E, factor, R, ld=n + 13, what=f"k = {k}")
    assert f.max_k == 4
    Z = f.apply(R, ld=n + 13)
    for j in range(k):
        assert same_bits(Z[j], f.apply(R[j])), j


def test_an_inactive_column_is_left_as_it_was(E, gpu):
    rng = np.random.default_rng(7)
    lengths = [65, 130, 7, 300]
    n = sum(lengths)
    factor = bc.staged_factor(rng, lengths)
    f = E.Bic.raw(*factor)
    R = bc.small_ints(rng, (5, n))
    want = bc.exact_apply(*factor, R)
    Z0 = rng.uniform(-1, 1, (5, n))
    for flags in ([1, 0, 1, 1, 0], [0, 0, 0, 0, 1], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]):
        Z = f.apply(R, ld=n + 3, active=flags, Z0=Z0)
        for j, on in enumerate(flags):
            assert same_bits(Z[j], want[j] if on else Z0[j]), (flags, j)
        assert np.isnan(f.last_pad).all()


@pytest.mark.parametrize("rows,max_k", [(5121, 3), (6827, 2), (10241, 1)])
def test_the_block_lengths_that_lower_max_k(E, gpu, rows, max_k):
    """four columns in passes of max_k: a long block of short rows beside a short one"""
    rng = np.random.default_rng(rows)
    factor = bc.staged_factor(rng, [rows, 77], per_row=1)
    f = check(E, factor, bc.small_ints(rng, (4, rows + 77)), ld=rows + 80, what=f"a block of {rows} rows")
    assert f.max_k == max_k
