"""The exact integer cases of exact_cases.py moved over the whole fp64 range and mantissa width.

Multiplying by a power of two is exact.  An integer case (every a_ij and x_j an integer, every row's sum |a_ij x_j| < 2^52)
scaled by powers of two -- per matrix, per row or per column -- still has ONE correct fp64 product whatever the order of
summation, as long as every product and partial sum of a row is a multiple of one unit 2^e >= 2^-1074 and stays below 2^1023.
So does an integer case redrawn with as many mantissa bits as its longest row leaves room for.  Every kernel path must
reproduce these products bit for bit (assert_exact), which shows what the +-1..7 by 26-bit cases cannot: a lost low mantissa
bit, a subnormal flushed to zero, arithmetic that mixes rows of different magnitude (a difference of prefix sums, an
accumulator shared between rows, a fold that adds and later subtracts), and an infinity met before the end of a finite sum.

family() takes an integer case in the plan's numbering and returns (V', x', y'); y' is the int64 product scaled with np.ldexp,
never recomputed in floating point.  It asserts its own preconditions and refuses (ValueError) a case it cannot make exact.

  low          V 2^-537         x 2^-537      y 2^-1074    inputs normal; every product, partial sum and result subnormal
  low-x        V                x 2^-1074     y 2^-1074    subnormal x through windows, halos, gathers
  low-v        V 2^-1074        x             y 2^-1074    subnormal matrix values; pairing by value on subnormals
  high         V 2^485          x 2^486       y 2^971      all finite below 2^1023; no early infinity
  graded-sym   V_ij 2^(ri+rj)   x_j 2^-rj     y_i 2^ri     r in [-480, 480]: symmetric in value, neighbouring rows binades apart
  graded-rows  V_ij 2^ri        x             y_i 2^ri     r in [-900, 900]: the same for paths without pairs
  graded-low   V_ij 2^(ri+30)   x 2^-30       y_i 2^ri     r in [-1074, -1000]: subnormal and normal rows side by side
  wide-v       odd, b bits      +-1           int64        b = min(52, 51 - ceil(log2(longest row))): every mantissa bit of a value
  wide-x       +-1..7           odd, b-3 bits int64        every mantissa bit of x

r_i is a hash of the row index in the plan's numbering.
"""
import numpy as np
import scipy.sparse as sp

from exact_cases import EXACT_LIMIT, _hash, as_int, integer_values

FAMILIES = ("low", "low-x", "low-v", "high", "graded-sym", "graded-rows", "graded-low", "wide-v", "wide-x")
GRADED = ("graded-sym", "graded-rows", "graded-low")
MIN_UNIT = -1074             # 2^-1074: the smallest subnormal
MAX_EXP = 1023               # every |sum| must stay below 2^1023
MIN_WIDE_BITS = 28           # wide-x draws b - 3 bits: below 25 they would fit fp32's 24-bit mantissa and show nothing
COLUMN_EXPONENTS = (-1074, 0, 940, -511, -1074 + 52, 470, 0, -1000)   # ehyb_spmm, per column of X (columns_scaled)


def row_exponents(n, lo, hi, salt=77):
    """r_i in [lo, hi]: a deterministic hash of the row index."""
    h = _hash(np.arange(n), np.zeros(n, dtype=np.int64), salt)
    return (h % np.uint64(hi - lo + 1)).astype(np.int64) + lo


def _bits(m):
    """ceil(log2(m + 1)) of non-negative integers given as float64 below 2^53: the binade a magnitude m ends in (m < 2^bits)."""
    return np.frexp(np.asarray(m, dtype=np.float64))[1].astype(np.int64)


def _int_product(n, I, J, vi, xi):
    """(A x, |A| |x|) in int64, duplicates summed."""
    A = sp.csr_matrix((vi, (np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64))), shape=(n, len(xi)), dtype=np.int64)
    return A @ xi, abs(A) @ np.abs(xi)


def wide_bits(I, n):
    """b of the wide families for the longest row of the pattern; ValueError if that row leaves too few bits."""
    longest = int(np.bincount(np.asarray(I, dtype=np.int64), minlength=max(n, 1)).max()) if len(I) else 1
    b = min(52, 51 - int(np.ceil(np.log2(max(longest, 1)))))
    if b < MIN_WIDE_BITS:
        raise ValueError(f"longest row has {longest} entries: {b} bits per value left, fewer than {MIN_WIDE_BITS}")
    return b


def odd_integers(h, bits):
    """Odd integers of exactly `bits` bits (top and lowest bit set) with a sign, from 64-bit hashes."""
    assert 2 <= bits <= 52
    mag = (h >> np.uint64(64 - bits)) | (np.uint64(1) << np.uint64(bits - 1)) | np.uint64(1)
    sign = np.where((h >> np.uint64(3)) & np.uint64(1), -1, 1)
    return mag.astype(np.int64) * sign


def _scaled(ints, e):
    """ints * 2^e elementwise, asserting that nothing is lost: every result round-trips through ldexp(., -e)."""
    out = np.ldexp(ints.astype(np.float64), e)
    e = np.broadcast_to(e, out.shape)
    # (2^1074 is not an fp64 number: undo the shift in two exact halves)
    back = np.ldexp(np.ldexp(out, -(e // 2)), -(e - e // 2))
    if not (np.isfinite(out).all() and np.array_equal(back, ints.astype(np.float64))):
        raise ValueError("a scaled value does not round-trip: it left the fp64 range or lost a bit")
    return out


def family(name, n, I, J, V, x, y, symmetric=False, x_salt=0):
    """Integer case (I, J, V, x, exact y; the plan's numbering) -> (V', x', y') of family `name`.
    symmetric: the case is symmetric in value and wide-v must keep it so (values by a hash of (min, max)).
    x_salt: another draw of the x a wide family makes (several columns for one matrix)."""
    I = np.asarray(I, dtype=np.int64)
    J = np.asarray(J, dtype=np.int64)
    vi, xi, yi = as_int(V), as_int(x), as_int(y)
    if name not in FAMILIES:
        raise ValueError(f"unknown family {name!r}")
    zero, zx = np.zeros(n, dtype=np.int64), np.zeros(len(xi), dtype=np.int64)
    # exponents: e_v per entry, e_x per column, e_y per row; every product of row i has the unit 2^e_y[i]
    if name == "wide-v":
        b = wide_bits(I, n)
        a, c = (np.minimum(I, J), np.maximum(I, J)) if symmetric else (I, J)
        vi = odd_integers(_hash(a, c, 0x51D), b)
        xi = np.where(_hash(np.arange(len(xi)), np.zeros(len(xi), dtype=np.int64), 0xA11 + x_salt) & np.uint64(1), -1, 1).astype(np.int64)
        e_v, e_x, e_y = zero[I], zx, zero
    elif name == "wide-x":
        b = wide_bits(I, n)
        vi = as_int(integer_values(I, J, symmetric))
        xi = odd_integers(_hash(np.arange(len(xi)), np.zeros(len(xi), dtype=np.int64), 0xB22 + x_salt), b - 3)
        e_v, e_x, e_y = zero[I], zx, zero
    elif name == "low":
        e_v, e_x, e_y = zero[I] - 537, zx - 537, zero - 1074
    elif name == "low-x":
        e_v, e_x, e_y = zero[I], zx - 1074, zero - 1074
    elif name == "low-v":
        e_v, e_x, e_y = zero[I] - 1074, zx, zero - 1074
    elif name == "high":
        e_v, e_x, e_y = zero[I] + 485, zx + 486, zero + 971
    elif name == "graded-sym":
        if len(xi) != n:
            raise ValueError("graded-sym needs a square case")
        r = row_exponents(n, -480, 480)
        e_v, e_x, e_y = r[I] + r[J], -r, r
    elif name == "graded-rows":
        r = row_exponents(n, -900, 900)
        e_v, e_x, e_y = r[I], zx, r
    else:  # graded-low
        r = row_exponents(n, -1074, -1000)
        e_v, e_x, e_y = r[I] + 30, zx - 30, r
    # ---- preconditions
    y_int, mag = _int_product(n, I, J, vi, xi)
    if len(vi) and mag.max() >= EXACT_LIMIT:
        raise ValueError(f"row sum {float(mag.max()):.3e} too large for an exact fp64 product")
    if name.startswith("wide"):
        yi = y_int
    elif not np.array_equal(y_int, yi):
        raise ValueError("y is not the int64 product of V and x")
    assert np.array_equal(e_v + e_x[J], e_y[I]), "every product of a row must share the row's unit"
    if min(e_v.min(initial=0), e_x.min(initial=0), e_y.min(initial=0)) < MIN_UNIT:
        raise ValueError("a unit below 2^-1074")
    if n and (_bits(mag.astype(np.float64)) + e_y).max() > MAX_EXP:
        raise ValueError("a row's sum |a_ij x_j| reaches 2^1023")
    return _scaled(vi, e_v), _scaled(xi, e_x), _scaled(yi, e_y)


def columns_scaled(X, Y, exponents=COLUMN_EXPONENTS):
    """ehyb_spmm, per column: the matrix stays as it is, column j of the integer X is scaled by 2^e_j and so is its exact
    product Y_j.  One call then carries a subnormal column beside a near-overflow one."""
    X, Y = np.atleast_2d(X), np.atleast_2d(Y)
    e = np.resize(np.asarray(exponents, dtype=np.int64), len(X))
    for ej in e:
        # |y| <= sum |a x| < 2^52, and so is every partial sum: 2^(52 + e) must stay below 2^1023
        if 52 + ej > MAX_EXP or ej < MIN_UNIT:
            raise ValueError(f"column exponent {ej} leaves the fp64 range")
    Xs = np.stack([_scaled(as_int(xj), ej) for xj, ej in zip(X, e)])
    Ys = np.stack([_scaled(as_int(yj), ej) for yj, ej in zip(Y, e)])
    return Xs, Ys
