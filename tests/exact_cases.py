"""Integer matrices and vectors whose product is exact in fp64, for bit-for-bit checks of every kernel path.

If every a_ij and x_j is an integer and every row has sum_j |a_ij x_j| < 2^53, every partial sum of the row is an
integer below 2^53 and so exact in fp64, in any order: the product is ONE number, whatever the summation order,
the atomics or the LDS adds of a path.  Every path must then reproduce it bit for bit (np.array_equal; an empty
row may come out as -0.0).

x holds ODD integers of magnitude in [2^25, 2^26): fp32 cannot hold them, so a pass of x or of a product through
fp32 changes the result.  Matrix values are small (+-1..7) so that a matrix that is not symmetric still has
entries with a_ij == a_ji by accident -- what symmetric pair storage pairs by value (layout.cpp).
"""
import numpy as np

EXACT_LIMIT = 2.0 ** 52      # row sums of |a_ij x_j| must stay below 2^53; one bit of margin


def _hash(a, b, salt):
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    h = a * np.uint64(0x9E3779B97F4A7C15) ^ (b + np.uint64(salt)) * np.uint64(0xC2B2AE3D27D4EB4F)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0x94D049BB133111EB)
    h ^= h >> np.uint64(32)
    return h


def integer_values(I, J, symmetric, lo=1, hi=7, salt=0):
    """Deterministic non-zero integers, |v| in [lo, hi], from a hash of (i, j); symmetric: of (min, max), so that
    a_ij == a_ji wherever both are stored."""
    I = np.asarray(I, dtype=np.int64)
    J = np.asarray(J, dtype=np.int64)
    a, b = (np.minimum(I, J), np.maximum(I, J)) if symmetric else (I, J)
    h = _hash(a, b, salt)
    mag = (h % np.uint64(hi - lo + 1)).astype(np.int64) + lo
    sign = np.where((h >> np.uint64(40)) & np.uint64(1), -1, 1)
    return (sign * mag).astype(np.float64)


def integer_x(n, seed):
    """Odd integers with magnitude in [2^25, 2^26) and random sign (not representable in fp32)."""
    rng = np.random.default_rng(seed)
    mag = rng.integers(1 << 24, 1 << 25, n, dtype=np.int64) * 2 + 1
    return (mag * rng.choice(np.array([-1, 1], dtype=np.int64), n)).astype(np.float64)


def as_int(v):
    """float64 array of integers -> int64, asserting that it holds integers only."""
    v = np.asarray(v, dtype=np.float64)
    assert np.isfinite(v).all() and np.array_equal(v, np.round(v)) and (np.abs(v) < 2.0 ** 62).all()
    return v.astype(np.int64)


def exact_reference(n, I, J, V, x, O=None):
    """y = A x in int64, independent of the fp oracle; asserts the exactness precondition and returns float64.
    With O (the oracle module) also checks that the oracle's COO product gives the same vector bit for bit."""
    import scipy.sparse as sp

    I = np.asarray(I, dtype=np.int64)
    J = np.asarray(J, dtype=np.int64)
    vi, xi = as_int(V), as_int(x)
    A = sp.csr_matrix((vi, (I, J)), shape=(n, len(xi)), dtype=np.int64)     # duplicates summed, in int64
    mag = abs(A) @ np.abs(xi)
    assert len(vi) == 0 or mag.max() < EXACT_LIMIT, f"row sum {mag.max():.3e} too large for an exact fp64 product"
    y = (A @ xi).astype(np.float64)
    if O is not None:
        y_o = O.spmv_coo(n, I.astype(np.int32), J.astype(np.int32), V, x)
        assert np.array_equal(y_o, y), "the fp64 oracle is not exact on an integer input"
    return y


def value_class(y):
    """Per row: 0 finite, 1 NaN, 2 +inf, 3 -inf -- what a product with non-finite entries must reproduce exactly."""
    y = np.asarray(y, dtype=np.float64)
    c = np.zeros(len(y), dtype=np.int8)
    c[np.isnan(y)] = 1
    c[y == np.inf] = 2
    c[y == -np.inf] = 3
    return c


def nonfinite_reference(n, I, J, V, x):
    """y = A x where some V or x are non-finite: the class of every row (value_class) does not depend on the order
    of summation, and a finite row is the exact integer sum of its (all finite, integer) terms."""
    I = np.asarray(I, dtype=np.int64)
    J = np.asarray(J, dtype=np.int64)
    V = np.asarray(V, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        prod = V * x[J]
    nan = np.zeros(n, dtype=bool)
    pinf = np.zeros(n, dtype=bool)
    ninf = np.zeros(n, dtype=bool)
    np.logical_or.at(nan, I, np.isnan(prod))
    np.logical_or.at(pinf, I, prod == np.inf)
    np.logical_or.at(ninf, I, prod == -np.inf)
    fin = np.isfinite(prod)
    y = exact_reference(n, I[fin], J[fin], V[fin], np.where(np.isfinite(x), x, 0.0))
    y[pinf] = np.inf
    y[ninf] = -np.inf
    y[nan | (pinf & ninf)] = np.nan
    return y


def assert_exact(y, y_ref, what=""):
    """Bit-for-bit (up to the sign of zero) equality with the exact product, with a useful message."""
    y = np.asarray(y)
    ok = (y == y_ref) | (np.isnan(y) & np.isnan(y_ref))
    if not ok.all():
        bad = np.flatnonzero(~ok)
        i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {len(y)} rows differ from the exact product "
                             f"({int(np.isnan(y[bad]).sum())} NaN); row {i}: {y[i]!r} != {y_ref[i]!r}")
