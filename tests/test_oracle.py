"""The oracle against everything that can pin it (CPU only).

The reference has no golden vectors and cannot be built here (oracle/ehyb_oracle.c header), so
the pins are: glibc known answers for the x rule, scipy.sparse as an independent product, the
committed fixtures of tests/golden, and self-consistency of the restated reference format
(build + kernel walk == COO product).
"""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import ehyb_ref_layout as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_x_rule_known_answers(O, E):
    """solver_test.c:89-92 under glibc: values recorded in SURVEY.md section 4."""
    known = json.load(open(os.path.join(GOLD, "x_known.json")))
    x = O.x_glibc(943695)
    for k, v in known.items():
        if k.isdigit():
            assert x[int(k)] == pytest.approx(v, abs=1e-15), k
    assert x[:10974].sum() == pytest.approx(known["sum_0_10973"], abs=1e-9)
    assert np.all(x >= -0.1) and np.all(x < 0.1)
    # the product's harness helper follows the same rule
    assert np.array_equal(E.x_glibc(5000), x[:5000])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_products_agree_with_scipy(O, seed):
    rng = np.random.default_rng(seed)
    n = 700
    A = sp.random(n, n, density=0.02, random_state=seed, format="coo", dtype=np.float64)
    order = rng.permutation(A.nnz)  # storage order must not matter beyond rounding
    I, J, V = A.row[order].astype(np.int32), A.col[order].astype(np.int32), A.data[order]
    x = O.x_glibc(n)
    y = O.spmv_coo(n, I, J, V, x)
    scale = O.abs_rowsum(n, I, J, V, x)
    assert O.check_strict(y, A.tocsr() @ x, scale)[0] == 0
    C = A.tocsr()
    for omp in (False, True):
        yc = O.spmv_csr(C.indptr, C.indices, C.data, x, omp=omp)
        assert O.check_strict(yc, y, scale)[0] == 0
    assert np.allclose(scale, abs(C) @ abs(x), rtol=1e-13)


def test_symmetric_rule_equals_expanded(O):
    """solver_test.c:235-255: applying each stored lower entry twice == product with the expanded matrix."""
    rng = np.random.default_rng(5)
    n = 300
    L = sp.tril(sp.random(n, n, density=0.05, random_state=3), format="coo")
    x = O.x_glibc(n)
    y = O.spmv_sym_lower(n, L.row.astype(np.int32), L.col.astype(np.int32), L.data, x)
    full = L + sp.tril(L, -1).T
    scale = abs(full) @ abs(x)
    assert O.check_strict(y, full @ x, scale)[0] == 0
    del rng


def test_compare_restated(O):
    """compare() of solver_test.c:7-29."""
    a = np.array([1.0, 2.0, 0.0, -4.0])
    b = np.array([1.0, 2.05, 0.0, -4.0])
    bad, diff, ampl = O.compare(a, b, 0.01)
    assert bad == 1
    assert diff == pytest.approx(0.05)
    assert ampl == pytest.approx(0.05 / 2.0)
    assert O.compare(a, a, 0.01) == (0, 0.0, 0.0)


def test_reference_sizing_known_cases():
    """solver_test.c:158-182 restated: the two cases SURVEY.md 8a/8d quotes."""
    assert R.reference_sizing(10974, True) == (10, 8192, 8)       # bcsstk17
    assert R.reference_sizing(943695, True)[:2] == (164, 6144)    # audikw_1
    # int16 overflow of vectorCacheSize past ~2.6 M rows
    assert R.reference_sizing(4194304, True)[1] < 0 or R.reference_sizing(4194304, True)[1] * 8 <= 93 * 1024


def _small_matrix(seed, n=640, nparts=4, cache=192):
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    size = n // nparts
    for i in range(n):
        p = i // size
        k = rng.integers(1, 12)
        local = rng.integers(p * size, (p + 1) * size, k)
        far = rng.integers(0, n, rng.integers(0, 3))
        for j in set(local.tolist() + far.tolist() + [i]):
            rows.append(i)
            cols.append(j)
    A = sp.coo_matrix((rng.uniform(-1, 1, len(rows)), (rows, cols)), shape=(n, n)).tocsr()
    A.sort_indices()
    pb = np.arange(0, n + 1, size)
    return A, pb, cache


@pytest.mark.parametrize("warp", [32, 64])
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_format_walk_equals_product(O, warp, seed):
    """Restated COO2EHYB + kernel walk (convert.c / kernel.cu) reproduces the CPU product."""
    A, pb, cache = _small_matrix(seed)
    n = A.shape[0]
    x = O.x_glibc(n)
    L = R.build_reference_ehyb(A.indptr, A.indices, A.data, pb, cache, warp=warp)
    y = R.walk_reference_ehyb(L, x)
    I = np.repeat(np.arange(n), np.diff(A.indptr)).astype(np.int32)
    y_ref = O.spmv_coo(n, I, A.indices, A.data, x)
    scale = O.abs_rowsum(n, I, A.indices, A.data, x)
    assert O.check_strict(y, y_ref, scale)[0] == 0
    assert L["nnz_ell"] + L["to_er"] == A.nnz
    assert L["size_block_ell"] == L["nnz_ell"] + L["waste"]
    assert L["to_er"] > 0  # the generator leaves some entries outside the window


# ---- the NaN-strict checker every parity test ends in (oracle_check_strict)
NAN, INF = float("nan"), float("inf")


def _strict(O, a, b, scale=None):
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    return O.check_strict(a, b, np.ones(len(a)) if scale is None else np.array(scale, dtype=np.float64))


def test_check_tolerance_passes_nan(O):
    """The reason check_strict exists: the old check counts no NaN row as bad (kept as it is for bench.py / smoke())."""
    a, b = np.array([NAN, 1.0, 2.0]), np.array([1.0, 1.0, NAN])
    assert O.check_tolerance(a, b, np.ones(3)) == (0, 0.0)
    assert O.check_strict(a, b, np.ones(3)) == (2, INF)


@pytest.mark.parametrize("a,b", [([NAN], [1.0]), ([1.0], [NAN]), ([NAN, 0.0], [0.0, NAN]), ([NAN], [INF]), ([-INF], [NAN])])
def test_strict_nan_on_one_side_fails(O, a, b):
    bad, worst = _strict(O, a, b)
    assert bad == len(a) and worst == INF


def test_strict_nan_on_both_sides_passes(O):
    assert _strict(O, [NAN, 1.0], [NAN, 1.0]) == (0, 0.0)
    assert _strict(O, [-NAN], [NAN]) == (0, 0.0)          # the sign / payload of a NaN is not compared


@pytest.mark.parametrize("a,b", [([INF], [-INF]), ([INF], [1.0]), ([-1e300], [-INF]), ([0.0], [INF])])
def test_strict_infinity_against_other_fails(O, a, b):
    assert _strict(O, a, b) == (1, INF)
    assert _strict(O, a, b, [INF]) == (1, INF)           # not even the infinite scale of a reference row that holds an inf


def test_strict_matching_infinities_pass(O):
    assert _strict(O, [INF, -INF, 3.0], [INF, -INF, 3.0], [0.0, 0.0, 0.0]) == (0, 0.0)


def test_strict_zero_scale(O):
    """scale 0 (an empty row, or a row whose x are all zero): only exact equality passes."""
    assert _strict(O, [0.0, -0.0, 5.0], [0.0, 0.0, 5.0], [0.0, 0.0, 0.0]) == (0, 0.0)
    assert _strict(O, [1e-300], [0.0], [0.0]) == (1, INF)


def test_strict_finite_rows_as_check_tolerance(O):
    """Where everything is finite, check_strict agrees with check_tolerance row for row, worst included."""
    rng = np.random.default_rng(11)
    b = rng.standard_normal(5000)
    scale = np.abs(b) * rng.uniform(1, 10, 5000)
    scale[::97] = 0
    a = b + rng.standard_normal(5000) * scale * 1e-12 * rng.choice([0.5, 2.0], 5000)
    a[::193] = b[::193]
    ref = O.check_tolerance(a, b, scale)
    assert ref[0] > 0 and ref[1] > 1e-12
    assert O.check_strict(a, b, scale) == ref
    a[::1000] = b[::1000] + scale[::1000] * 1e-13
    ok = np.arange(0, 5000, 1000)
    assert O.check_strict(a[ok], b[ok], scale[ok]) == O.check_tolerance(a[ok], b[ok], scale[ok])


def test_strict_worst_inf_whenever_a_row_fails_non_finite(O):
    a = np.array([1.0, 2.0, 3.0, NAN])
    b = np.array([1.0, 2.5, 3.0, 4.0])
    s = np.ones(4)
    bad, worst = O.check_strict(a, b, s, tol=1.0)      # row 1 within tol, row 3 NaN
    assert bad == 1 and worst == INF
    bad, worst = O.check_strict(a[:3], b[:3], s[:3], tol=0.1)   # row 1 bad, finite
    assert bad == 1 and worst == pytest.approx(0.5)
    a[3] = INF
    assert O.check_strict(a, b, s, tol=1.0) == (1, INF)
