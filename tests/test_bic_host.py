"""The host side of the block incomplete Cholesky preconditioner (bic.cpp; no GPU): blocks, local orders, pattern, levels, shifts
and counts against the restatement of bic_cases.py exactly, the factor within the restatement's bound, the same bits on one and
four OpenMP threads, the level properties, the shift and the fallback rule on blocks built to need them, the errors, and whether
the preconditioner is worth having: on the two 120 x 100 systems of test_gpu_coarse.py the restated PCG with the library's L
must need at most two thirds of Jacobi's iterations on the hard one and no more than Jacobi on the easy one, in both orders."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest
import scipy.sparse as sp

import bic_cases as bc
import coarse_cases as kc
import fsai_cases as fc
from test_gpu_cg import spd_matrix

ERR_ARG, ERR_STATE = 1, 8
ORDERS = ("stored", "colour")
EXACT = ("block_ptr", "perm", "row_ptr", "cols", "level_f", "level_b", "shift", "counts")


def from_scipy(E, A, cfg):
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=True)
    m.reorder(cfg)
    return m


@pytest.fixture(scope="module")
def grid(E):
    cfg = E.make_config(lds_doubles=1024, sym_pairs=0)
    m = from_scipy(E, kc.near_singular_grid(48, 40, 1, 0.0005), cfg)
    return m, m.to_scipy(), cfg


def check_against_restatement(f, want, what):
    got = bc.from_library(f)
    for name in EXACT:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name)
    dv, dd = np.abs(got["vals"] - want["vals"]), np.abs(got["dinv"] - want["dinv"])
    worst_v = float(np.max(np.divide(dv, want["vals_bound"], out=np.zeros_like(dv), where=want["vals_bound"] > 0), initial=0.0))
    worst_d = float(np.max(dd / want["dinv_bound"]))
    print(f"{what}: {got['counts'][0]} blocks, {len(got['cols'])} entries, levels {got['counts'][3]}; worst |VALS - restated| / bound {worst_v:.3f}, "
          f"DINV {worst_d:.3f}")
    assert (dv <= want["vals_bound"]).all() and (dd <= want["dinv_bound"]).all()
    return got


def longest_partition(m):
    return int(np.diff(m.part_boundary).max())


@pytest.mark.parametrize("order", ORDERS)
def test_the_object_equals_the_restatement(E, grid, order):
    m, A, cfg = grid
    assert len(m.part_boundary) - 1 > 1, "more than one partition"
    for block_rows in (0, 1, 64, longest_partition(m) + 1):
        want = bc.build(A, m.part_boundary, block_rows, order)
        f = E.Bic(m, block_rows, order, upload=False)
        got = check_against_restatement(f, want, f"{order}, block_rows {block_rows}")
        lengths = np.diff(got["block_ptr"])
        assert (lengths >= 1).all() and got["block_ptr"][-1] == m.n
        if block_rows in (0, longest_partition(m) + 1):
            assert np.array_equal(got["block_ptr"], m.part_boundary[np.concatenate([[True], np.diff(m.part_boundary) > 0])])
        if block_rows == 1:
            assert f.blocks == m.n and len(got["cols"]) == 0 and f.levels == 1
            assert np.array_equal(got["dinv"], 1.0 / np.sqrt(A.diagonal()))
        if block_rows == 64:
            assert lengths.max() <= 64 and f.blocks > len(m.part_boundary) - 1
            # the runs of a partition differ by one row at the most, the longer ones first
            for lo, hi in zip(m.part_boundary[:-1], m.part_boundary[1:]):
                inside = lengths[(got["block_ptr"][:-1] >= lo) & (got["block_ptr"][:-1] < hi)]
                assert inside.sum() == hi - lo and inside.max() - inside.min() <= 1 and (np.diff(inside) <= 0).all()
        assert f.shifted_blocks == 0 and f.fallback_blocks == 0 and not got["shift"].any()
        assert f.max_k == min(4, bc.MAX_BLOCK // lengths.max())
        # within a block the positions are a permutation of its rows
        for lo, hi in zip(got["block_ptr"][:-1], got["block_ptr"][1:]):
            assert np.array_equal(np.sort(got["perm"][lo:hi]), np.arange(lo, hi))
        if order == "stored":
            assert np.array_equal(got["perm"], np.arange(m.n))
            if block_rows == 0:
                # the pattern of tril of the diagonal blocks
                part = np.searchsorted(m.part_boundary, np.arange(m.n), side="right")
                low = sp.tril(A, -1).tocoo()
                assert len(got["cols"]) == int((part[low.row] == part[low.col]).sum())


@pytest.mark.parametrize("order", ORDERS)
def test_level_properties(E, grid, order):
    m, A, cfg = grid
    f = E.Bic(m, 0, order, upload=False)
    g = bc.from_library(f)
    first = np.repeat(g["block_ptr"][:-1], np.diff(g["block_ptr"]))
    rows = np.repeat(np.arange(m.n), np.diff(g["row_ptr"]))
    cols = first[rows] + g["cols"]
    assert (g["cols"] >= 0).all() and (cols < rows).all(), "strictly lower, inside the block"
    # every stored entry's column has a smaller level than its row (forward), its row a smaller one than its column (backward)
    assert (g["level_f"][cols] < g["level_f"][rows]).all() and (g["level_b"][rows] < g["level_b"][cols]).all()
    empty = np.diff(g["row_ptr"]) == 0
    assert np.array_equal(g["level_f"] == 0, empty), "level 0: exactly the rows without entries"
    no_column = np.bincount(cols, minlength=m.n) == 0
    assert np.array_equal(g["level_b"] == 0, no_column)
    # each level is reached: a row of level l > 0 has an entry of level l - 1
    deepest = np.zeros(m.n, dtype=np.int64)
    np.maximum.at(deepest, rows, g["level_f"][cols] + 1)
    assert np.array_equal(deepest, g["level_f"])
    assert f.levels == max(g["level_f"].max(), g["level_b"].max()) + 1
    if order == "colour":
        colours = bc.build(A, m.part_boundary, 0, order)["colours"]
        print(f"colours per block {colours}, levels {f.levels}")
        assert f.levels <= max(colours)
        stored = E.Bic(m, 0, "stored", upload=False)
        assert f.levels < stored.levels
        assert len(g["cols"]) == len(stored.array("cols")), "the same entries in another order"


def test_the_same_bits_on_one_and_four_threads(E, grid):
    m, A, cfg = grid
    omp = C.CDLL(ctypes.util.find_library("gomp") or "libgomp.so.1")
    before = omp.omp_get_max_threads()
    out = {}
    try:
        for threads in (1, 4):
            omp.omp_set_num_threads(threads)
            for order in ORDERS:
                for block_rows in (0, 64):
                    out[threads, order, block_rows] = bc.from_library(E.Bic(m, block_rows, order, upload=False))
    finally:
        omp.omp_set_num_threads(before)
    for (threads, order, block_rows), got in out.items():
        if threads == 1:
            continue
        for name, a in out[1, order, block_rows].items():
            b = got[name]
            assert a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.itemsize == 8 else np.int32),
                                                         b.view(np.int64 if b.itemsize == 8 else np.int32)), (order, block_rows, name)


def with_component(A, S):
    """A and the small dense symmetric S as one more connected component"""
    return sp.block_diag([sp.csr_matrix(A), sp.csr_matrix(S)]).tocsr()


@pytest.mark.parametrize("case,order", [("kershaw", "stored"), ("five", "stored"), ("five", "colour")])
def test_a_block_ic0_breaks_down_on_is_shifted(E, case, order):
    """An SPD matrix that is not an H-matrix as a component of its own -- Kershaw's 4 x 4 (a 4-cycle: two colours, and in the
    coloured order IC(0) goes through, so it serves the stored order alone) and a 5 x 5 with a triangle for both orders.  IC(0)
    with alpha = 0 meets a non-positive pivot, verified here in the restatement, on the matrix as it stands and again on the
    block as the reordering left it.  Its block must come out shifted with the alpha of the rule, the others not."""
    K = bc.kershaw() if case == "kershaw" else bc.five()
    assert np.linalg.eigvalsh(K).min() > 0
    comparison = 2 * np.diag(np.diag(K)) - np.abs(K)
    assert np.linalg.eigvals(comparison).real.min() < 0, "an H-matrix would not break down"
    assert bc.build(sp.csr_matrix(K), np.array([0, len(K)]), 0, order)["counts"][1] == 1, "IC(0) of the matrix as it stands breaks down"
    cfg = E.make_config(lds_doubles=1024, sym_pairs=0)
    base = kc.near_singular_grid(48, 40, 1, 0.0005)
    m = from_scipy(E, with_component(base, K), cfg)
    A = m.to_scipy()
    want = bc.build(A, m.part_boundary, 0, order)
    f = E.Bic(m, 0, order, upload=False)
    got = check_against_restatement(f, want, f"{order}, with the {case} block")
    assert f.shifted_blocks == 1 == int((got["shift"] > 0).sum()) and f.fallback_blocks == 0
    b = int(np.flatnonzero(got["shift"] > 0)[0])
    alpha = float(got["shift"][b])
    print(f"block {b} of {f.blocks} shifted by {alpha}")
    assert alpha in bc.SHIFTS
    # the alpha of the rule: the first of the sequence the whole block factors with -- every smaller one breaks down
    lo, hi = got["block_ptr"][b], got["block_ptr"][b + 1]
    one = sp.csr_matrix(A[lo:hi][:, lo:hi])
    for a in [0.0] + [s for s in bc.SHIFTS if s < alpha]:
        shifted = (one + a * sp.diags(one.diagonal())).tocsr()
        alone = bc.build(shifted, np.array([0, hi - lo]), 0, order)
        assert alone["counts"][1] == 1 or a == alpha, a
    alone = bc.build((one + alpha * sp.diags(one.diagonal())).tocsr(), np.array([0, hi - lo]), 0, order)
    assert alone["counts"][1] == 0
    # the block holds the component's entries
    assert np.isin(np.unique(K[K != 0]), one.data).all()


def test_a_block_no_shift_saves_takes_its_jacobi_form(E):
    """through create_host: a 2 x 2 component with a positive diagonal and off-diagonal entries 10^6 times larger -- not positive
    definite, and a_ii (1 + alpha) - a_ij^2 / (a_ii (1 + alpha)) < 0 for every alpha up to 2^10"""
    cfg = E.make_config(lds_doubles=1024, sym_pairs=0)
    S = np.array([[1.0, 1e6], [1e6, 1.0]])
    m = from_scipy(E, with_component(kc.near_singular_grid(48, 40, 1, 0.0005), S), cfg)
    A = m.to_scipy()
    want = bc.build(A, m.part_boundary, 0, "stored")
    f = E.Bic(m, 0, "stored", upload=False)
    got = check_against_restatement(f, want, "with a block beyond every shift")
    assert f.fallback_blocks == 1 and f.shifted_blocks == 0 and int((got["shift"] == bc.FALLBACK).sum()) == 1
    b = int(np.flatnonzero(got["shift"] == bc.FALLBACK)[0])
    lo, hi = got["block_ptr"][b], got["block_ptr"][b + 1]
    assert not got["vals"][got["row_ptr"][lo]:got["row_ptr"][hi]].any(), "nothing but the diagonal"
    assert np.array_equal(got["dinv"][lo:hi], 1.0 / np.sqrt(A.diagonal()[got["perm"][lo:hi]]))
    good = E.Bic(from_scipy(E, kc.near_singular_grid(48, 40, 1, 0.0005), cfg), 0, "stored", upload=False)
    assert good.fallback_blocks == 0


def test_errors(E, grid):
    lib = E.host._lib.load()
    m, A, cfg = grid
    h = C.c_void_p()
    mp = C.byref(m.c)
    create = lambda mat, block_rows=0, order=0, out=C.byref(h): lib.ehyb_bic_create_host(mat, block_rows, order, out)  # noqa: E731
    assert create(None) == ERR_ARG and b"null" in lib.ehyb_last_error()
    assert create(mp, out=None) == ERR_ARG
    assert create(mp, block_rows=-1) == ERR_ARG and b"block_rows -1" in lib.ehyb_last_error()
    assert create(mp, order=2) == ERR_ARG and b"order 2" in lib.ehyb_last_error()
    assert create(mp, order=-1) == ERR_ARG
    fresh = E.Matrix.generate("stencil2d", 8, 8, 5, 0, 1)
    fresh.c.nParts = 0
    assert create(C.byref(fresh.c)) == ERR_ARG and b"partition" in lib.ehyb_last_error()
    assert not h.value
    bad = from_scipy(E, kc.near_singular_grid(12, 10, 1, 0.0005), cfg)
    keep = int(bad.J[5])
    bad.J[5] = bad.n
    assert create(C.byref(bad.c)) == ERR_ARG and b"outside the matrix" in lib.ehyb_last_error() and not h.value
    bad.J[5] = keep
    assert lib.ehyb_bic_upload(None) == ERR_ARG
    assert lib.ehyb_bic_host_array(None, 0, C.byref(C.c_void_p()), C.byref(C.c_int64())) == ERR_ARG
    assert lib.ehyb_bic_apply(None, None, 0, None, 0, 1, None) == ERR_ARG
    assert lib.ehyb_bic_max_k(None) == 0
    lib.ehyb_bic_destroy(None)
    f = E.Bic(m, upload=False)
    assert lib.ehyb_bic_host_array(f.h, 10, C.byref(C.c_void_p()), C.byref(C.c_int64())) == ERR_ARG
    # a diagonal entry that is not positive
    d = int(np.flatnonzero(bad.J[bad.row_idx[7]:bad.row_idx[8]] == 7)[0])
    for value in (-1.0, 0.0, np.inf, np.nan):
        bad.V[bad.row_idx[7] + d] = value
        with pytest.raises(E.EhybError) as ei:
            E.Bic(bad, upload=False)
        assert ei.value.code == ERR_ARG and "not positive definite" in str(ei.value) and "row 7" in str(ei.value)
        with pytest.raises(ValueError):
            bc.build(bad.to_scipy(), bad.part_boundary)


def test_raw_objects_and_their_refusals(E):
    rng = np.random.default_rng(4)
    bp, rp, cols, vals, dinv = bc.staged_factor(rng, [5, 1, 70])
    f = E.Bic.raw(bp, rp, cols, vals, dinv, upload=False)
    g = bc.from_library(f)
    lf, lb, most = bc.levels(bp, rp, cols)
    assert np.array_equal(g["level_f"], lf) and np.array_equal(g["level_b"], lb) and f.levels == most <= 5 and f.blocks == 3
    assert np.array_equal(g["perm"], np.arange(76)) and np.array_equal(g["vals"], vals) and np.array_equal(g["dinv"], dinv)

    def refused(bp=bp, rp=rp, cols=cols, vals=vals, dinv=dinv, word=b""):
        with pytest.raises(E.EhybError) as ei:
            E.Bic.raw(bp, rp, cols, vals, dinv, upload=False)
        assert ei.value.code == ERR_ARG and word in str(ei.value).encode(), str(ei.value)

    row = int(np.flatnonzero(np.diff(rp) >= 2)[0])
    c = cols.copy()
    c[rp[row]] = row - (0 if row < 5 else 5 if row == 5 else 6)          # its own position: the diagonal
    refused(cols=c, word=b"not strictly lower")
    c = cols.copy()
    c[rp[row]] = -1
    refused(cols=c, word=b"outside the block")
    c = cols.copy()
    c[rp[row]:rp[row] + 2] = c[rp[row]:rp[row] + 2][::-1].copy()
    refused(cols=c, word=b"unsorted")
    refused(bp=np.array([0, 5, 5, 76], dtype=np.int32), word=b"rows (1 ..")
    n = bc.MAX_BLOCK + 1
    refused(bp=np.array([0, n]), rp=np.zeros(n + 1, dtype=np.int64), cols=np.zeros(0), vals=np.zeros(0), dinv=np.ones(n), word=b"20481 rows")
    for length, want in ((bc.MAX_BLOCK, 1), (10241, 1), (10240, 2), (6827, 2), (6826, 3), (5121, 3), (5120, 4), (1, 4)):
        f = E.Bic.raw(np.array([0, length]), np.zeros(length + 1, dtype=np.int64), np.zeros(0), np.zeros(0), np.ones(length), upload=False)
        assert f.max_k == want, (length, f.max_k)


def test_solver_argument_order(E, grid):
    """what shows without a device: everything up to the uploads, which come last"""
    lib = E.host._lib.load()
    m, A, cfg = grid
    plan = E.Plan(m, cfg, upload=False)
    f = E.Bic(m, upload=False)
    small = from_scipy(E, kc.near_singular_grid(12, 10, 1, 0.0005), cfg)
    other = E.Bic(small, upload=False)
    p = C.c_void_p(0x10000)             # never read: every call fails before device work
    one = lambda plan_h, f_h, b=p, x=p, max_iter=10, rtol=1e-8: lib.ehyb_pcg_bic(plan_h, f_h, b, x, max_iter, rtol, 10, None, None, None)  # noqa: E731
    multi = lambda plan_h, f_h, ldb=m.n, k=2, max_iter=10: lib.ehyb_pcg_bic_multi(plan_h, f_h, p, ldb, p, m.n, k, max_iter, 1e-8, 10, None, None,  # noqa: E731
                                                                                   None)
    assert one(None, None) == ERR_ARG and b"null argument" in lib.ehyb_last_error()
    assert one(plan.h, None, b=None) == ERR_ARG and b"null argument" in lib.ehyb_last_error()
    assert one(plan.h, None, max_iter=-1) == ERR_ARG and b"max_iter" in lib.ehyb_last_error()
    assert one(plan.h, None, rtol=float("nan")) == ERR_ARG and b"rtol" in lib.ehyb_last_error()
    assert multi(plan.h, None, k=0) == ERR_ARG and b"right-hand sides" in lib.ehyb_last_error()
    assert multi(plan.h, None, ldb=m.n - 1) == ERR_ARG and b"ldb" in lib.ehyb_last_error()
    for call in (one, multi):
        assert call(plan.h, None) == ERR_ARG and b"null bic object" in lib.ehyb_last_error()
        assert call(plan.h, other.h) == ERR_ARG and f"{small.n} rows".encode() in lib.ehyb_last_error()
        assert call(plan.h, f.h) == ERR_STATE and b"plan not uploaded" in lib.ehyb_last_error()
    assert lib.ehyb_bic_apply(f.h, p, m.n, p, m.n, 1, None) == ERR_STATE and b"bic object not uploaded" in lib.ehyb_last_error()
    assert lib.ehyb_bic_apply(f.h, p, m.n - 1, p, m.n, 1, None) == ERR_ARG and lib.ehyb_bic_apply(f.h, p, m.n, p, m.n, 0, None) == ERR_ARG


# ------------------------------------------------------------------ worth it?
@pytest.mark.parametrize("name", ["hard", "easy"])
def test_bic_against_jacobis_iterations(E, name):
    """The two 120 x 100 systems of test_gpu_coarse.py, lds_doubles = 2048, whole partitions, b uniform in [-1, 1] in the permuted
    numbering, rtol 1e-10, the restated PCG with the library's L: at most 2 / 3 of Jacobi's iterations on the hard system, no
    more than Jacobi's on the easy one, in both orders.  A prototype on contiguous blocks of 2048 rows gave 239 (stored) and 360
    (colour) against 668, and 33 and 42 against 74; the library's partitions are more compact, and the bar leaves the weaker arm
    a margin of about 1.2."""
    A0 = kc.near_singular_grid(120, 100, 1, 0.0005) if name == "hard" else spd_matrix(120, 100, 3000, 1)
    cfg = E.make_config(lds_doubles=2048, sym_pairs=0)
    m = from_scipy(E, A0, cfg)
    A = m.to_scipy()
    b = np.random.default_rng(3).uniform(-1, 1, m.n)
    it_jacobi = fc.jacobi_pcg(A, b, max_iter=5000, rtol=1e-10)
    for order in ORDERS:
        f = E.Bic(m, 0, order, upload=False)
        assert f.shifted_blocks == 0 and f.fallback_blocks == 0
        x, it = bc.pcg(A, b, bc.Solver(bc.from_library(f)), max_iter=5000, rtol=1e-10)
        print(f"{name}, {order}: BIC-PCG {it} iterations, Jacobi-PCG {it_jacobi} (ratio {it_jacobi / it:.2f}); {f.blocks} blocks, {f.levels} levels")
        assert np.linalg.norm(A @ x - b) <= 2e-10 * np.linalg.norm(b)
        if name == "hard":
            assert 3 * it <= 2 * it_jacobi, (it, it_jacobi)
        else:
            assert it <= it_jacobi, (it, it_jacobi)
