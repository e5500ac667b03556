"""The host side of the FSAI preconditioner (fsai.cpp; no GPU): the pattern against the numpy restatement of fsai_cases.py, the
row cap and its ties rule, every row of G against the backward-error bound of its dense solve, the same bits on 1, 2 and 5
OpenMP threads, the plans of G and G^T slot by slot, the fallback, the errors, and whether the preconditioner is worth having:
on the two 120 x 100 systems of test_gpu_coarse.py the restated PCG with the library's G must need at most two thirds of
Jacobi's iterations."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_cases as kc
import fsai_cases as fc
from test_gpu_cg import spd_matrix

ERR_ARG, ERR_STATE = 1, 8


def from_scipy(E, A, cfg):
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=True)
    m.reorder(cfg)
    return m


def tied_banded(E, cfg, n=192, block=96):
    """dense diagonal blocks (ehyb_gen_banded with band = block: m_i runs through 1 .. block) with SPD values on three levels of
    magnitude, so that a capped row has to choose among equals"""
    P = sp.csr_matrix(E.Matrix.generate("banded", n, block, block, cfg=cfg).to_scipy())
    P.sort_indices()
    A = kc.spd_on_the_pattern(P, 0.5).tocoo()
    off = A.row != A.col
    data = np.where(off, -(1.0 + (A.row + A.col) % 3), 0.0)
    A = sp.csr_matrix((data, (A.row, A.col)), shape=A.shape)
    return (A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 0.5)).tocsr()


@pytest.fixture(scope="module")
def grid(E):
    cfg = E.make_config(lds_doubles=1024, sym_pairs=0)
    m = from_scipy(E, kc.near_singular_grid(48, 40, 1, 0.0005), cfg)
    return m, m.to_scipy(), cfg


@pytest.fixture(scope="module")
def banded(E):
    cfg = E.make_config(lds_doubles=1024, sym_pairs=0)
    m = from_scipy(E, tied_banded(E, cfg), cfg)
    return m, m.to_scipy(), cfg


def arrays(f):
    return f.array("row_ptr"), f.array("cols"), f.array("vals")


def test_pattern_equals_the_restatement(E, grid):
    m, A, cfg = grid
    assert len(m.part_boundary) - 1 > 1, "more than one partition"
    f = E.Fsai(m, cfg=cfg, upload=False)
    row_ptr, cols, _ = arrays(f)
    want_ptr, want_cols, want_capped = fc.pattern(A)
    assert row_ptr.dtype == np.int64 and np.array_equal(row_ptr, want_ptr) and np.array_equal(cols, want_cols)
    assert f.capped_rows == want_capped == 0 and f.fallback_rows == 0
    assert len(cols) == (sp.tril(A).nnz), "the pattern of tril(A)"


def test_row_cap_and_ties(E, banded):
    m, A, cfg = banded
    lengths = np.diff(fc.pattern(A, 10 ** 6)[0])
    assert {1, 2, 63, 64, 65, 96} <= set(lengths.tolist()), "m_i runs through 1, 2, 63, 64 and beyond"
    capped = {}
    for cap in (0, 64, 8, 1):
        f = E.Fsai(m, row_cap=cap, cfg=cfg, upload=False)
        row_ptr, cols, vals = arrays(f)
        want_ptr, want_cols, want_capped = fc.pattern(A, cap)
        assert np.array_equal(row_ptr, want_ptr) and np.array_equal(cols, want_cols) and f.capped_rows == want_capped
        assert np.diff(row_ptr).max() == (cap or 64)
        capped[cap] = f.capped_rows
        worst, _ = fc.rows_within_bounds(A, row_ptr, cols, vals)
        print(f"row_cap {cap}: {f.capped_rows} capped rows, worst residual / bound {worst:.3f}")
        assert worst <= 1 and f.fallback_rows == 0
        for i in range(m.n):
            J = cols[row_ptr[i]:row_ptr[i + 1]]
            assert J[-1] == i and (np.diff(J) > 0).all()
        if cap == 8:
            # the ties rule on the rows themselves: every dropped column is smaller in magnitude than every kept one, or equal
            # to the smallest kept and then to the right of every kept column of that magnitude
            ties = 0
            for i in np.flatnonzero(lengths > 8):
                kept = cols[row_ptr[i]:row_ptr[i + 1] - 1]
                row = np.abs(A[i].toarray().ravel())
                dropped = np.setdiff1d(np.flatnonzero(row[:i]), kept)
                low = row[kept].min()
                assert (row[dropped] <= low).all()
                equal = dropped[row[dropped] == low]
                ties += len(equal) > 0
                assert len(equal) == 0 or equal.min() > kept[row[kept] == low].max()
            assert ties > 0, "no row had to choose among equals"
    assert capped[0] == capped[64] == int((lengths > 64).sum()) > 0 and capped[8] > capped[64] and capped[1] == m.n - 2


def test_every_row_meets_the_backward_error_bound(E, grid):
    m, A, cfg = grid
    f = E.Fsai(m, cfg=cfg, upload=False)
    row_ptr, cols, vals = arrays(f)
    want, fell = fc.factor(A, row_ptr, cols)
    worst_r, worst_f = fc.rows_within_bounds(A, row_ptr, cols, vals, other=want)
    print(f"grid: {m.n} rows, worst residual / bound {worst_r:.3f}, worst distance to numpy's rows / forward bound {worst_f:.3f}")
    assert fell == 0 and worst_r <= 1 and worst_f <= 1
    G = fc.matrix(row_ptr, cols, vals)
    assert np.abs((G @ A @ G.T).diagonal() - 1).max() <= 1e-12, "diag(G A G^T) = 1"


def test_the_same_bits_on_one_two_and_five_threads(E, grid, banded):
    omp = C.CDLL(ctypes.util.find_library("gomp") or "libgomp.so.1")
    before = omp.omp_get_max_threads()
    out = {}
    try:
        for threads in (1, 2, 5):
            omp.omp_set_num_threads(threads)
            for name, (m, _, cfg), cap in (("grid", grid, 0), ("banded", banded, 8)):
                f = E.Fsai(m, row_cap=cap, cfg=cfg, upload=False)
                out[threads, name] = arrays(f) + (f.array("counts"),)
    finally:
        omp.omp_set_num_threads(before)
    for name in ("grid", "banded"):
        for threads in (2, 5):
            for a, b in zip(out[1, name], out[threads, name]):
                assert a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.itemsize == 8 else np.int32),
                                                             b.view(np.int64 if b.itemsize == 8 else np.int32)), (name, threads)


@pytest.mark.parametrize("plan_kw", [dict(), dict(direct=2), dict(direct=2, window_mode=1, lds_doubles=512), dict(direct=2, val_f32=1)],
                         ids=["default", "window", "csr-residual", "val_f32"])
def test_the_plans_hold_exactly_the_values(E, grid, plan_kw):
    m, A, cfg = grid
    kw = {**dict(lds_doubles=1024, sym_pairs=0), **plan_kw}
    f = E.Fsai(m, cfg=E.make_config(**{**kw, "sym_pairs": 1}), upload=False)     # (sym_pairs is forced off)
    row_ptr, cols, vals = arrays(f)
    G = fc.matrix(row_ptr, cols, vals)
    Gt = G.T.tocsr()
    Gt.sort_indices()
    plan_g, plan_t = f.plans
    for plan, M in ((plan_g, G), (plan_t, Gt)):
        st = plan.stats
        assert st["sym_pairs"] == 0 and st["nnz"] == M.nnz and st["n_rows"] == m.n
        assert np.array_equal(plan.array("part_boundary"), m.part_boundary), "G lives on the partitions of A"
        seen = []
        for val, src in (("ell_val", "ell_src"), ("er_val", "er_src")):
            v, s = plan.array(val), plan.array(src)
            assert len(v) == len(s)
            assert np.array_equal(v[s >= 0].view(np.int64), M.data[s[s >= 0]].view(np.int64)) and not v[s < 0].any()
            seen.append(s[s >= 0])
        assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(M.nnz)), "every entry of the matrix sits in exactly one slot"
    if "window_mode" in plan_kw:
        assert plan_g.stats["nnz_er"] > 0
    if "direct" in plan_kw:
        assert plan_g.stats["nnz_ell"] > 0
    # transpose="spmv_t": one plan
    if plan_kw.get("val_f32"):
        with pytest.raises(E.EhybError) as ei:
            E.Fsai(m, cfg=E.make_config(lds_doubles=1024, **plan_kw), transpose="spmv_t", upload=False)
        refusal = E.Plan(m, E.make_config(lds_doubles=1024, sym_pairs=0, **plan_kw), upload=False).spmv_t_refusal
        assert ei.value.code == ERR_ARG == refusal[0] and refusal[1] and refusal[1] in str(ei.value)
    else:
        one = E.Fsai(m, cfg=E.make_config(**kw), transpose="spmv_t", upload=False)
        assert one.plans[1] is None and np.array_equal(one.array("vals").view(np.int64), vals.view(np.int64))


def test_an_indefinite_block_falls_back_and_is_counted(E):
    cfg = E.make_config(lds_doubles=1024, sym_pairs=0)
    m = from_scipy(E, kc.near_singular_grid(48, 40, 1, 0.0005), cfg)
    good = E.Fsai(m, cfg=cfg, upload=False)
    row_ptr, cols, vals = arrays(good)
    A = m.to_scipy()
    i = int(np.flatnonzero(np.diff(row_ptr) == 3)[100])
    j = int(cols[row_ptr[i]])
    rp, J, V = m.row_idx, m.J, m.V
    big = -10.0 * A[i, i]
    for r, c in ((i, j), (j, i)):            # the pair a_ij = a_ji beyond the diagonal: the block of row i is indefinite
        at = rp[r] + int(np.flatnonzero(J[rp[r]:rp[r + 1]] == c)[0])
        V[at] = big
    B = m.to_scipy()
    assert B[i, j] == B[j, i] == big and np.linalg.eigvalsh(fc.block(B, cols[row_ptr[i]:row_ptr[i + 1]])).min() < 0
    f = E.Fsai(m, cfg=cfg, upload=False)
    rp2, cols2, vals2 = arrays(f)
    assert np.array_equal(rp2, row_ptr) and np.array_equal(cols2, cols) and f.fallback_rows == 1 and good.fallback_rows == 0
    want = np.zeros(3)
    want[-1] = 1.0 / np.sqrt(B[i, i])
    assert np.array_equal(vals2[row_ptr[i]:row_ptr[i + 1]], want)
    others = np.ones(len(vals), dtype=bool)
    others[row_ptr[i]:row_ptr[i + 1]] = False
    assert np.array_equal(vals2[others].view(np.int64), vals[others].view(np.int64)), "the other rows are left alone"
    want_vals, fell = fc.factor(B, row_ptr, cols)
    assert fell == 1 and np.array_equal(want_vals[row_ptr[i]:row_ptr[i + 1]], want)


def test_errors(E, grid):
    lib = E.host._lib.load()
    m, A, cfg = grid
    h = C.c_void_p()
    mp = C.byref(m.c)
    create = lambda mat, cap=0, mode=0, out=C.byref(h): lib.ehyb_fsai_create_host(mat, cap, C.byref(cfg), mode, out)  # noqa: E731
    assert create(None) == ERR_ARG and b"null" in lib.ehyb_last_error()
    assert create(mp, out=None) == ERR_ARG
    assert create(mp, cap=65) == ERR_ARG and b"row_cap 65" in lib.ehyb_last_error()
    assert create(mp, mode=2) == ERR_ARG and b"transpose_mode" in lib.ehyb_last_error()
    fresh = E.Matrix.generate("stencil2d", 8, 8, 5, 0, 1)
    fresh.c.nParts = 0
    assert create(C.byref(fresh.c)) == ERR_ARG and b"partition" in lib.ehyb_last_error()
    assert not h.value
    assert lib.ehyb_fsai_upload(None) == ERR_ARG
    assert lib.ehyb_fsai_host_array(None, 0, C.byref(C.c_void_p()), C.byref(C.c_int64())) == ERR_ARG
    assert lib.ehyb_fsai_plans(None, C.byref(C.c_void_p()), C.byref(C.c_void_p())) == ERR_ARG
    assert lib.ehyb_fsai_apply(None, None, None, None) == ERR_ARG
    assert lib.ehyb_fsai_set_values(None, None, 0, None, 0, None) == ERR_ARG
    lib.ehyb_fsai_destroy(None)
    f = E.Fsai(m, cfg=cfg, upload=False)
    assert lib.ehyb_fsai_host_array(f.h, 4, C.byref(C.c_void_p()), C.byref(C.c_int64())) == ERR_ARG
    # a diagonal entry that is not positive
    bad = from_scipy(E, kc.near_singular_grid(12, 10, 1, 0.0005), cfg)
    d = int(np.flatnonzero(bad.J[bad.row_idx[7]:bad.row_idx[8]] == 7)[0])
    for value in (-1.0, 0.0, np.inf, np.nan):
        bad.V[bad.row_idx[7] + d] = value
        with pytest.raises(E.EhybError) as ei:
            E.Fsai(bad, cfg=cfg, upload=False)
        assert ei.value.code == ERR_ARG and "not positive definite" in str(ei.value) and "row 7" in str(ei.value)


def test_solver_argument_order(E, grid):
    """what shows without a device: everything up to the uploads, which come last"""
    lib = E.host._lib.load()
    m, A, cfg = grid
    plan = E.Plan(m, cfg, upload=False)
    f = E.Fsai(m, cfg=cfg, upload=False)
    small = from_scipy(E, kc.near_singular_grid(12, 10, 1, 0.0005), cfg)
    other = E.Fsai(small, cfg=cfg, upload=False)
    p = C.c_void_p(0x10000)             # never read: every call fails before device work
    one = lambda plan_h, f_h, b=p, x=p, max_iter=10, rtol=1e-8: lib.ehyb_pcg_fsai(plan_h, f_h, b, x, max_iter, rtol, 10, None, None, None)  # noqa: E731
    multi = lambda plan_h, f_h, ldb=m.n, k=2, max_iter=10: lib.ehyb_pcg_fsai_multi(plan_h, f_h, p, ldb, p, m.n, k, max_iter, 1e-8, 10, None, None,  # noqa: E731
                                                                                    None)
    assert one(None, None) == ERR_ARG and b"null argument" in lib.ehyb_last_error()
    assert one(plan.h, None, b=None) == ERR_ARG and b"null argument" in lib.ehyb_last_error()
    assert one(plan.h, None, max_iter=-1) == ERR_ARG and b"max_iter" in lib.ehyb_last_error()
    assert one(plan.h, None, rtol=float("nan")) == ERR_ARG and b"rtol" in lib.ehyb_last_error()
    assert multi(plan.h, None, k=0) == ERR_ARG and b"right-hand sides" in lib.ehyb_last_error()
    assert multi(plan.h, None, ldb=m.n - 1) == ERR_ARG and b"ldb" in lib.ehyb_last_error()
    for call in (one, multi):
        assert call(plan.h, None) == ERR_ARG and b"null fsai object" in lib.ehyb_last_error()
        assert call(plan.h, other.h) == ERR_ARG and f"{small.n} rows".encode() in lib.ehyb_last_error()
        assert call(plan.h, f.h) == ERR_STATE and b"plan not uploaded" in lib.ehyb_last_error()
    assert lib.ehyb_fsai_apply(f.h, p, p, None) == ERR_STATE and b"fsai object not uploaded" in lib.ehyb_last_error()
    assert lib.ehyb_fsai_set_values(f.h, p, m.nnz, None, 1, None) == ERR_STATE
    assert lib.ehyb_fsai_tt_step(5, p, p, 2, None) == ERR_ARG and lib.ehyb_fsai_tt_step(5, None, p, 0, None) == ERR_ARG


# ------------------------------------------------------------------ worth it?
@pytest.mark.parametrize("name", ["hard", "easy"])
def test_fsai_needs_at_most_two_thirds_of_jacobis_iterations(E, name):
    """The two 120 x 100 systems of test_gpu_coarse.py, lds_doubles = 2048, b uniform in [-1, 1] in the permuted numbering, rtol
    1e-10: 1.5 * it_fsai <= it_jacobi for the restated PCG with the library's G.  A prototype of the specification gave 355
    against 668 on the nearly singular grid and 40 against 74 on the diagonally dominant one; the factor 1.5 is a condition on
    the preconditioner, not a measurement of it.  With G rounded to fp32 (cfg.val_f32) the count may grow by a tenth at the most:
    the condition test_gpu_fsai.py takes its fp32 margin from."""
    A0 = kc.near_singular_grid(120, 100, 1, 0.0005) if name == "hard" else spd_matrix(120, 100, 3000, 1)
    cfg = E.make_config(lds_doubles=2048, sym_pairs=0)
    m = from_scipy(E, A0, cfg)
    A = m.to_scipy()
    b = np.random.default_rng(3).uniform(-1, 1, m.n)
    f = E.Fsai(m, cfg=cfg, upload=False)
    G = fc.matrix(*arrays(f))
    x, it = fc.pcg(A, b, G, max_iter=5000, rtol=1e-10)
    it_jacobi = fc.jacobi_pcg(A, b, max_iter=5000, rtol=1e-10)
    G32 = fc.matrix(f.array("row_ptr"), f.array("cols"), f.array("vals").astype(np.float32).astype(np.float64))
    x32, it32 = fc.pcg(A, b, G32, max_iter=5000, rtol=1e-10)
    print(f"{name}: FSAI-PCG {it} iterations, with G in fp32 {it32}, Jacobi-PCG {it_jacobi} (ratio {it_jacobi / it:.2f})")
    assert np.linalg.norm(A @ x - b) <= 2e-10 * np.linalg.norm(b) and np.linalg.norm(A @ x32 - b) <= 2e-10 * np.linalg.norm(b)
    assert 1.5 * it <= it_jacobi, (it, it_jacobi)
    assert it32 <= 1.1 * it, (it32, it)
