"""ehyb_bicgstab_multi: k independent BiCGSTAB solves that share both multiplies of every iteration (ehyb_spmm).

Column j is ehyb_bicgstab(b_j) by construction -- the same grid, index walk and summation order per column, its own scalars,
status word and counter, all decided on the device -- so with plain storage every column must equal the one-vector solve bit
for bit: X, iterations and relative residual, whatever k, check_every, graph use, stream and the other columns.  Where the
multiply's summation order is free (symmetric pairs, a panel-form residual) the columns are held to the bounds of
tests/test_gpu_bicgstab.py.  Everything runs in the permuted numbering unless said otherwise."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from test_gpu_bicgstab import System, cd_matrix, cpu_bicgstab, panel_matrix

pytestmark = pytest.mark.gpu

ERR_ARG = 1
KS = (1, 2, 3, 4, 5, 7)

# plain storage over the multiply shapes of test_gpu_bicgstab.SHAPES, and the halo window at widths where one pass serves
# fewer than four columns.  The last entry is the widest k one pass serves: this matrix of 12,000 rows fills a window of 5,429
# doubles at lds_doubles = 8192 (three images fit: k = 5 takes passes of 3 + 2, k = 7 of 3 + 2 + 2) and one of 7,430 at 12288
# (two fit: k = 5 takes three passes)
PLAIN = [
    ("halo-window", lambda: cd_matrix(120, 100, 3000, 1), dict(window_mode=2, lds_doubles=2048), None),
    ("reference-window-csr-residual", lambda: cd_matrix(120, 100, 3000, 2), dict(window_mode=1, lds_doubles=512), None),
    ("direct", lambda: cd_matrix(110, 90, 2000, 3), dict(direct=1), None),
    ("halo-window-three-wide", lambda: cd_matrix(120, 100, 3000, 1), dict(window_mode=2, lds_doubles=8192), 3),
    ("halo-window-two-wide", lambda: cd_matrix(120, 100, 3000, 1), dict(window_mode=2, lds_doubles=12288), 2),
]


def rhs_bank(E, s, k, seed=0):
    """k right-hand sides (permuted) that stop at different iteration counts: smooth ones, random ones, spikes"""
    rng = np.random.default_rng(seed)
    n = s.n
    out = []
    for j in range(k):
        kind = j % 4
        if kind == 0:
            b = s.A @ (np.ones(n) if j == 0 else np.linspace(-1, 1, n))
        elif kind == 1:
            b = rng.uniform(-1, 1, n) * 10.0 ** (1 - j)
        elif kind == 2:
            b = np.zeros(n)
            b[rng.integers(0, n, 1 + j)] = 1.0
        else:
            b = s.A @ np.sin(np.arange(n) * (0.001 * (j + 1))) + 0.01 * rng.uniform(-1, 1, n)
        out.append(E.vector_reorder(b, s.perm))
    return np.stack(out)


def singles(plan, B, X0=None, **kw):
    xs, its, rels = [], [], []
    for j in range(len(B)):
        x, it, rel = plan.bicgstab(B[j], x0=None if X0 is None else X0[j], allow_breakdown=True, **kw)
        xs.append(x)
        its.append(it)
        rels.append(rel)
    return np.stack(xs), np.array(its), np.array(rels)


def assert_same_bits(got, want, what):
    X, it, rel = got
    Xw, itw, relw = want
    assert np.array_equal(it, itw), (what, it, itw)
    assert np.array_equal(np.asarray(rel).view(np.int64), np.asarray(relw).view(np.int64)), (what, rel, relw)
    for j in range(len(X)):
        assert np.array_equal(X[j].view(np.int64), Xw[j].view(np.int64)), (what, j, np.abs(X[j] - Xw[j]).max())


class PlainCase:
    """a plain-storage system, a bank of seven right-hand sides and guesses, and the one-vector solves of the bank (once each)"""
    RUN = dict(max_iter=600, rtol=1e-10)

    def __init__(self, E, name, make, kw, k_max):
        self.name = name
        self.s = System(E, make(), sym_pairs=0, **kw)
        st = self.s.plan.stats
        assert st["sym_pairs"] == 0
        if k_max is not None:
            assert self.s.plan.spmm_max_k == k_max, self.s.plan.spmm_max_k
        if name == "direct":
            assert st["nnz_ell"] == 0
        elif name == "reference-window-csr-residual":
            assert st["nnz_er"] > 0 and st["nnz_ell"] > 0
        else:
            assert st["nnz_ell"] > 0
        self.B = rhs_bank(E, self.s, max(KS), seed=21)
        self.X0 = np.zeros_like(self.B)
        self.X0[1::3] = 0.01 * np.random.default_rng(22).uniform(-1, 1, self.X0[1::3].shape)   # some columns start from a guess
        self._single = {}

    def single(self, jacobi):
        if jacobi not in self._single:
            self._single[jacobi] = singles(self.s.plan, self.B, self.X0, inv_diag=self.s.inv_diag if jacobi else None, **self.RUN)
        return self._single[jacobi]


@pytest.fixture(scope="module", params=PLAIN, ids=[p[0] for p in PLAIN])
def plain_case(request):
    import ehyb_spmv_gpu_amd as E

    return PlainCase(E, *request.param)


@pytest.mark.parametrize("k", KS)
def test_bit_identity_with_the_one_vector_solve(E, gpu, plain_case, k):
    c = plain_case
    for jacobi in (True, False):
        want = tuple(a[:k] for a in c.single(jacobi))
        got = c.s.plan.bicgstab_multi(c.B[:k], c.X0[:k], check_every=4, allow_breakdown=True,
                                      inv_diag=c.s.inv_diag if jacobi else None, **c.RUN)
        assert_same_bits(got, want, f"{c.name} k={k} jacobi={jacobi}")
        assert (got[1] > 0).all(), got[1]
        if k >= 2:
            assert len(set(int(i) for i in got[1])) >= 2, (c.name, k, got[1])     # or nothing ever froze beside a running column


@pytest.mark.parametrize("max_iter", [2000, 23], ids=["converges", "max-iter"])
def test_same_bits_for_every_check_every_graph_and_stream(E, gpu, max_iter):
    A = cd_matrix(120, 100, 3000, 6)
    kw = dict(window_mode=2, lds_doubles=2048, sym_pairs=0)
    s = System(E, A, **kw)
    plain = E.Plan(s.m, E.make_config(graphs=2, **kw))
    B = rhs_bank(E, s, 4, seed=8)
    run = dict(max_iter=max_iter, rtol=1e-10, inv_diag=s.inv_diag)
    ref = s.plan.bicgstab_multi(B, check_every=1, **run)
    assert (ref[1] > 0).all() and ((ref[1] < max_iter).all() if max_iter == 2000 else (ref[1] == max_iter).any()), ref[1:]
    for check_every in (3, 10, 0):
        assert_same_bits(s.plan.bicgstab_multi(B, check_every=check_every, **run), ref, f"check_every={check_every}")
        assert_same_bits(plain.bicgstab_multi(B, check_every=check_every, **run), ref, f"graphs=2 check_every={check_every}")
    st = E.Stream()
    try:
        assert_same_bits(s.plan.bicgstab_multi(B, check_every=10, stream=st.ptr, **run), ref, "user stream")
    finally:
        st.destroy()
    assert_same_bits(s.plan.bicgstab_multi(B, check_every=1, **run), ref, "second run")


def test_past_the_unrolled_loops(E, gpu):
    """4 * 131072 < n < 5 * 131072: at 512 workgroups every thread takes a four-stride trip and the first 256 a tail trip too"""
    A = cd_matrix(768, 683, 20000, 31)
    n = A.shape[0]
    assert n == 4 * 131072 + 256
    s = System(E, A, lds_doubles=5120, sym_pairs=0)
    assert s.plan.spmm_max_k == 4 and s.plan.stats["sym_pairs"] == 0
    B = rhs_bank(E, s, 4, seed=32)
    run = dict(max_iter=12, rtol=1e-30, inv_diag=s.inv_diag)
    got = s.plan.bicgstab_multi(B, **run)
    assert (got[1] == 12).all(), got[1]
    assert_same_bits(got, singles(s.plan, B, **run), "n = 524,544")


def test_columns_with_nothing_to_do_or_broken_stay_put(E, gpu):
    """b = 0, an exact integer solution as the guess (integer matrix: A x0 is exact), a NaN in b, and two ordinary columns"""
    rng = np.random.default_rng(10)
    A = cd_matrix(90, 80, 1500, 10, pe_max=3.0)
    A.data = np.round(A.data * 4)
    A.eliminate_zeros()
    s = System(E, A, lds_doubles=2048, sym_pairs=0)
    n = s.n
    x_exact = rng.integers(-50, 50, n).astype(np.float64)
    B = np.stack([E.vector_reorder(b, s.perm) for b in
                  (rng.uniform(-1, 1, n), np.zeros(n), A @ x_exact, rng.uniform(-1, 1, n), A @ np.linspace(-1, 1, n) + 0.5)])
    B[3, n // 3] = np.nan
    X0 = np.zeros_like(B)
    X0[2] = E.vector_reorder(x_exact, s.perm)
    X0[3] = rng.uniform(-1, 1, n)
    X0[4] = 0.01 * rng.uniform(-1, 1, n)
    run = dict(max_iter=500, rtol=1e-12, check_every=4, inv_diag=s.inv_diag)
    with pytest.raises(E.EhybError) as ei:
        s.plan.bicgstab_multi(B, X0, **run)
    assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value) and "ehyb_bicgstab_multi" in str(ei.value)
    X, it, rel = s.plan.bicgstab_multi(B, X0, allow_breakdown=True, **run)
    for j in (1, 2):
        assert it[j] == 0 and rel[j] == 0.0, (j, it[j], rel[j])
        assert np.array_equal(X[j].view(np.int64), X0[j].view(np.int64)), j
    assert it[3] == 0 and np.isnan(rel[3])
    assert np.array_equal(X[3].view(np.int64), X0[3].view(np.int64))
    live = [0, 4]
    assert (it[live] > 0).all() and (rel[live] <= 1e-12).all(), (it, rel)
    assert_same_bits((X[live], it[live], rel[live]), singles(s.plan, B[live], X0[live], **run), "ordinary columns")


def test_exact_breakdown_beside_an_exact_half_step(E, gpu):
    """A: the cyclic shift, no preconditioner.  b = e_k: r^.(A r^) is exactly 0, a breakdown before any update.  b = ones:
    v = A p^ = ones, alpha = 1, s = 0 exactly -- the half step x += p^ solves it"""
    n = 20000
    A = sp.csr_matrix((np.ones(n), (np.arange(n), (np.arange(n) + 1) % n)), shape=(n, n))
    s = System(E, A, lds_doubles=2048, sym_pairs=0)
    b = np.zeros(n)
    b[1234] = 1.0
    B = np.stack([E.vector_reorder(b, s.perm), np.ones(n)])
    with pytest.raises(E.EhybError) as ei:
        s.plan.bicgstab_multi(B, max_iter=50, rtol=1e-10)
    assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value)
    X, it, rel = s.plan.bicgstab_multi(B, max_iter=50, rtol=1e-10, allow_breakdown=True)
    assert it[0] == 0 and rel[0] == 1.0, (it, rel)
    assert np.array_equal(X[0].view(np.int64), np.zeros(n).view(np.int64))
    assert it[1] == 1 and rel[1] == 0.0, (it, rel)
    assert np.array_equal(X[1].view(np.int64), np.ones(n).view(np.int64))


def test_leading_dimensions_leave_the_gaps_alone(E, gpu):
    s = System(E, cd_matrix(100, 90, 2000, 13), lds_doubles=2048, sym_pairs=0)
    n, k = s.n, 3
    B = rhs_bank(E, s, k, seed=5)
    ldb, ldx = n + 37, n + 5
    Bb = np.full((k, ldb), -7.25)
    Bb[:, :n] = B
    Xb = np.full((k, ldx), 1e300)
    Xb[:, :n] = 0.0
    db, dx = E.DeviceBuffer(k * ldb).upload(Bb.ravel()), E.DeviceBuffer(k * ldx).upload(Xb.ravel())
    dd = E.DeviceBuffer(n).upload(s.inv_diag)
    lib = E.host._lib.load()
    it = (C.c_int * k)()
    rel = (C.c_double * k)()
    args = (s.plan.h, C.c_void_p(dd.ptr), C.c_void_p(db.ptr), ldb, C.c_void_p(dx.ptr), ldx, k, 500, 1e-10, 6, None)
    assert lib.ehyb_bicgstab_multi(*args, it, rel) == 0, lib.ehyb_last_error()
    Xo = dx.download().reshape(k, ldx)
    assert np.array_equal(db.download().reshape(k, ldb).view(np.int64), Bb.view(np.int64))
    assert (Xo[:, n:] == 1e300).all()
    want = s.plan.bicgstab_multi(B, max_iter=500, rtol=1e-10, check_every=6, inv_diag=s.inv_diag)
    assert (want[1] > 0).all()
    assert_same_bits((Xo[:, :n], np.array(list(it)), np.array(list(rel))), want, "ld > n")
    # NULL outputs are allowed
    dx.upload(Xb.ravel())
    assert lib.ehyb_bicgstab_multi(*args, None, None) == 0, lib.ehyb_last_error()
    assert np.array_equal(dx.download().reshape(k, ldx).view(np.int64), np.concatenate([want[0], Xb[:, n:]], axis=1).view(np.int64))


FREE_ORDER = [
    ("panel-residual", lambda E, kw: panel_matrix(E, E.make_config(**kw)),
     dict(partitioner=1, er_mode=2, er_panel_cols=4096, lds_doubles=4096), lambda st: st["er_partials"] > 0),
    ("symmetric-pairs", lambda E, kw: cd_matrix(120, 100, 600, 4, calm=0.5, shift=1.0),
     dict(lds_doubles=2048, sym_pairs=1, direct=2), lambda st: st["sym_pairs"] > 0),
]


@pytest.mark.parametrize("name,make,kw,taken", FREE_ORDER, ids=[s[0] for s in FREE_ORDER])
def test_where_the_summation_order_is_free(E, gpu, name, make, kw, taken):
    """the matrices, right-hand sides and bounds of test_gpu_bicgstab.test_plan_shapes_against_cpu_and_scipy, four columns wide:
    its two right-hand sides and the same two times a power of two (the same solve, scaled exactly)"""
    A = make(E, kw)
    assert abs(A - A.T).nnz > 0, "the system must be unsymmetric"
    s = System(E, A, **kw)
    assert taken(s.plan.stats), (name, s.plan.stats)
    assert s.plan.spmm_max_k == 4, s.plan.spmm_max_k
    n = s.n
    rng = np.random.default_rng(7)
    rtol = 1e-9
    b0, b1 = A @ np.sin(np.arange(n) * 0.01) + 0.1, rng.uniform(-1, 1, n)
    bs = [b0, b1, 0.5 * b0, -2.0 * b1]
    X, its, rels = s.plan.bicgstab_multi(np.stack([E.vector_reorder(b, s.perm) for b in bs]), max_iter=2000, rtol=rtol, check_every=4,
                                         inv_diag=s.inv_diag)
    lu = spla.splu(A.tocsc())
    cpu = {}
    for j, b in enumerate(bs):
        x, it, rel = E.vector_recover(X[j], s.perm), its[j], rels[j]
        assert 0 < it and rel <= rtol, (name, j, it, rel)
        assert np.linalg.norm(b - A @ x) <= 10 * rtol * np.linalg.norm(b), (name, j)
        if j < 2:
            cpu[j] = cpu_bicgstab(A, b, max_iter=2000, rtol=rtol, dinv=1.0 / A.diagonal())[1:]
        it_cpu, rel_cpu, status = cpu[j % 2]
        assert status == "converged" and abs(it - it_cpu) <= 5, (name, j, it, it_cpu, rel, rel_cpu)
        x_ref = lu.solve(b)
        assert np.linalg.norm(x - x_ref) <= 1e-6 * np.linalg.norm(x_ref), (name, j, np.linalg.norm(x - x_ref))
