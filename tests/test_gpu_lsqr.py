"""ehyb_lsqr / ehyb_lsqr_multi: LSQR on the device for least-squares problems on A and A^T.

The systems are lsqr_cases.systems(): every one has 1,440 rows once padded square, so a plan with lds_doubles = 256 has several
partitions.  lsqr_cases.cpu_lsqr restates the device's recurrences, stop and breakdown rules in numpy (test_lsqr_host.py holds it
against scipy); the device must end the same way within one iteration and agree in x, and x must be what the problem asks for
(numpy's lstsq, the normal equations, the minimum-norm solution).  With a plan of A^T in plain storage the device's order of
summation is fixed, so x and every field of info are the same bits whatever check_every, graph use or stream, and column j of a
k-column solve is the one-vector solve of b_j.  Vectors go in and out in the original numbering unless said otherwise."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import lsqr_cases as lc

pytestmark = pytest.mark.gpu

ERR_ARG = 1
PLAIN = dict(window_mode=2, lds_doubles=256, direct=2, sym_pairs=2)
TOL = dict(atol=1e-10, btol=1e-10)


class System:
    """a padded square matrix, its plan, and the plan of its transpose in the same numbering"""

    def __init__(self, E, Asq, symmetric=False, **kw):
        self.A = Asq.tocsr()
        self.n = self.A.shape[0]
        self.cfg = E.make_config(**kw)
        self.m = E.Matrix.from_csr(self.A.indptr, self.A.indices, self.A.data, self.cfg, symmetric=symmetric)
        self.m.reorder(self.cfg)
        self.perm = self.m.reorder_list.copy()
        self.parts = len(self.m.part_boundary) - 1
        self.plan = E.Plan(self.m, self.cfg)
        if symmetric:
            self.mt, self.plan_t = None, self.plan
        else:
            self.mt = self.m.transposed_like(self.cfg)
            self.plan_t = E.Plan(self.mt, E.make_config(**dict(kw, sym_pairs=2)))

    def solve(self, E, b, transposed="plan", x0=None, plan=None, **kw):
        """b, x0 in the original numbering -> (x in the original numbering, info)"""
        x, info = (plan or self.plan).lsqr(E.vector_reorder(b, self.perm), plan_t=self.plan_t if transposed == "plan" else None,
                                           x0=None if x0 is None else E.vector_reorder(x0, self.perm), **kw)
        return E.vector_recover(x, self.perm), info


@pytest.fixture(scope="module")
def cases():
    """the six systems and, per system, the restatement's answer -- computed once"""
    out = lc.systems()
    for s in out.values():
        s["x_cpu"], s["info_cpu"] = lc.cpu_lsqr(s["Asq"], s["b"], damp=s["damp"], max_iter=1000, **TOL)
    T = out["b"]["A"].toarray()
    out["b"]["x_ref"] = np.linalg.lstsq(T, out["b"]["b"], rcond=None)[0]
    out["c"]["x_ref"] = np.linalg.solve(T.T @ T + 0.25 * np.eye(lc.M_COLS), T.T @ out["c"]["b"])
    out["d"]["x_ref"] = np.linalg.pinv(T.T) @ out["d"]["b"][:lc.M_COLS]
    out["a"]["x_ref"] = np.linalg.solve(out["a"]["A"].toarray(), out["a"]["b"])
    return out


_built = {}


def system_of(E, cases, name):
    key = "b" if name == "c" else "a" if name == "f" else name       # (c) is (b) damped, (f) is (a) with b = 0
    if key not in _built:
        _built[key] = System(E, cases[key]["Asq"], **PLAIN)
        assert _built[key].parts >= 4, (key, _built[key].parts)
    return _built[key]


@pytest.fixture(scope="module")
def plain(E, gpu, cases):
    return system_of(E, cases, "a")


def rel_err(x, want):
    return np.linalg.norm(x - want) / np.linalg.norm(want)


# ------------------------------------------------------------------ (a) - (d), with a plan of A^T and with ehyb_spmv_t
@pytest.mark.parametrize("transposed", ["plan", "spmv_t"])
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_against_the_restatement_and_the_direct_answer(E, gpu, cases, name, transposed):
    c = cases[name]
    s = system_of(E, cases, name)
    m, n = c["shape"]
    x, info = s.solve(E, c["b"], transposed=transposed, damp=c["damp"], max_iter=1000, check_every=4, **TOL)
    cpu = c["info_cpu"]
    err_cpu, err_ref = rel_err(x, c["x_cpu"]), rel_err(x[:n], c["x_ref"])
    print(name, transposed, "device", info, "cpu", cpu, "error against cpu_lsqr", err_cpu, "against the direct answer", err_ref)
    assert info["istop"] == cpu["istop"] == {"a": 1, "b": 2, "c": 2, "d": 1}[name], (info, cpu)
    assert abs(info["iters"] - cpu["iters"]) <= 1, (info, cpu)
    assert err_cpu <= 1e-9, err_cpu
    assert err_ref <= 1e-8, err_ref
    assert np.array_equal(x[n:].view(np.int64), np.zeros(lc.N - n).view(np.int64)), "the padded entries of x must be +0.0"
    if info["iters"] == cpu["iters"]:        # (arnorm ends at rounding level)
        for key in ("rnorm", "anorm", "xnorm"):
            assert abs(info[key] - cpu[key]) <= 1e-6 * abs(cpu[key]), (key, info, cpu)


def test_a_diagonal_of_two_values_needs_exactly_two_iterations(E, gpu, cases):
    """(e): two distinct singular values: the bidiagonalisation ends after two steps"""
    c = cases["e"]
    s = System(E, c["Asq"], symmetric=True, **PLAIN)
    for transposed in ("plan", "spmv_t"):
        x, info = s.solve(E, c["b"], transposed=transposed, max_iter=50, **TOL)
        assert info["iters"] == 2 and info["istop"] in (1, 2), info
        assert rel_err(x, c["b"] / c["A"].diagonal()) <= 1e-12


def test_zero_b_is_istop_0_and_x_is_untouched(E, gpu, cases, plain):
    """(f), and alpha_1 = 0: b in the null space of A^T"""
    x, info = plain.solve(E, np.zeros(lc.N), **TOL)
    assert info["istop"] == 0 and info["iters"] == 0 and info["rnorm"] == 0.0, info
    assert np.array_equal(x.view(np.int64), np.zeros(lc.N).view(np.int64))
    # (d) is 600 x 1,440 padded with empty rows: a b that lives in the padded rows only has A^T b = 0
    s = system_of(E, cases, "d")
    b = np.zeros(lc.N)
    b[lc.M_COLS:] = 1.0
    x, info = s.solve(E, b, **TOL)
    assert info["istop"] == 0 and info["iters"] == 0 and info["rnorm"] == np.sqrt(lc.N - lc.M_COLS) and info["arnorm"] == 0.0, info
    assert np.array_equal(x.view(np.int64), np.zeros(lc.N).view(np.int64))


def test_max_iter_and_a_start_that_already_solves(E, gpu, cases, plain):
    c = cases["a"]
    x, info = plain.solve(E, c["b"], max_iter=0, **TOL)
    assert info["istop"] == 7 and info["iters"] == 0 and not x.any() and info["rnorm"] == pytest.approx(np.linalg.norm(c["b"]), rel=1e-14), info
    x, info = plain.solve(E, c["b"], max_iter=5, **TOL)
    assert info["istop"] == 7 and info["iters"] == 5, info
    # bnorm is the norm of the FIRST residual, so at the start test 1 reads beta_1 <= btol beta_1: it holds from btol = 1 on
    x0 = np.linspace(-1, 1, lc.N)
    x, info = plain.solve(E, c["b"], x0=x0, atol=0.0, btol=1.0)
    assert info["iters"] == 0 and info["istop"] == 1 and np.array_equal(x.view(np.int64), x0.view(np.int64)), info
    # x0 != 0 reaches the same answer
    x, info = plain.solve(E, c["b"], x0=np.random.default_rng(4).uniform(-1, 1, lc.N), **TOL)
    assert info["istop"] == 1 and rel_err(x, c["x_ref"]) <= 1e-8, info


def test_a_symmetric_pair_plan_runs_with_plan_t_equal_to_plan(E, gpu):
    """plan_t == plan is the caller's statement that A is symmetric; plan_t = None is refused on pair storage"""
    A0 = lc.convection()
    A = ((A0 + A0.T) * 0.5).tocsr()                                         # symmetric: diagonal 5, every coupling -1
    b = A @ np.cos(np.arange(lc.N) * 0.02)
    s = System(E, A, symmetric=True, window_mode=2, lds_doubles=256, direct=2, sym_pairs=1)
    assert s.plan.stats["sym_pairs"] > 0.25 * A.nnz and s.plan_t is s.plan
    x, info = s.solve(E, b, max_iter=3000, **TOL)
    x_cpu, cpu = lc.cpu_lsqr(A, b, max_iter=3000, **TOL)
    print("device", info, "cpu", cpu, "error", rel_err(x, x_cpu))
    assert info["istop"] == cpu["istop"] and info["istop"] in (1, 2) and abs(info["iters"] - cpu["iters"]) <= max(1, 0.03 * cpu["iters"]), (info, cpu)
    assert np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b)
    with pytest.raises(E.EhybError) as ei:
        s.solve(E, b, transposed="spmv_t")
    assert ei.value.code == ERR_ARG and "ehyb_spmv_t: not built for" in str(ei.value)


# ------------------------------------------------------------------ bit identity
def _same_bits(got, want, what):
    (x, info), (xw, infow) = got, want
    assert info["istop"] == infow["istop"] and info["iters"] == infow["iters"], (what, info, infow)
    for key in ("rnorm", "arnorm", "anorm", "xnorm"):
        assert np.array_equal(np.array([info[key]]), np.array([infow[key]]), equal_nan=True), (what, key, info, infow)
    assert np.array_equal(x.view(np.int64), xw.view(np.int64)), (what, np.abs(x - xw).max())


@pytest.mark.parametrize("max_iter", [1000, 23], ids=["converges", "max-iter-odd"])
def test_plain_storage_is_exact_for_every_check_every_graph_and_stream(E, gpu, cases, max_iter):
    c = cases["c"]
    s = system_of(E, cases, "c")
    launches = E.Plan(s.m, E.make_config(graphs=2, **PLAIN))
    b = E.vector_reorder(c["b"], s.perm)
    run = dict(plan_t=s.plan_t, damp=c["damp"], max_iter=max_iter, **TOL)
    ref = s.plan.lsqr(b, check_every=1, **run)
    assert ref[1]["iters"] > 0 and (ref[1]["istop"] == 2) == (max_iter == 1000), ref[1]
    if max_iter == 23:
        assert ref[1]["iters"] == 23 and ref[1]["istop"] == 7
    for check_every in (2, 10, 1000):
        _same_bits(s.plan.lsqr(b, check_every=check_every, **run), ref, f"check_every={check_every}")
        _same_bits(launches.lsqr(b, check_every=check_every, **run), ref, f"graphs=2 check_every={check_every}")
    _same_bits(launches.lsqr(b, check_every=1, **run), ref, "graphs=2 check_every=1")
    st = E.Stream()
    try:
        _same_bits(s.plan.lsqr(b, check_every=10, stream=st.ptr, **run), ref, "user stream")
    finally:
        st.destroy()
    _same_bits(s.plan.lsqr(b, check_every=1, **run), ref, "second run")


# ------------------------------------------------------------------ breakdown, the C ABI, refusals
def test_nan_in_b_is_a_breakdown_and_x_stays(E, gpu, plain):
    s = plain
    rng = np.random.default_rng(12)
    b = rng.uniform(-1, 1, s.n)
    b[s.n // 3] = np.nan
    x0 = rng.uniform(-1, 1, s.n)
    for plan_t in (s.plan_t, None):
        with pytest.raises(E.EhybError) as ei:
            s.plan.lsqr(b, plan_t=plan_t, x0=x0)
        assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value)
        x, info = s.plan.lsqr(b, plan_t=plan_t, x0=x0, allow_breakdown=True)
        assert info["istop"] == -1 and info["iters"] == 0 and np.isnan(info["rnorm"]), info
        assert np.array_equal(x.view(np.int64), x0.view(np.int64))
    x0[5] = np.nan
    x, info = s.plan.lsqr(rng.uniform(-1, 1, s.n), plan_t=s.plan_t, x0=x0, allow_breakdown=True)
    assert info["istop"] == -1 and info["iters"] == 0 and np.array_equal(x.view(np.int64), x0.view(np.int64))


def test_null_info_and_the_c_abi(E, gpu, cases, plain):
    s = plain
    b = E.vector_reorder(cases["a"]["b"], s.perm)
    want = s.plan.lsqr(b, plan_t=s.plan_t, **TOL)
    db, dx = E.DeviceBuffer(s.n).upload(b), E.DeviceBuffer(s.n).upload(np.zeros(s.n))
    lib = E.host._lib.load()
    assert lib.ehyb_lsqr(s.plan.h, s.plan_t.h, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), 0.0, 1e-10, 1e-10, 1000, 10, None, None) == 0
    assert np.array_equal(dx.download().view(np.int64), want[0].view(np.int64))
    assert np.array_equal(db.download(), b)


def test_a_plan_t_of_another_dimension_is_refused(E, gpu, plain):
    other = System(E, lc.convection(20, 18), **PLAIN)
    b = np.ones(plain.n)
    for multi in (False, True):
        with pytest.raises(E.EhybError) as ei:
            (plain.plan.lsqr_multi if multi else plain.plan.lsqr)(b, plan_t=other.plan)
        assert ei.value.code == ERR_ARG and "plan_t has 360 rows" in str(ei.value)


# ------------------------------------------------------------------ k columns
def column_mix(E, s, c):
    """ordinary, early-converging (b = A v with v close to the first right singular vector: a Krylov space of about one
    dimension), zero, NaN, ordinary"""
    n = s.n
    rng = np.random.default_rng(3)
    nan = c["b"].copy()
    nan[7] = np.nan
    v = np.ones(n)
    for _ in range(300):                                             # the power method on A^T A
        v = c["A"].T @ (c["A"] @ v)
        v /= np.linalg.norm(v)
    B = [c["b"], c["A"] @ v, np.zeros(n), nan, rng.uniform(-1, 1, n)]
    X0 = [np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), rng.uniform(-1, 1, n)]
    return np.stack([E.vector_reorder(b, s.perm) for b in B]), np.stack([E.vector_reorder(x, s.perm) for x in X0])


def info_tuple(info):
    return tuple(info[k] for k in ("istop", "iters", "rnorm", "arnorm", "anorm", "xnorm"))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_every_column_of_a_multi_solve_is_the_single_solve(E, gpu, cases, plain, k):
    """k = 5: launches 3 + 2 columns wide.  The NaN column (from k = 4 on) breaks down at the start, the zero column and the early
    one stop before the others; each finite column is ehyb_lsqr on it, bit for bit."""
    s = plain
    B, X0 = column_mix(E, s, cases["a"])
    run = dict(plan_t=s.plan_t, max_iter=1000, atol=1e-6, btol=1e-6, check_every=4)
    if k >= 4:
        with pytest.raises(E.EhybError) as ei:
            s.plan.lsqr_multi(B[:k], X0=X0[:k], **run)
        assert ei.value.code == ERR_ARG and "breakdown in column 3" in str(ei.value)
    X, infos = s.plan.lsqr_multi(B[:k], X0=X0[:k], allow_breakdown=True, **run)
    print("k", k, [(i["istop"], i["iters"]) for i in infos])
    for j in range(k):
        if j == 3:
            assert infos[j]["istop"] == -1 and infos[j]["iters"] == 0 and np.array_equal(X[j], X0[j])
            continue
        _same_bits((X[j], infos[j]), s.plan.lsqr(B[j], x0=X0[j], **run), f"k={k} column {j}")
    assert infos[0]["istop"] == 1 and infos[0]["iters"] > 0
    if k >= 3:
        assert infos[2]["istop"] == 0 and infos[2]["iters"] == 0 and 0 < infos[1]["iters"] < infos[0]["iters"], infos
    # with ehyb_spmv_t the transposed side runs column by column: the same answers up to the order of summation
    if k == 3:
        Xs, infos_s = s.plan.lsqr_multi(B[:k], X0=X0[:k], **dict(run, plan_t=None))
        for j in (0, 1):
            assert abs(infos_s[j]["iters"] - infos[j]["iters"]) <= 1 and rel_err(Xs[j], X[j]) <= 1e-5, (j, infos_s[j], infos[j])


def test_multi_with_leading_dimensions(E, gpu, cases, plain):
    from ehyb_spmv_gpu_amd import _lib

    s, n, k = plain, plain.n, 3
    B, X0 = column_mix(E, s, cases["a"])
    ldb, ldx = n + 37, n + 5
    Bb = np.full((k, ldb), -7.25)
    Bb[:, :n] = B[:k]
    Xb = np.full((k, ldx), -6.02214076e23)
    Xb[:, :n] = X0[:k]
    db, dx = E.DeviceBuffer(k * ldb).upload(Bb.ravel()), E.DeviceBuffer(k * ldx).upload(Xb.ravel())
    info = (_lib.LsqrInfo * k)()
    lib = E.host._lib.load()
    rc = lib.ehyb_lsqr_multi(s.plan.h, s.plan_t.h, C.c_void_p(db.ptr), ldb, C.c_void_p(dx.ptr), ldx, k, 0.0, 1e-6, 1e-6, 1000, 4, None, info)
    assert rc == 0, lib.ehyb_last_error()
    Xo = dx.download().reshape(k, ldx)
    assert np.array_equal(Xo[:, n:].view(np.int64), Xb[:, n:].view(np.int64)), "the gap behind the columns of X"
    for j in range(k):
        want = s.plan.lsqr(B[j], plan_t=s.plan_t, x0=X0[j], max_iter=1000, atol=1e-6, btol=1e-6, check_every=4)
        _same_bits((Xo[j, :n].copy(), info[j].as_dict()), want, f"column {j}")


# ------------------------------------------------------------------ past the unrolled loops in a composed solve
BIG_NX, BIG_NY = 725, 724             # 524,900 rows > 4 * 131,072: every thread of the vector kernels runs an unrolled trip
NEVER = 1e-150


def test_six_iterations_past_the_unrolled_loops(E, gpu):
    """the convection stencil at 524,900 rows, six iterations at tolerances that never stop, every iterate against cpu_lsqr: an
    indexing error is O(1), six iterations of rounding stay near 1e-15.  Then 4 columns wide: each column is the single solve,
    bit for bit, where the K-wide kernels run their unrolled bodies."""
    import solver_cases as sc

    n = BIG_NX * BIG_NY
    A = lc.convection(BIG_NX, BIG_NY)
    s = System(E, A, lds_doubles=5120, direct=2, sym_pairs=2)
    for p in (s.plan, s.plan_t):
        assert p.stats["sym_pairs"] == 0 and p.stats["er_partials"] == 0
        assert (p.array("er_seg_row") >= 0).all(), "no residual row may be split into segments"
    assert n >= 4 * sc.S + 1 and sc.solver_grid(n) == sc.STEP_GRID
    assert {(1, 0), (1, 1)} <= sc.walk_profile(n, sc.STEP_GRID)
    rng = np.random.default_rng(9)
    B = rng.uniform(-1, 1, (4, n))
    never = dict(atol=NEVER, btol=NEVER)
    for j, damp in ((0, 0.0), (1, 0.75)):
        iterates = []
        _, cpu = lc.cpu_lsqr(A, B[j], damp=damp, max_iter=6, iterates=iterates, **never)
        assert cpu["iters"] == 6 and cpu["istop"] == 7 and len(iterates) == 6
        for it in range(1, 7):
            x, info = s.solve(E, B[j], damp=damp, max_iter=it, **never)
            err = rel_err(x, iterates[it - 1])
            print("damp", damp, "iterate", it, "error against cpu_lsqr", err)
            assert info["iters"] == it and info["istop"] == 7 and err <= 1e-12, (it, info, err)
        for key in ("rnorm", "arnorm", "anorm", "xnorm"):
            assert abs(info[key] - cpu[key]) <= 1e-12 * abs(cpu[key]), (key, info, cpu)
    Bp = np.stack([E.vector_reorder(b, s.perm) for b in B])
    run = dict(plan_t=s.plan_t, damp=0.75, max_iter=6, **never)
    singles = [s.plan.lsqr(Bp[j], **run) for j in range(4)]
    X, infos = s.plan.lsqr_multi(Bp, **run)
    for j in range(4):
        _same_bits((X[j], infos[j]), singles[j], f"k=4 column {j}")
