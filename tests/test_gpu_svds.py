"""ehyb_svds: thick-restart Golub-Kahan-Lanczos bidiagonalisation on the device for the largest singular triplets of a plan.

The systems are svds_cases.systems(): the matrices of lsqr_cases.py (1,440 rows once padded square, several partitions with
lds_doubles = 256) and a few small ones on which a cycle ends early.  cpu_svds restates the solver's rules in numpy
(test_svds_host.py holds it against dense singular values); the device must agree with it to two cycles' worth of multiplies, reach
the true residuals, and agree with the dense singular values.  With s0 the largest returned value and tol = 1e-10 (the margins of
test_gpu_eigsh.py):
    |sigma_i - dense_i|                         <= 10 tol s0
    ||A v_i - sigma_i u_i||, ||A^T u_i - sigma_i v_i||  <= 10 tol s0     the rule bounds the estimate of the second by tol s0
    max |U U^T - I|, max |V V^T - I|            <= 1e-12                 cpu_svds leaves <= 2e-14 on every input here
    multiplies                                  within 4 (m - keep) of cpu_svds
On the collapse cases the counts are exact: svds_cases keeps every deciding ratio of theirs above 2^-60 or below 2^-100, and the
start vector is handed over so that the device runs the restatement's problem and not a permutation of it.  With a plan of A^T in
plain storage every output is the same bits from run to run, for graphs and plain launches, for a given and a private stream.
Vectors go in and out in the original numbering unless said otherwise."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import eigsh_cases as ec
import lsqr_cases as lc
import svds_cases as sv

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 8
TOL = 1e-10
PLAIN = dict(window_mode=2, lds_doubles=256, direct=2, sym_pairs=2)
SMALL = dict(direct=1, sym_pairs=2)
_dp = C.POINTER(C.c_double)
COUNTS = ("found", "nconv", "multiplies", "restarts")


class System:
    """a square (padded) matrix, its plan, and the plan of its transpose in the same numbering"""

    def __init__(self, E, A, symmetric=False, **kw):
        self.E = E
        self.A = A.tocsr()
        self.n = self.A.shape[0]
        self.kw = kw
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

    def svds(self, nsv, arm="plan", v0=None, plan=None, **kw):
        """v0 in the original numbering -> (s, U, V (found, n) in the original numbering, info)"""
        E = self.E
        s, U, V, info = (plan or self.plan).svds(nsv, plan_t=self.plan_t if arm == "plan" else None,
                                                 v0=None if v0 is None else E.vector_reorder(v0, self.perm), **kw)
        back = lambda X: None if X is None else np.array([E.vector_recover(x, self.perm) for x in X]).reshape(len(X), self.n)  # noqa: E731
        return s, back(U), back(V), info


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def dense_of(name, A):
    return cached(("dense", name), lambda: np.linalg.svd(A.toarray(), compute_uv=False))


PLAN_OF = {"convection-4": "convection", "convection-1": "convection", "convection-8-24": "convection", "tall-6": "tall", "tall-16-40": "tall",
           "tall-T-6": "tall-T"}


def system_of(E, name, A):
    """the System of a matrix, built once -> (System, its key for dense_of)"""
    key = PLAN_OF.get(name, name)
    return cached(("system", key), lambda: System(E, A, **(PLAIN if A.shape[0] > 100 else SMALL))), key


def check(what, A, got, nsv, dense, tol=TOL, cpu=None, basis=0, as_set=False):
    """the assertions of the module docstring; -> info.  as_set: every value is compared with the nearest dense one and the first
    with the first -- for a matrix with multiple singular values, of which a run finds one copy and rounding may bring in another"""
    s, U, V, info = got
    want = len(s)
    s0 = s[0]
    err = max(np.abs(s[:, None] - dense[None, :]).min(axis=1).max(), abs(s0 - dense[0])) if as_set else np.abs(s - dense[:want]).max()
    right = max(np.linalg.norm(A @ V[i] - s[i] * U[i]) for i in range(want))
    left = max(np.linalg.norm(A.T @ U[i] - s[i] * V[i]) for i in range(want))
    ou, ov = np.abs(U @ U.T - np.eye(want)).max(), np.abs(V @ V.T - np.eye(want)).max()
    print(what, "device", [info[k] for k in COUNTS], f"err/s0 {err / s0:.2e} right/s0 {right / s0:.2e} left/s0 {left / s0:.2e} orth {ou:.1e} {ov:.1e}")
    assert info["status"] == "ok" and info["found"] == want, (what, info)
    assert (np.diff(s) <= 0).all(), (what, s)
    assert err <= 10 * tol * s0, (what, err / s0)
    assert right <= 10 * tol * s0 and left <= 10 * tol * s0, (what, right / s0, left / s0)
    assert ou <= 1e-12 and ov <= 1e-12, (what, ou, ov)
    if cpu is not None:
        m, keep = ec.resolve_basis(nsv, basis, A.shape[0])
        print(what, "cpu", [cpu[k] for k in COUNTS])
        assert cpu["status"] == "ok" and info["nconv"] == cpu["nconv"] == want, (what, info, cpu)
        assert abs(info["multiplies"] - cpu["multiplies"]) <= 4 * (m - keep), (what, info["multiplies"], cpu["multiplies"])
    return info


SYSTEMS = sv.systems()
LARGE = [n for n in SYSTEMS if n not in sv.COLLAPSE_SYSTEMS]


@pytest.mark.parametrize("arm", ["plan", "spmv_t"])
@pytest.mark.parametrize("name", LARGE + ["repeated-diagonal"])
def test_against_the_restatement_and_dense_values(E, gpu, name, arm):
    c = SYSTEMS[name]
    A, nsv, basis = c["A"], c["nsv"], c["basis"]
    s, key = system_of(E, name, A)
    if A.shape[0] > 100:
        assert s.parts >= 4, s.parts
    cpu = cached(("cpu", name), lambda: sv.cpu_svds(A, nsv, basis=basis, tol=TOL)[3])
    assert (cpu["multiplies"], cpu["restarts"], cpu["collapse"]) == c["expect"]
    # repeated-diagonal has seven distinct values among sixteen: an exact run would end at j = 6; in fp64 beta^2 there is 2^-62 of
    # its column, far above the collapse threshold, and the run goes on through noise vectors until they collapse -- the count is
    # rounding's, within the allowance, and so is whether a second copy of 5 shows
    check(f"{name} {arm}", A, s.svds(nsv, arm=arm, basis=basis, tol=TOL), nsv, dense_of(key, A), cpu=cpu, basis=basis,
          as_set=name == "repeated-diagonal")


def test_a_symmetric_matrix_with_plan_t_equal_to_plan(E, gpu):
    """plan_t == plan is the caller's statement that A is symmetric, the only way onto symmetric pair storage (plan_t = None is
    refused there); the singular values are the largest |lambda|"""
    A = ec.sym_grid(24, 20, 1)
    s = System(E, A, symmetric=True, window_mode=2, lds_doubles=256, direct=2, sym_pairs=1)
    assert s.plan.stats["sym_pairs"] > 0 and s.plan_t is s.plan
    lam = np.sort(np.abs(np.linalg.eigvalsh(A.toarray())))[::-1]
    cpu = sv.cpu_svds(A, 4, tol=TOL)[3]
    got = s.svds(4, tol=TOL)
    check("symmetric pairs", A, got, 4, lam, cpu=cpu)
    assert np.abs(got[0] - lam[:4]).max() <= 10 * TOL * lam[0]
    with pytest.raises(E.EhybError) as ei:
        s.svds(4, arm="spmv_t")
    assert ei.value.code == ERR_ARG and "ehyb_spmv_t" in str(ei.value)


EXACT = {"wide-7x30": (3, 3, 15, 0), "wide-T": (3, 3, 16, 0), "identity": (1, 1, 2, 0), "zero": (0, 0, 1, 0)}


@pytest.mark.parametrize("arm", ["plan", "spmv_t"])
@pytest.mark.parametrize("name", list(EXACT))
def test_a_collapse_ends_the_cycle_with_exact_counts(E, gpu, name, arm):
    c = SYSTEMS[name]
    A, nsv = c["A"], c["nsv"]
    s, _ = system_of(E, name, A)
    got = s.svds(nsv, arm=arm, v0=ec.start_vector(A.shape[0]), tol=TOL)
    info = got[3]
    print(name, arm, info)
    assert tuple(info[k] for k in COUNTS) == EXACT[name] and info["status"] == "ok", (name, info)
    if name == "zero":
        assert len(got[0]) == 0 and got[1].shape == (0, 6) and got[2].shape == (0, 6) and len(info["resid"]) == 0
        return
    assert (info["resid"] == 0).all(), info
    check(name, A, got, nsv, np.linalg.svd(A.toarray(), compute_uv=False))


def test_nsv_beyond_the_rank_found_returns_fewer(E, gpu):
    """7 x 30: the left collapse leaves seven triplets whatever nsv asks for"""
    A = SYSTEMS["wide-7x30"]["A"]
    s, _ = system_of(E, "wide-7x30", A)
    got = s.svds(10, v0=ec.start_vector(30), tol=TOL)
    assert tuple(got[3][k] for k in COUNTS) == (7, 7, 15, 0), got[3]
    check("nsv 10 of rank 7", A, got, 10, np.linalg.svd(A.toarray(), compute_uv=False))


def test_one_and_two_rows(E, gpu):
    s = System(E, sp.csr_matrix(np.array([[-3.5]])), **SMALL)
    for arm in ("plan", "spmv_t"):
        sg, U, V, info = s.svds(2, arm=arm)
        assert tuple(info[k] for k in COUNTS) == (1, 1, 2, 0), info
        assert sg.tolist() == [3.5] and np.abs(U).tolist() == [[1.0]] and np.abs(V).tolist() == [[1.0]] and U[0, 0] * V[0, 0] == -1.0
    A = sp.csr_matrix(np.array([[2.0, 1.0], [-1.0, 3.0]]))
    s = System(E, A, **SMALL)
    for arm in ("plan", "spmv_t"):
        got = s.svds(2, arm=arm)
        assert tuple(got[3][k] for k in COUNTS) == (2, 2, 4, 0), got[3]
        check("n=2", A, got, 2, np.linalg.svd(A.toarray(), compute_uv=False))


def test_the_smallest_legal_basis_and_the_largest_nsv(E, gpu):
    """basis = nsv + 2: keep = nsv + 1, one step per cycle, every restart with kk = keep: multiplies = 2 (nsv + 2) + 2 restarts.
    nsv = 16 with basis = 64 on the tall matrix."""
    A = SYSTEMS["wide-T"]["A"]
    s, _ = system_of(E, "wide-T", A)
    dense = np.linalg.svd(A.toarray(), compute_uv=False)
    cpu = sv.cpu_svds(A, 2, basis=4, tol=TOL)[3]
    info = check("basis=4", A, s.svds(2, basis=4, tol=TOL), 2, dense, cpu=cpu, basis=4)
    assert info["restarts"] > 3 and info["multiplies"] == 2 * 4 + 2 * info["restarts"], info
    A = SYSTEMS["tall-6"]["A"]
    s, key = system_of(E, "tall-6", A)
    cpu = sv.cpu_svds(A, 16, basis=64, tol=TOL)[3]
    info = check("nsv=16 basis=64", A, s.svds(16, basis=64, tol=TOL), 16, dense_of(key, A), cpu=cpu, basis=64)
    assert info["restarts"] >= 1, info


def test_max_restarts_exhausted(E, gpu):
    """found = nsv, nconv < nsv, multiplies exactly 2 m and 2 m + 3 * 2 (m - keep); U and V are still orthonormal"""
    A = SYSTEMS["convection-4"]["A"]
    s, _ = system_of(E, "convection-4", A)
    m, keep = ec.resolve_basis(4, 0, s.n)
    for max_restarts, mult in ((0, 2 * m), (3, 2 * m + 3 * 2 * (m - keep))):
        sg, U, V, info = s.svds(4, max_restarts=max_restarts, tol=TOL)
        assert info["found"] == 4 and info["nconv"] < 4 and info["multiplies"] == mult and info["restarts"] == max_restarts, info
        assert info["resid"][info["nconv"]] > TOL * sg[0]
        assert U.shape == V.shape == (4, s.n)
        assert np.abs(U @ U.T - np.eye(4)).max() <= 1e-12 and np.abs(V @ V.T - np.eye(4)).max() <= 1e-12


def _same_bits(got, want, what, vectors=True):
    s, U, V, info = got
    sw, Uw, Vw, infow = want
    assert [info[k] for k in COUNTS] == [infow[k] for k in COUNTS], (what, info, infow)
    assert np.array_equal(s.view(np.int64), sw.view(np.int64)), (what, s, sw)
    assert np.array_equal(info["resid"].view(np.int64), infow["resid"].view(np.int64)), (what, info["resid"], infow["resid"])
    if vectors:
        assert np.array_equal(U.view(np.int64), Uw.view(np.int64)), (what, np.abs(U - Uw).max())
        assert np.array_equal(V.view(np.int64), Vw.view(np.int64)), (what, np.abs(V - Vw).max())


def test_plain_storage_is_exact_for_graph_stream_and_run(E, gpu):
    A = SYSTEMS["tall-6"]["A"]
    s, _ = system_of(E, "tall-6", A)
    assert s.plan.stats["sym_pairs"] == 0 and s.plan_t.stats["sym_pairs"] == 0
    plain = E.Plan(s.m, E.make_config(graphs=2, **PLAIN))
    run = dict(tol=TOL)
    ref = s.svds(6, **run)
    assert ref[3]["nconv"] == 6 and ref[3]["restarts"] >= 3, ref[3]            # the steady cycle has been replayed
    _same_bits(s.svds(6, **run), ref, "second run")
    _same_bits(s.svds(6, plan=plain, **run), ref, "graphs=2")
    st = E.Stream()
    try:
        _same_bits(s.svds(6, stream=st.ptr, **run), ref, "user stream")
        _same_bits(s.svds(6, plan=plain, stream=st.ptr, **run), ref, "user stream, graphs=2")
    finally:
        st.destroy()
    values = s.svds(6, vectors=False, **run)
    assert values[1] is None and values[2] is None
    _same_bits(values, ref, "vectors=False", vectors=False)
    plain.destroy()


def test_norm2_is_the_first_singular_value_at_its_tolerance(E, gpu):
    A = SYSTEMS["convection-4"]["A"]
    s, key = system_of(E, "convection-4", A)
    nrm = s.plan.norm2(plan_t=s.plan_t)
    one = s.plan.svds(1, plan_t=s.plan_t, tol=1e-6, vectors=False)[0][0]
    assert np.array_equal(np.float64(nrm).view(np.int64), np.float64(one).view(np.int64))
    exact = dense_of(key, A)[0]
    assert exact * (1 - 10 * 1e-6) <= nrm <= exact * (1 + 1e-12), (nrm, exact)          # from inside
    assert abs(s.plan.norm2() - exact) <= 10 * 1e-6 * exact                             # through ehyb_spmv_t
    z, _ = system_of(E, "zero", SYSTEMS["zero"]["A"])
    assert z.plan.norm2(plan_t=z.plan_t) == 0.0


def test_nan_is_a_breakdown_and_the_vectors_stay(E, gpu):
    A = SYSTEMS["convection-4"]["A"]
    s, _ = system_of(E, "convection-4", A)
    v0 = np.random.default_rng(1).uniform(0.5, 1.5, s.n)
    v0[s.n // 3] = np.nan
    B = A.copy()
    B.data[B.indptr[7]] = np.nan
    sb = System(E, B, **PLAIN)
    lib = E.host._lib.load()
    n, ld = s.n, s.n + (s.n & 1)
    pattern = np.arange(4 * ld, dtype=np.float64) * 0.5 - 7.0
    for what, system, start in (("nan in v0", s, v0), ("nan in the matrix", sb, None)):
        with pytest.raises(E.EhybError) as ei:
            system.plan.svds(4, plan_t=system.plan_t, v0=start)
        assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value), what
        sg, U, V, info = system.plan.svds(4, plan_t=system.plan_t, v0=start, allow_breakdown=True)
        assert info["found"] == info["nconv"] == 0 and info["status"] == "breakdown" and len(sg) == 0 and U.shape == V.shape == (0, n), (what, info)
        du, dv = E.DeviceBuffer(len(pattern)).upload(pattern), E.DeviceBuffer(len(pattern)).upload(pattern)
        d0 = None if start is None else E.DeviceBuffer(n).upload(start)
        found, nconv, mult, rest = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        svals, resid = np.full(4, -3.0), np.full(4, -3.0)
        rc = lib.ehyb_svds(system.plan.h, system.plan_t.h, C.c_void_p(d0.ptr) if d0 else None, 4, 0, 300, TOL, svals.ctypes.data_as(_dp),
                           C.c_void_p(du.ptr), ld, C.c_void_p(dv.ptr), ld, None, C.byref(found), C.byref(nconv), C.byref(mult), C.byref(rest),
                           resid.ctypes.data_as(_dp))
        assert rc == ERR_ARG and b"breakdown" in lib.ehyb_last_error(), what
        assert (found.value, nconv.value, rest.value) == (0, 0, 0) and mult.value == 0, (what, found.value, nconv.value, mult.value, rest.value)
        for d in (du, dv):
            assert np.array_equal(d.download().view(np.int64), pattern.view(np.int64)), what


def test_null_outputs_and_the_c_abi(E, gpu):
    A = SYSTEMS["tall-6"]["A"]
    s, _ = system_of(E, "tall-6", A)
    want = s.plan.svds(6, plan_t=s.plan_t, tol=TOL)
    lib = E.host._lib.load()
    svals = np.zeros(6)
    call = lambda sv_, U, ldu, V, ldv: lib.ehyb_svds(s.plan.h, s.plan_t.h, None, 6, 0, 300, TOL, sv_, U, ldu, V, ldv, None, None, None, None,  # noqa: E731
                                                     None, None)
    assert call(svals.ctypes.data_as(_dp), None, 0, None, 0) == 0
    assert np.array_equal(svals.view(np.int64), want[0].view(np.int64))
    assert call(None, None, 0, None, 0) == 0
    ldu, ldv = s.n + 2, s.n + 4                  # leading dimensions beyond n and of their own: column i at U_dev + i ldu
    du, dv = E.DeviceBuffer(6 * ldu).upload(np.full(6 * ldu, -9.0)), E.DeviceBuffer(6 * ldv).upload(np.full(6 * ldv, -9.0))
    assert call(None, C.c_void_p(du.ptr), ldu, None, 1) == 0                              # U alone; ldv is not looked at
    assert call(None, None, 1, C.c_void_p(dv.ptr), ldv) == 0                              # V alone
    for d, ld, w in ((du, ldu, want[1]), (dv, ldv, want[2])):
        got = d.download().reshape(6, ld)
        assert np.array_equal(got[:, :s.n].view(np.int64), w.view(np.int64)) and (got[:, s.n:] == -9.0).all()
    # a plan_t that was never uploaded: the last check, after the plan's own
    cold = E.Plan(s.mt, E.make_config(**PLAIN), upload=False)
    assert lib.ehyb_svds(s.plan.h, cold.h, None, 6, 0, 300, TOL, None, None, 0, None, 0, None, None, None, None, None, None) == ERR_STATE
    assert b"ehyb_svds: plan_t not uploaded" in lib.ehyb_last_error()


def test_lsqr_is_unchanged_around_a_solve(E, gpu):
    """ehyb_lsqr shares its checks and its transposed multiply with ehyb_svds (transpose_pair.h): system (b) of lsqr_cases ends as
    test_gpu_lsqr.py pins it -- the stop test of the restatement, its iteration count within one -- before and after an svds on the
    same plans, with the same bits both times"""
    c = lc.systems()["b"]
    s, _ = system_of(E, "tall-6", SYSTEMS["tall-6"]["A"])
    assert (s.A != c["Asq"]).nnz == 0
    _, cpu = lc.cpu_lsqr(c["Asq"], c["b"], damp=0.0, max_iter=1000, atol=1e-10, btol=1e-10)
    b = E.vector_reorder(c["b"], s.perm)
    runs = []
    for _ in range(2):
        runs.append(s.plan.lsqr(b, plan_t=s.plan_t, max_iter=1000, check_every=4, atol=1e-10, btol=1e-10))
        s.plan.svds(2, plan_t=s.plan_t, tol=1e-6, vectors=False)
    for x, info in runs:
        assert info["istop"] == cpu["istop"] == 2 and abs(info["iters"] - cpu["iters"]) <= 1, (info, cpu)
    assert np.array_equal(runs[0][0].view(np.int64), runs[1][0].view(np.int64)) and runs[0][1] == runs[1][1]
