"""ehyb_eigsh: thick-restart Lanczos on the device for the few largest or smallest eigenpairs of a symmetric plan.

The matrices are eigsh_cases.sym_grid (a weighted grid Laplacian with a random positive diagonal and, planted, six raised and six
lowered diagonal entries: indefinite with well-separated ends).  cpu_eigsh restates the solver's rules in numpy; the device must
agree with it to two cycles' worth of multiplies, reach the true residual, and agree with dense or scipy eigenvalues.  With
nrm = max |theta| of the returned values, unless said otherwise:
    ||A x_i - theta_i x_i||_2 <= 10 tol nrm     the rule bounds the estimate by tol times the largest Ritz magnitude; the factor 10
                                                between estimate and true residual is the one the GMRES tests give
    |theta_i - lambda_i|      <= 10 tol nrm     against eigvalsh (n <= 2000) or scipy eigsh(tol=1e-12): for a symmetric matrix the
                                                eigenvalue error is at most the residual norm
    max |X^T X - I|           <= 1e-12          cpu_eigsh leaves <= 2e-14 on every input here
    multiplies                within 2 (m - keep) of cpu_eigsh
cpu_eigsh on the 120 x 100 grid, seed 1, tol 1e-10: nev 4 largest 28 multiplies / 1 restart, nev 4 smallest 36 / 2, nev 1 largest
20 / 0.  With plain storage the host arithmetic is deterministic and every device sum is re-added in a fixed order: evals, evecs,
resid and the counters are the same bits from run to run, for graphs and plain launches, for a given and a private stream.
Everything runs in the permuted numbering unless said otherwise."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import eigsh_cases as ec
from util import fem_plus_rmat

pytestmark = pytest.mark.gpu

ERR_ARG = 1
TOL = 1e-10
_dp = C.POINTER(C.c_double)


class System:
    def __init__(self, E, A, **kw):
        self.E = E
        self.A = A.tocsr()
        self.n = A.shape[0]
        self.kw = kw
        self.cfg = E.make_config(**kw)
        self.m = E.Matrix.from_csr(self.A.indptr, self.A.indices, self.A.data, self.cfg, symmetric=False)
        self.m.reorder(self.cfg)
        self.perm = self.m.reorder_list.copy()
        self.plan = E.Plan(self.m, self.cfg)

    def eigsh(self, nev, which, scale=None, v0=None, plan=None, **kw):
        """scale, v0 in the original numbering -> (evals, X (found, n) in the original numbering, info)"""
        E = self.E
        ev, X, info = (plan or self.plan).eigsh(nev, which, scale=None if scale is None else E.vector_reorder(scale, self.perm),
                                                 v0=None if v0 is None else E.vector_reorder(v0, self.perm), **kw)
        return ev, np.array([E.vector_recover(x, self.perm) for x in X]).reshape(len(X), self.n), info


def reference(A, nev, which, scale=None):
    """the nev wanted eigenvalues from the wanted end: dense for n <= 2000, else scipy's eigsh at tol 1e-12"""
    n = A.shape[0]
    if n <= 2000:
        D = A.toarray() if scale is None else scale[:, None] * A.toarray() * scale[None, :]
        lam = np.linalg.eigvalsh(D)
    else:
        assert scale is None
        lam = np.sort(spla.eigsh(A, k=nev, which=which, tol=1e-12, ncv=max(4 * nev, 40))[0])
    return lam[::-1][:nev] if which == "LA" else lam[:nev]


def check(what, A, got, nev, which, tol=TOL, scale=None, basis=0, cpu=True, **kw):
    """the four assertions of the module docstring; -> info"""
    ev, X, info = got
    want = min(nev, A.shape[0])
    op = (lambda x: A @ x) if scale is None else (lambda x: scale * (A @ (scale * x)))
    nrm = np.abs(ev).max()
    res = max(np.linalg.norm(op(X[i]) - ev[i] * X[i]) for i in range(len(ev)))
    err = np.abs(ev - reference(A, want, which, scale)).max()
    orth = np.abs(X @ X.T - np.eye(len(ev))).max()
    print(what, which, "device", info["multiplies"], info["restarts"], info["nconv"], f"res/nrm {res / nrm:.2e} err/nrm {err / nrm:.2e} orth {orth:.1e}")
    assert info["found"] == info["nconv"] == want == len(ev), (what, info)
    assert res <= 10 * tol * nrm, (what, res / nrm)
    assert err <= 10 * tol * nrm, (what, err / nrm)
    assert orth <= 1e-12, (what, orth)
    if cpu:
        _, _, ci = ec.cpu_eigsh(A, nev, which, basis=basis, tol=tol, scale=scale, **kw)
        m, keep = ec.resolve_basis(nev, basis, A.shape[0])
        print(what, which, "cpu", ci["multiplies"], ci["restarts"], ci["nconv"])
        assert ci["status"] == "ok" and ci["nconv"] == want
        assert abs(info["multiplies"] - ci["multiplies"]) <= 2 * (m - keep), (what, info["multiplies"], ci["multiplies"])
    return info


def panel_matrix(E, cfg):
    """fem_plus_rmat made symmetric, with the planted diagonal of sym_grid on top"""
    m = fem_plus_rmat(E, cfg, rmat_scale=12, rmat_edges=1 << 16)
    A = sp.csr_matrix((m.V.copy(), (m.I.copy(), m.J.copy())), shape=(m.n, m.n))
    m.free()
    A = ((A + A.T) * 0.5).tocsr()
    return (A + sp.diags(ec.planted_diagonal(A.shape[0], 5))).tocsr()


SHAPES = [
    ("halo-window", lambda E: (ec.sym_grid(120, 100, 1), dict(window_mode=2, lds_doubles=2048)),
     lambda st: st["nnz_ell"] > 0),
    ("reference-window-csr-residual", lambda E: (ec.sym_grid(120, 100, 2), dict(window_mode=1, lds_doubles=512)),
     lambda st: st["nnz_er"] > 0 and st["nnz_ell"] > 0),
    ("direct", lambda E: (ec.sym_grid(120, 100, 3), dict(direct=1)),
     lambda st: st["nnz_ell"] == 0),
    ("panel-residual", lambda E: (None, dict(partitioner=1, er_mode=2, lds_doubles=4096)),
     lambda st: st["er_partials"] > 0),
    ("symmetric-pairs", lambda E: (ec.sym_grid(120, 100, 4), dict(lds_doubles=2048, sym_pairs=1, direct=2)),
     lambda st: st["sym_pairs"] > 0),
]


@pytest.mark.parametrize("name,make,taken", SHAPES, ids=[s[0] for s in SHAPES])
def test_plan_shapes_against_cpu_and_reference(E, gpu, name, make, taken):
    A, kw = make(E)
    if A is None:
        A = panel_matrix(E, E.make_config(**kw))
    assert abs(A - A.T).nnz == 0, "the matrix must be symmetric"
    s = System(E, A, **kw)
    assert taken(s.plan.stats), (name, s.plan.stats)
    for which in ("LA", "SA"):
        check(name, A, s.eigsh(4, which, tol=TOL), 4, which)
    if name == "halo-window":
        info = check(name + " nev=1", A, s.eigsh(1, "LA", tol=TOL), 1, "LA")
        assert info["restarts"] <= 1


def test_full_spectrum_of_a_small_matrix(E, gpu):
    """n = 48 and basis = 64 resolves to 48: one cycle of 48 multiplies, then w is rounding noise and the invariant rule fires"""
    A = ec.sym_grid(8, 6, 2)
    s = System(E, A, direct=1)
    for nev, which in ((5, "LA"), (16, "SA")):
        info = check("n=48", A, s.eigsh(nev, which, basis=64, tol=TOL), nev, which, basis=64)
        assert info["multiplies"] == 48 and info["restarts"] == 0, info
        assert (info["resid"] == 0).all()


def test_one_and_two_rows(E, gpu):
    s = System(E, sp.csr_matrix(np.array([[3.5]])), direct=1)
    ev, X, info = s.eigsh(2, "LA")
    assert (info["found"], info["nconv"], info["multiplies"], info["restarts"]) == (1, 1, 1, 0), info
    assert ev.tolist() == [3.5] and np.abs(X).tolist() == [[1.0]]
    A = sp.csr_matrix(np.array([[2.0, 1.0], [1.0, -1.0]]))
    s = System(E, A, direct=1)
    for which in ("LA", "SA"):
        ev, X, info = s.eigsh(2, which)
        assert (info["found"], info["nconv"], info["multiplies"], info["restarts"]) == (2, 2, 2, 0), info
        lam = np.linalg.eigvalsh(A.toarray())
        assert np.abs(ev - (lam[::-1] if which == "LA" else lam)).max() <= 10 * TOL * np.abs(lam).max()
        assert max(np.linalg.norm(A @ X[i] - ev[i] * X[i]) for i in range(2)) <= 10 * TOL * np.abs(lam).max()
        assert np.abs(X @ X.T - np.eye(2)).max() <= 1e-12


def test_an_invariant_subspace_smaller_than_nev(E, gpu):
    """three distinct eigenvalues, each twenty-fold: the Krylov space of any start vector has dimension 3, and a multiple
    eigenvalue is found once"""
    A = sp.diags(np.r_[np.ones(20), 2 * np.ones(20), 5 * np.ones(20)]).tocsr()
    s = System(E, A, direct=1)
    ev, X, info = s.eigsh(4, "LA")
    assert (info["found"], info["nconv"], info["multiplies"], info["restarts"]) == (3, 3, 3, 0), info
    assert np.abs(ev - [5.0, 2.0, 1.0]).max() <= 10 * TOL * 5.0
    assert max(np.linalg.norm(A @ X[i] - ev[i] * X[i]) for i in range(3)) <= 10 * TOL * 5.0
    assert np.abs(X @ X.T - np.eye(3)).max() <= 1e-12


def test_the_smallest_legal_basis_and_the_largest_nev(E, gpu):
    """basis = nev + 2: one step per cycle, every restart with kk = keep (cpu_eigsh: 70 restarts for the largest three, 103 for the
    smallest); nev = 16 with basis = 64 (cpu_eigsh: 8 and 19 restarts)"""
    A = ec.sym_grid(8, 6, 2)
    s = System(E, A, direct=1)
    for which in ("LA", "SA"):
        info = check("basis=5", A, s.eigsh(3, which, basis=5, tol=TOL), 3, which, basis=5)
        assert info["restarts"] > 20 and info["multiplies"] == 5 + info["restarts"], info
    A = ec.sym_grid(50, 40, 4)
    s = System(E, A, window_mode=2, lds_doubles=2048)
    for which in ("LA", "SA"):
        info = check("nev=16", A, s.eigsh(16, which, basis=64, tol=TOL), 16, which, basis=64)
        assert info["restarts"] > 2, info


def test_scale_and_the_spectrum_bounds(E, gpu):
    """S A S with S = diag(A)^-1/2 has the spectrum of D^-1 A (cpu_eigsh: 7 and 6 restarts).  lambda_max is a Rayleigh quotient
    from below like the Ritz value, and the Lanczos one has converged; spectrum_bounds brackets nothing outside the dense spectrum"""
    A = (ec.sym_grid(50, 40, 3, False) + sp.diags(np.random.default_rng(3).uniform(0, 30, 2000))).tocsr()
    d = A.diagonal()
    scale = 1.0 / np.sqrt(d)
    s = System(E, A, window_mode=2, lds_doubles=2048)
    theta = {}
    for which in ("LA", "SA"):
        got = s.eigsh(2, which, scale=scale, tol=TOL)
        check("scale", A, got, 2, which, scale=scale)
        theta[which] = got[0][0]
    inv_diag = E.vector_reorder(1.0 / d, s.perm)
    lam = s.plan.lambda_max(inv_diag)
    assert 0 < lam <= theta["LA"] * (1 + 1e-9), (lam, theta["LA"])
    dense = np.linalg.eigvalsh(scale[:, None] * A.toarray() * scale[None, :])
    lo, hi = s.plan.spectrum_bounds(inv_diag)
    slack = 1e-12 * dense[-1]
    assert dense[0] - slack <= lo <= hi <= dense[-1] + slack, (lo, hi, dense[0], dense[-1])
    assert lo - dense[0] <= 10 * 1e-4 * hi and dense[-1] - hi <= 10 * 1e-4 * hi, (lo, hi, dense[0], dense[-1])
    lo, hi = s.plan.spectrum_bounds()
    dense = np.linalg.eigvalsh(A.toarray())
    assert dense[0] * (1 - 1e-12) <= lo <= hi <= dense[-1] * (1 + 1e-12)


def test_max_restarts_exhausted(E, gpu):
    A = ec.sym_grid(120, 100, 1, False)
    s = System(E, A, window_mode=2, lds_doubles=2048)
    ev, X, info = s.eigsh(4, "SA", max_restarts=3, tol=TOL)
    assert info["found"] == 4 and info["nconv"] < 4 and info["multiplies"] == 44 and info["restarts"] == 3, info
    assert info["resid"][info["nconv"]] > TOL * np.abs(ev).max()
    assert X.shape == (4, s.n) and np.abs(X @ X.T - np.eye(4)).max() <= 1e-12
    ev0, _, info0 = s.eigsh(4, "SA", max_restarts=0, tol=TOL)
    assert info0["multiplies"] == 20 and info0["restarts"] == 0 and info0["found"] == 4 and info0["nconv"] < 4


def _same_bits(got, want, what):
    ev, X, info = got
    evw, Xw, infow = want
    assert [info[k] for k in ("found", "nconv", "multiplies", "restarts")] == [infow[k] for k in ("found", "nconv", "multiplies", "restarts")], (what, info, infow)
    assert np.array_equal(ev.view(np.int64), evw.view(np.int64)), (what, ev, evw)
    assert np.array_equal(info["resid"].view(np.int64), infow["resid"].view(np.int64)), (what, info["resid"], infow["resid"])
    assert np.array_equal(X.view(np.int64), Xw.view(np.int64)), (what, np.abs(X - Xw).max())


@pytest.mark.parametrize("grid,nev,which,basis,restarts", [((120, 100, 1), 4, "LA", 0, 1), ((8, 6, 2), 3, "SA", 5, None)],
                         ids=["one-restart", "many-replays"])
def test_plain_storage_is_exact_for_graph_stream_and_run(E, gpu, grid, nev, which, basis, restarts):
    A = ec.sym_grid(*grid)
    kw = dict(window_mode=2, lds_doubles=2048, sym_pairs=0) if A.shape[0] > 1000 else dict(direct=1, sym_pairs=0)
    s = System(E, A, **kw)
    plain = E.Plan(s.m, E.make_config(graphs=2, **kw))
    run = dict(basis=basis, tol=TOL)
    ref = s.eigsh(nev, which, **run)
    assert ref[2]["nconv"] == nev and (ref[2]["restarts"] == restarts if restarts is not None else ref[2]["restarts"] > 20), ref[2]
    _same_bits(s.eigsh(nev, which, **run), ref, "second run")
    _same_bits(s.eigsh(nev, which, plan=plain, **run), ref, "graphs=2")
    st = E.Stream()
    try:
        _same_bits(s.eigsh(nev, which, stream=st.ptr, **run), ref, "user stream")
        _same_bits(s.eigsh(nev, which, plan=plain, stream=st.ptr, **run), ref, "user stream, graphs=2")
    finally:
        st.destroy()


def test_val_f32_equals_the_fp64_plan_of_the_rounded_matrix(E, gpu):
    A = ec.sym_grid(120, 100, 14)
    A.data *= 1.0 + 2.0 ** -30
    f32 = lambda v: v.astype(np.float32).astype(np.float64)             # noqa: E731
    assert (f32(A.data) != A.data).mean() > 0.9
    kw = dict(window_mode=2, lds_doubles=2048, direct=2, sym_pairs=0)
    cfg1, cfg0 = E.make_config(val_f32=1, **kw), E.make_config(**kw)
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg1, symmetric=False)
    m.reorder(cfg1)
    p32 = E.Plan(m, cfg1)
    m.V[:] = f32(m.V)
    p64 = E.Plan(m, cfg0)
    assert p32.stats == p64.stats and p32.stats["sym_pairs"] == 0
    for which in ("LA", "SA"):
        got = p32.eigsh(4, which, tol=TOL)
        assert got[2]["nconv"] == 4 and got[2]["multiplies"] >= 20, got[2]
        _same_bits(got, p64.eigsh(4, which, tol=TOL), "val_f32 against the rounded fp64 plan")
    p32.destroy(), p64.destroy()


def test_nan_is_a_breakdown_and_evecs_stay(E, gpu):
    A = ec.sym_grid(60, 50, 2)
    s = System(E, A, window_mode=2, lds_doubles=2048)
    v0 = np.random.default_rng(1).uniform(0.5, 1.5, s.n)
    v0[s.n // 3] = np.nan
    B = A.copy()
    B.data[B.indptr[7] + list(B.indices[B.indptr[7]:B.indptr[8]]).index(7)] = np.nan       # the diagonal entry of row 7
    sb = System(E, B, window_mode=2, lds_doubles=2048)
    lib = E.host._lib.load()
    n, ldv = s.n, s.n + (s.n & 1)
    pattern = np.arange(4 * ldv, dtype=np.float64) * 0.5 - 7.0
    for what, system, start in (("nan in v0", s, v0), ("nan in the matrix", sb, None)):
        with pytest.raises(E.EhybError) as ei:
            system.plan.eigsh(4, "LA", v0=start)
        assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value), what
        ev, X, info = system.plan.eigsh(4, "LA", v0=start, allow_breakdown=True)
        assert info["found"] == info["nconv"] == 0 and len(ev) == 0 and X.shape == (0, n), (what, info)
        dv = E.DeviceBuffer(len(pattern)).upload(pattern)
        d0 = None if start is None else E.DeviceBuffer(n).upload(start)
        found, nconv, mult, rest = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        evals, resid = np.full(4, -3.0), np.full(4, -3.0)
        rc = lib.ehyb_eigsh(system.plan.h, None, C.c_void_p(d0.ptr) if d0 else None, 4, 0, 0, 300, TOL, evals.ctypes.data_as(_dp),
                            C.c_void_p(dv.ptr), ldv, None, C.byref(found), C.byref(nconv), C.byref(mult), C.byref(rest), resid.ctypes.data_as(_dp))
        assert rc == ERR_ARG and b"breakdown" in lib.ehyb_last_error(), what
        assert (found.value, nconv.value, rest.value) == (0, 0, 0) and mult.value == 0, (what, found.value, nconv.value, mult.value, rest.value)
        assert np.array_equal(dv.download().view(np.int64), pattern.view(np.int64)), what


def test_null_outputs_and_the_c_abi(E, gpu):
    A = ec.sym_grid(120, 100, 13)
    s = System(E, A, window_mode=2, lds_doubles=2048, sym_pairs=0)
    want = s.plan.eigsh(4, "SA", tol=TOL)
    lib = E.host._lib.load()
    evals = np.zeros(4)
    assert lib.ehyb_eigsh(s.plan.h, None, None, 4, 1, 0, 300, TOL, evals.ctypes.data_as(_dp), None, 0, None, None, None, None, None, None) == 0
    assert np.array_equal(evals.view(np.int64), want[0].view(np.int64))
    assert lib.ehyb_eigsh(s.plan.h, None, None, 4, 1, 0, 300, TOL, None, None, 0, None, None, None, None, None, None) == 0
    ldv = s.n + 2                              # a leading dimension beyond n: column i at evecs_dev + i ldv
    dv = E.DeviceBuffer(4 * ldv).upload(np.full(4 * ldv, -9.0))
    assert lib.ehyb_eigsh(s.plan.h, None, None, 4, 1, 0, 300, TOL, None, C.c_void_p(dv.ptr), ldv, None, None, None, None, None, None) == 0
    got = dv.download().reshape(4, ldv)
    assert np.array_equal(got[:, :s.n].view(np.int64), want[1].view(np.int64)) and (got[:, s.n:] == -9.0).all()
