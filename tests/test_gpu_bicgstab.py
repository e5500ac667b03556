"""ehyb_bicgstab: right Jacobi-preconditioned BiCGSTAB on the device, for unsymmetric systems.

The test matrices are convection-diffusion operators (a 2-D 5-point upwind stencil whose Peclet number varies over the
domain, plus random one-sided couplings), loaded as general matrices and reordered.  cpu_bicgstab restates the solver's
recurrences, stopping and breakdown rules in numpy; the device must agree with it to a few iterations, reach the true
residual, and agree with scipy's direct solve.  With plain storage the device decides when to stop, so x, the iteration count
and the relative residual are the same bits whatever check_every, graph use or stream.  Everything runs in the permuted
numbering unless said otherwise."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from util import fem_plus_rmat

pytestmark = pytest.mark.gpu

ERR_ARG = 1


def cd_matrix(nx, ny, extra, seed, pe_max=8.0, calm=0.0, shift=0.2):
    """Upwind convection-diffusion on an nx x ny grid: diffusion -1 to every neighbour, the velocity (wx, wy) >= 0 varies
    over the domain (wx up to pe_max, wy up to pe_max / 2) and adds -w to the upwind neighbour and +w to the diagonal; the
    left `calm` fraction of the domain has no convection (there the value pairs are equal).  `extra` random one-sided
    couplings (row r only) with their magnitude added to row r's diagonal, and `shift` on top: strictly diagonally dominant."""
    rng = np.random.default_rng(seed)
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    X, Y = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny))
    wx = (pe_max * (0.5 + 0.5 * np.sin(3 * Y + 1.0))).ravel()
    wy = (0.5 * pe_max * X).ravel()
    still = idx[:, : int(calm * nx)].ravel()
    wx[still] = 0.0
    wy[still] = 0.0
    rows, cols, vals = [], [], []
    diag = np.full(n, 4.0)
    for a, b, w in ((idx[:, 1:].ravel(), idx[:, :-1].ravel(), wx), (idx[1:, :].ravel(), idx[:-1, :].ravel(), wy)):
        rows += [a, b]                                  # b is a's upwind neighbour
        cols += [b, a]
        vals += [-1.0 - w[a], -np.ones(len(a))]
        diag += w
    r, c = rng.integers(0, n, extra), rng.integers(0, n, extra)
    keep = r != c
    r, c = r[keep], c[keep]
    v = -rng.uniform(0.1, 1.0, len(r))
    rows.append(r)
    cols.append(c)
    vals.append(v)
    np.add.at(diag, r, -v)
    rows.append(np.arange(n))
    cols.append(np.arange(n))
    vals.append(diag + shift)
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    return A


def cpu_bicgstab(A, b, x0=None, max_iter=1000, rtol=1e-10, dinv=None):
    """The device's recurrences, stop and breakdown rules in numpy.  -> (x, iterations, relative residual, status)"""
    d = np.ones(len(b)) if dinv is None else dinv
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = b - A @ x
    rh = r.copy()
    p = d * r
    rho, rr, bb = rh @ r, r @ r, b @ b
    bb = bb if bb > 0 else 1.0
    thr = rtol * rtol
    rel = lambda: np.sqrt(rr / bb)                      # noqa: E731
    if not (np.isfinite(rr) and np.isfinite(bb)):
        return x, 0, rel(), "breakdown"
    if rr <= thr * bb:
        return x, 0, rel(), "converged"
    it = 0
    while it < max_iter:
        v = A @ p
        rv = rh @ v
        with np.errstate(all="ignore"):
            alpha = rho / rv
        if not np.isfinite(rho) or rv == 0 or not np.isfinite(rv) or not np.isfinite(alpha):
            return x, it, rel(), "breakdown"
        s = r - alpha * v
        ss = s @ s
        if ss <= thr * bb:                              # half step
            x = x + alpha * p
            rr = ss
            return x, it + 1, rel(), "converged"
        sh = d * s
        t = A @ sh
        ts, tt = t @ s, t @ t
        with np.errstate(all="ignore"):
            omega = ts / tt
        if tt == 0 or not np.isfinite(tt) or not np.isfinite(omega):
            return x, it, rel(), "breakdown"
        x = x + alpha * p + omega * sh
        r = s - omega * t
        rho_new, rr = rh @ r, r @ r
        it += 1
        if rr <= thr * bb:
            return x, it, rel(), "converged"
        with np.errstate(all="ignore"):
            beta = (rho_new / rho) * (alpha / omega)
        if rho == 0 or not np.isfinite(rho) or omega == 0 or not np.isfinite(rho_new) or not np.isfinite(beta):
            return x, it, rel(), "breakdown"
        p = d * r + beta * (p - omega * (d * v))
        rho = rho_new
    return x, it, rel(), "max_iter"


class System:
    def __init__(self, E, A, matrix=None, **kw):
        self.A = A.tocsr()
        self.n = A.shape[0]
        self.cfg = E.make_config(**kw)
        self.m = matrix if matrix is not None else E.Matrix.from_csr(self.A.indptr, self.A.indices, self.A.data, self.cfg,
                                                                     symmetric=False)
        self.m.reorder(self.cfg)
        self.perm = self.m.reorder_list.copy()
        self.plan = E.Plan(self.m, self.cfg)
        with np.errstate(divide="ignore"):                # (a permutation matrix has no diagonal: no preconditioner there)
            self.inv_diag = E.vector_reorder(1.0 / self.A.diagonal(), self.perm)

    def solve(self, E, b, jacobi=True, **kw):
        """b in the original numbering -> (x in the original numbering, iterations, relative residual)"""
        x, it, rel = self.plan.bicgstab(E.vector_reorder(b, self.perm), inv_diag=self.inv_diag if jacobi else None, **kw)
        return E.vector_recover(x, self.perm), it, rel


def panel_matrix(E, cfg):
    """fem_plus_rmat made unsymmetric (upper entries x 1.3, lower x 0.7) and strictly diagonally dominant"""
    m = fem_plus_rmat(E, cfg, rmat_scale=12, rmat_edges=1 << 16)
    A = sp.csr_matrix((m.V.copy(), (m.I.copy(), m.J.copy())), shape=(m.n, m.n))
    m.free()
    off = (A - sp.diags(A.diagonal())).tocsr()
    off.eliminate_zeros()
    return (sp.triu(off, 1) * 1.3 + sp.tril(off, -1) * 0.7 + sp.diags(np.asarray(abs(off).sum(axis=1)).ravel() + 1.0)).tocsr()


SHAPES = [
    ("halo-window", lambda E: (cd_matrix(120, 100, 3000, 1), dict(window_mode=2, lds_doubles=2048)),
     lambda st: st["nnz_ell"] > 0),
    ("reference-window-csr-residual", lambda E: (cd_matrix(120, 100, 3000, 2), dict(window_mode=1, lds_doubles=512)),
     lambda st: st["nnz_er"] > 0 and st["nnz_ell"] > 0),
    ("direct", lambda E: (cd_matrix(110, 90, 2000, 3), dict(direct=1)),
     lambda st: st["nnz_ell"] == 0),
    ("panel-residual", lambda E: (None, dict(partitioner=1, er_mode=2, lds_doubles=4096)),
     lambda st: st["er_partials"] > 0),
    # symmetric pairs add in LDS in an order that varies from launch to launch, so the iteration count is compared on a
    # system whose count does not move under rounding: the numpy restatement with every product perturbed by up to 8 ulp
    # gave the same count in 300 of 300 runs for both right-hand sides (with shift 0.2 and no one-sided couplings it
    # ranged over -4 .. +5 of the unperturbed count in 100)
    ("symmetric-pairs", lambda E: (cd_matrix(120, 100, 600, 4, calm=0.5, shift=1.0), dict(lds_doubles=2048, sym_pairs=1, direct=2)),
     lambda st: st["sym_pairs"] > 0),
]


@pytest.mark.parametrize("name,make,taken", SHAPES, ids=[s[0] for s in SHAPES])
def test_plan_shapes_against_cpu_and_scipy(E, gpu, name, make, taken):
    A, kw = make(E)
    if A is None:
        A = panel_matrix(E, E.make_config(**kw))
    assert abs(A - A.T).nnz > 0, "the system must be unsymmetric"
    s = System(E, A, **kw)
    assert taken(s.plan.stats), (name, s.plan.stats)
    n = s.n
    rng = np.random.default_rng(7)
    rtol = 1e-9
    lu = spla.splu(A.tocsc())                           # scipy's direct solve, factored once for both right-hand sides
    for b in (A @ np.sin(np.arange(n) * 0.01) + 0.1, rng.uniform(-1, 1, n)):
        x, it, rel = s.solve(E, b, max_iter=2000, rtol=rtol, check_every=4)
        assert 0 < it and rel <= rtol, (name, it, rel)
        assert np.linalg.norm(b - A @ x) <= 10 * rtol * np.linalg.norm(b), name
        _, it_cpu, rel_cpu, status = cpu_bicgstab(A, b, max_iter=2000, rtol=rtol, dinv=1.0 / A.diagonal())
        assert status == "converged" and abs(it - it_cpu) <= 5, (name, it, it_cpu, rel, rel_cpu)
        x_ref = lu.solve(b)
        assert np.linalg.norm(x - x_ref) <= 1e-6 * np.linalg.norm(x_ref), (name, np.linalg.norm(x - x_ref))


def test_jacobi_on_a_badly_scaled_system(E, gpu):
    A0 = cd_matrix(100, 90, 2000, 5)
    n = A0.shape[0]
    d = 10.0 ** np.random.default_rng(5).uniform(-0.75, 0.75, n)
    A = (sp.diags(d) @ A0 @ sp.diags(d)).tocsr()
    s = System(E, A, lds_doubles=2048)
    b = A @ np.linspace(-1, 1, n)
    x_pre, it_pre, rel_pre = s.solve(E, b, jacobi=True, max_iter=5000, rtol=1e-9)
    x_none, it_none, rel_none = s.solve(E, b, jacobi=False, max_iter=5000, rtol=1e-9)
    assert rel_pre <= 1e-9 and rel_none <= 1e-9, (rel_pre, rel_none)
    assert 0 < it_pre and it_pre * 3 < it_none, (it_pre, it_none)
    x_ref = spla.spsolve(A.tocsc(), b)
    for x in (x_pre, x_none):
        assert np.linalg.norm(x - x_ref) <= 1e-5 * np.linalg.norm(x_ref), np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)


def _same_bits(got, want, what):
    x, it, rel = got
    xw, itw, relw = want
    assert it == itw, (what, it, itw)
    assert np.array_equal(np.array([rel]), np.array([relw]), equal_nan=True), (what, rel, relw)
    assert np.array_equal(x.view(np.int64), xw.view(np.int64)), (what, np.abs(x - xw).max())


@pytest.mark.parametrize("max_iter", [2000, 23], ids=["converges", "max-iter"])
def test_plain_storage_is_exact_for_every_check_every_graph_and_stream(E, gpu, max_iter):
    A = cd_matrix(120, 100, 3000, 6)
    kw = dict(window_mode=2, lds_doubles=2048, sym_pairs=0)
    s = System(E, A, **kw)
    plain = E.Plan(s.m, E.make_config(graphs=2, **kw))
    b = E.vector_reorder(np.random.default_rng(8).uniform(-1, 1, s.n), s.perm)
    run = dict(max_iter=max_iter, rtol=1e-10, inv_diag=s.inv_diag)
    ref = s.plan.bicgstab(b, check_every=1, **run)
    assert ref[1] > 0 and (ref[1] < max_iter) == (max_iter == 2000), ref[1:]
    for check_every in (3, 10, 0):
        _same_bits(s.plan.bicgstab(b, check_every=check_every, **run), ref, f"check_every={check_every}")
        _same_bits(plain.bicgstab(b, check_every=check_every, **run), ref, f"graphs=2 check_every={check_every}")
    st = E.Stream()
    try:
        _same_bits(s.plan.bicgstab(b, check_every=10, stream=st.ptr, **run), ref, "user stream")
    finally:
        st.destroy()
    _same_bits(s.plan.bicgstab(b, check_every=1, **run), ref, "second run")


def test_short_runs_follow_the_cpu_rule_with_and_without_graphs(E, gpu):
    """The one-vector solve is the k-column driver at k = 1.  Runs too short for a capture (max_iter < 2), a capture followed by an
    odd last burst (7 = 4 + 3 at check_every 4, 2 + 2 + 2 + 1 at check_every 1) and a start that is already converged (b = A x0):
    status and iteration count are those of cpu_bicgstab, and the plan that replays a graph and the one that launches plainly
    (graphs = 2) give the same bits."""
    A = cd_matrix(120, 100, 3000, 1)
    kw = dict(window_mode=2, lds_doubles=2048, sym_pairs=0)
    s = System(E, A, **kw)
    plain = E.Plan(s.m, E.make_config(graphs=2, **kw))
    rng = np.random.default_rng(15)
    x_start = rng.uniform(-1, 1, s.n)
    rtol, dinv = 1e-10, 1.0 / A.diagonal()
    for what, b, x0 in (("random b", rng.uniform(-1, 1, s.n), None), ("b = A x0", A @ x_start, x_start)):
        bp, x0p = E.vector_reorder(b, s.perm), None if x0 is None else E.vector_reorder(x0, s.perm)
        for jacobi in (True, False):
            for max_iter in (0, 1, 2, 7):
                _, it_cpu, _, status_cpu = cpu_bicgstab(A, b, x0=x0, max_iter=max_iter, rtol=rtol, dinv=dinv if jacobi else None)
                assert status_cpu == ("converged" if x0 is not None else "max_iter"), (what, jacobi, max_iter, status_cpu)
                for check_every in (1, 4):
                    case = (what, jacobi, max_iter, check_every)
                    run = dict(x0=x0p, max_iter=max_iter, rtol=rtol, check_every=check_every, inv_diag=s.inv_diag if jacobi else None)
                    got = s.plan.bicgstab(bp, **run)              # (a breakdown would raise)
                    _same_bits(plain.bicgstab(bp, **run), got, f"graphs=2 {case}")
                    status = "converged" if got[2] <= rtol else "max_iter"
                    print(case, "device", got[1], status, got[2], "cpu", it_cpu, status_cpu)
                    assert status == status_cpu, (case, got[1:], it_cpu, status_cpu)
                    assert abs(got[1] - it_cpu) <= 5, (case, got[1], it_cpu)
                    if status_cpu == "max_iter":
                        assert got[1] == max_iter, (case, got[1])


def test_max_iter_is_the_count(E, gpu):
    s = System(E, cd_matrix(100, 90, 2000, 9), lds_doubles=2048)
    b = E.vector_reorder(np.ones(s.n), s.perm)
    for check_every in (1, 4, 10):
        _, it, rel = s.plan.bicgstab(b, max_iter=7, rtol=1e-30, check_every=check_every, inv_diag=s.inv_diag)
        assert it == 7 and 0 < rel < np.inf, (check_every, it, rel)
    _, it, _ = s.plan.bicgstab(b, max_iter=0, rtol=1e-30)
    assert it == 0


def test_nothing_to_do_leaves_x_alone(E, gpu):
    """integer matrix and integer x0: A x0 is exact on both sides, so r = 0 and nothing may move; b = 0 likewise"""
    rng = np.random.default_rng(10)
    A = cd_matrix(90, 80, 1500, 10, pe_max=3.0)
    A.data = np.round(A.data * 4)
    A.eliminate_zeros()
    s = System(E, A, lds_doubles=2048, sym_pairs=0)
    x0 = rng.integers(-50, 50, s.n).astype(np.float64)
    b = A @ x0
    x, it, rel = s.plan.bicgstab(E.vector_reorder(b, s.perm), x0=E.vector_reorder(x0, s.perm), rtol=1e-12, inv_diag=s.inv_diag)
    assert it == 0 and rel == 0.0, (it, rel)
    assert np.array_equal(E.vector_recover(x, s.perm).view(np.int64), x0.view(np.int64))
    x, it, rel = s.plan.bicgstab(np.zeros(s.n), rtol=0.0)
    assert it == 0 and rel == 0.0 and np.array_equal(x.view(np.int64), np.zeros(s.n).view(np.int64))


def test_exact_breakdown_on_a_permutation(E, gpu):
    """A: the cyclic shift (no fixed point), b = e_k, no preconditioner: every product of r^.(A r^) is exactly 0"""
    n = 20000
    A = sp.csr_matrix((np.ones(n), (np.arange(n), (np.arange(n) + 1) % n)), shape=(n, n))
    s = System(E, A, lds_doubles=2048, sym_pairs=0)
    b = np.zeros(n)
    b[1234] = 1.0
    bp = E.vector_reorder(b, s.perm)
    with pytest.raises(E.EhybError) as ei:
        s.plan.bicgstab(bp, max_iter=50, rtol=1e-10)
    assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value)
    x, it, rel = s.plan.bicgstab(bp, max_iter=50, rtol=1e-10, allow_breakdown=True)
    assert it == 0 and rel == 1.0, (it, rel)
    assert np.array_equal(x.view(np.int64), np.zeros(n).view(np.int64))
    assert cpu_bicgstab(A, b, max_iter=50, rtol=1e-10)[3] == "breakdown"


def test_nan_in_b_is_a_breakdown_and_x_stays(E, gpu):
    s = System(E, cd_matrix(100, 90, 2000, 11), lds_doubles=2048)
    rng = np.random.default_rng(12)
    b = rng.uniform(-1, 1, s.n)
    b[s.n // 3] = np.nan
    x0 = rng.uniform(-1, 1, s.n)
    with pytest.raises(E.EhybError) as ei:
        s.plan.bicgstab(b, x0=x0, inv_diag=s.inv_diag)
    assert "breakdown" in str(ei.value)
    x, it, rel = s.plan.bicgstab(b, x0=x0, inv_diag=s.inv_diag, allow_breakdown=True)
    assert it == 0 and np.isnan(rel)
    assert np.array_equal(x.view(np.int64), x0.view(np.int64))


def test_null_outputs_and_the_c_abi(E, gpu):
    s = System(E, cd_matrix(100, 90, 2000, 13), lds_doubles=2048, sym_pairs=0)
    b = E.vector_reorder(np.random.default_rng(13).uniform(-1, 1, s.n), s.perm)
    want = s.plan.bicgstab(b, rtol=1e-10)
    db, dx = E.DeviceBuffer(s.n).upload(b), E.DeviceBuffer(s.n).upload(np.zeros(s.n))
    lib = E.host._lib.load()
    assert lib.ehyb_bicgstab(s.plan.h, None, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), 1000, 1e-10, 10, None, None, None) == 0
    assert np.array_equal(dx.download().view(np.int64), want[0].view(np.int64))
    assert np.array_equal(db.download(), b)


def test_full_size_unsymmetric_audikw_with_jacobi(E, gpu):
    """the timing tool's system (audikw_1-like, off-diagonals x 1.3 above and x 0.7 below the diagonal, diagonal = row sum of
    |a_ij| + mean), plain storage, Jacobi to rtol 1e-8; the true residual in the original numbering on the CPU"""
    import bench as Bn

    gen, gargs, _ = Bn.WORKLOADS["audikw_1-like"]
    cfg = E.make_config(partitioner=Bn.partitioner_for(E, gen), sym_pairs=0)
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    I, J, V = m.I, m.J, m.V
    V[I < J] *= 1.3
    V[I > J] *= 0.7
    off = np.bincount(I, weights=np.abs(V) * (I != J), minlength=m.n)
    V[I == J] = (off + 1.0 * off.mean())[I[I == J]]
    n = m.n
    A = sp.csr_matrix((V.copy(), (I.copy(), J.copy())), shape=(n, n))
    m.reorder(cfg)
    perm = m.reorder_list.copy()
    plan = E.Plan(m, cfg)
    m.free()
    b = np.random.default_rng(14).uniform(-1, 1, n)
    x, it, rel = plan.bicgstab(E.vector_reorder(b, perm), max_iter=500, rtol=1e-8,
                               inv_diag=E.vector_reorder(1.0 / A.diagonal(), perm))
    x = E.vector_recover(x, perm)
    assert 0 < it < 500 and rel <= 1e-8, (it, rel)
    assert np.linalg.norm(b - A @ x) <= 10 * 1e-8 * np.linalg.norm(b)
