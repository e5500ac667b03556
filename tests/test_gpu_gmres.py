"""ehyb_gmres: right Jacobi-preconditioned restarted GMRES on the device, for the unsymmetric systems BiCGSTAB cannot solve.

The matrices are the convection-diffusion operators of test_gpu_bicgstab.py (cd_matrix, copied in) and the skew central-difference
operator on which BiCGSTAB breaks down.  cpu_gmres restates the solver's rules in numpy; the device must agree with it to a few
steps, reach the true residual, and agree with scipy's direct solve.  With plain storage the device decides everything, so x, the
step count and the relative residual are the same bits from run to run, for graphs and plain launches, for a given and a private
stream.  Everything runs in the permuted numbering unless said otherwise."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from util import fem_plus_rmat

pytestmark = pytest.mark.gpu

ERR_ARG = 1
RTOL = 1e-10


def cd_matrix(nx, ny, extra, seed, pe_max=8.0, calm=0.0, shift=0.2):
    """Upwind convection-diffusion on an nx x ny grid: diffusion -1 to every neighbour, the velocity (wx, wy) >= 0 varies
    over the domain (wx up to pe_max, wy up to pe_max / 2) and adds -w to the upwind neighbour and +w to the diagonal; the
    left `calm` fraction of the domain has no convection.  `extra` random one-sided couplings (row r only) with their magnitude
    added to row r's diagonal, and `shift` on top: strictly diagonally dominant."""
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


def skew_matrix(nx, ny):
    """Central differences of a pure convection on an nx x ny grid: -1 / +1 to the left / right neighbour, -0.5 / +0.5 to the
    lower / upper one, zero diagonal: skew-symmetric."""
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    rows, cols, vals = [], [], []
    for a, b, w in ((idx[:, :-1].ravel(), idx[:, 1:].ravel(), 1.0), (idx[:-1, :].ravel(), idx[1:, :].ravel(), 0.5)):
        rows += [a, b]
        cols += [b, a]
        vals += [np.full(len(a), w), np.full(len(a), -w)]
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()


def cpu_bicgstab(A, b, x0=None, max_iter=1000, rtol=1e-10, dinv=None):
    """ehyb_bicgstab's recurrences, stop and breakdown rules in numpy.  -> (x, iterations, relative residual, status)"""
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


def cpu_gmres(A, b, x0=None, restart=30, passes=2, max_iter=1000, rtol=1e-10, dinv=None):
    """ehyb_gmres's rules (include/ehyb.h) in numpy.  -> (x, steps, relative residual, status)"""
    n = len(b)
    d = np.ones(n) if dinv is None else dinv
    x = np.zeros(n) if x0 is None else x0.copy()
    bb = b @ b
    bb = 1.0 if bb == 0 else bb
    thr = rtol * rtol
    it = 0
    with np.errstate(all="ignore"):
        while True:
            r = b - A @ x
            rho = r @ r
            if not (np.isfinite(bb) and np.isfinite(rho)):
                return x, it, np.sqrt(rho / bb), "breakdown"
            if rho <= thr * bb:
                return x, it, np.sqrt(rho / bb), "converged"
            beta = np.sqrt(rho)
            V = [r / beta]
            gt = [beta]
            g, cs, sn = [], [], []
            R = np.zeros((restart, restart))
            status = None
            for j in range(min(restart, max_iter - it)):
                w = A @ (d * V[j])
                h = np.zeros(j + 2)
                Vm = np.array(V)
                for _ in range(passes):
                    c = Vm @ w
                    w = w - c @ Vm
                    h[:j + 1] += c
                h[j + 1] = hn = np.sqrt(w @ w)
                if not np.isfinite(h).all():
                    status = "breakdown"
                    break
                for i in range(j):
                    t = cs[i] * h[i] + sn[i] * h[i + 1]
                    h[i + 1] = -sn[i] * h[i] + cs[i] * h[i + 1]
                    h[i] = t
                gamma = np.hypot(h[j], h[j + 1])
                if gamma == 0 or not np.isfinite(gamma):
                    status = "breakdown"
                    break
                cs.append(h[j] / gamma)
                sn.append(h[j + 1] / gamma)
                R[:j, j] = h[:j]
                R[j, j] = gamma
                gt.append(-sn[j] * gt[j])
                g.append(cs[j] * gt[j])
                it += 1
                rho = gt[j + 1] ** 2
                if rho <= thr * bb:
                    status = "converged"
                    break
                if hn == 0:
                    status = "breakdown"
                    break
                V.append(w / hn)
            J = len(g)
            if J:
                y = sla.solve_triangular(R[:J, :J], np.array(g))
                x = x + d * (y @ np.array(V[:J]))
            if status is not None:
                return x, it, np.sqrt(rho / bb), status
            if it >= max_iter:
                return x, it, np.sqrt(rho / bb), "max_iter"


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
        with np.errstate(divide="ignore"):
            self.inv_diag = E.vector_reorder(1.0 / self.A.diagonal(), self.perm)

    def solve(self, E, b, jacobi=True, **kw):
        """b in the original numbering -> (x in the original numbering, steps, relative residual)"""
        x, it, rel = self.plan.gmres(E.vector_reorder(b, self.perm), inv_diag=self.inv_diag if jacobi else None, **kw)
        return E.vector_recover(x, self.perm), it, rel


def panel_matrix(E, cfg):
    """fem_plus_rmat made unsymmetric (upper entries x 1.3, lower x 0.7) and strictly diagonally dominant"""
    m = fem_plus_rmat(E, cfg, rmat_scale=12, rmat_edges=1 << 16)
    A = sp.csr_matrix((m.V.copy(), (m.I.copy(), m.J.copy())), shape=(m.n, m.n))
    m.free()
    off = (A - sp.diags(A.diagonal())).tocsr()
    off.eliminate_zeros()
    return (sp.triu(off, 1) * 1.3 + sp.tril(off, -1) * 0.7 + sp.diags(np.asarray(abs(off).sum(axis=1)).ravel() + 1.0)).tocsr()


def rhs(n):
    return np.random.default_rng(11).standard_normal(n)


SHAPES = [
    ("halo-window", lambda E: (cd_matrix(120, 100, 3000, 1), dict(window_mode=2, lds_doubles=2048)),
     lambda st: st["nnz_ell"] > 0),
    ("reference-window-csr-residual", lambda E: (cd_matrix(120, 100, 3000, 2), dict(window_mode=1, lds_doubles=512)),
     lambda st: st["nnz_er"] > 0 and st["nnz_ell"] > 0),
    ("direct", lambda E: (cd_matrix(110, 90, 2000, 3), dict(direct=1)),
     lambda st: st["nnz_ell"] == 0),
    ("panel-residual", lambda E: (None, dict(partitioner=1, er_mode=2, lds_doubles=4096)),
     lambda st: st["er_partials"] > 0),
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
    b = rhs(s.n)
    x_ref = spla.spsolve(A.tocsc(), b)
    for restart in (30, 20):
        x, it, rel = s.solve(E, b, restart=restart, max_iter=2000, rtol=RTOL)
        _, it_cpu, rel_cpu, status = cpu_gmres(A, b, restart=restart, max_iter=2000, rtol=RTOL, dinv=1.0 / A.diagonal())
        print(name, restart, "device", it, rel, "cpu", it_cpu, rel_cpu, status)
        assert 0 < it and rel <= RTOL, (name, restart, it, rel)
        assert np.linalg.norm(b - A @ x) <= 10 * RTOL * np.linalg.norm(b), (name, restart)
        assert status == "converged" and abs(it - it_cpu) <= 5, (name, restart, it, it_cpu, rel, rel_cpu)
        assert np.linalg.norm(x - x_ref) <= 1e-6 * np.linalg.norm(x_ref), (name, restart, np.linalg.norm(x - x_ref))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_where_bicgstab_breaks_down(E, gpu, seed):
    """the 8 x 6 skew operator (n = 48, zero diagonal, no preconditioner): BiCGSTAB breaks down by its rule, on the CPU and on the
    device; full GMRES (restart = n) solves the system in at most n steps"""
    A = skew_matrix(8, 6)
    n = A.shape[0]
    assert n == 48 and abs(A + A.T).nnz == 0 and not A.diagonal().any()
    b = np.random.default_rng(seed).standard_normal(n)
    assert cpu_bicgstab(A, b, max_iter=500, rtol=RTOL)[3] == "breakdown"
    s = System(E, A, direct=1, sym_pairs=0)
    bp = E.vector_reorder(b, s.perm)
    try:
        _, it_b, rel_b = s.plan.bicgstab(bp, max_iter=500, rtol=RTOL)
        broke = False
    except E.EhybError as e:
        broke = "breakdown" in str(e)
        it_b, rel_b = None, None
    assert broke, ("ehyb_bicgstab did not break down", it_b, rel_b)
    x, it, rel = s.solve(E, b, jacobi=False, restart=48, max_iter=200, rtol=RTOL)
    print("skew seed", seed, "gmres", it, rel, np.linalg.norm(b - A @ x) / np.linalg.norm(b))
    assert 0 < it <= 48 and rel <= RTOL, (it, rel)
    assert np.linalg.norm(b - A @ x) <= 10 * RTOL * np.linalg.norm(b)
    _, it_cpu, _, status = cpu_gmres(A, b, restart=48, max_iter=200, rtol=RTOL)
    assert status == "converged" and it_cpu <= 48, (it_cpu, status)


def _same_bits(got, want, what):
    x, it, rel = got
    xw, itw, relw = want
    assert it == itw, (what, it, itw)
    assert np.array_equal(np.array([rel]), np.array([relw]), equal_nan=True), (what, rel, relw)
    assert np.array_equal(x.view(np.int64), xw.view(np.int64)), (what, np.abs(x - xw).max())


@pytest.mark.parametrize("max_iter,restart", [(2000, 30), (47, 10), (40, 10), (7, 30)],
                         ids=["converges", "partial-last-cycle", "full-cycles", "no-full-cycle"])
def test_plain_storage_is_exact_for_graph_stream_and_run(E, gpu, max_iter, restart):
    A = cd_matrix(120, 100, 3000, 6)
    kw = dict(window_mode=2, lds_doubles=2048, sym_pairs=0)
    s = System(E, A, **kw)
    plain = E.Plan(s.m, E.make_config(graphs=2, **kw))
    b = E.vector_reorder(rhs(s.n), s.perm)
    run = dict(restart=restart, max_iter=max_iter, rtol=RTOL, inv_diag=s.inv_diag)
    ref = s.plan.gmres(b, **run)
    if max_iter == 2000:
        assert 0 < ref[1] < max_iter and ref[2] <= RTOL, ref[1:]
    else:
        assert ref[1] == max_iter and ref[2] > RTOL, ref[1:]
    _same_bits(s.plan.gmres(b, **run), ref, "second run")
    _same_bits(plain.gmres(b, **run), ref, "graphs=2")
    st = E.Stream()
    try:
        _same_bits(s.plan.gmres(b, stream=st.ptr, **run), ref, "user stream")
        _same_bits(plain.gmres(b, stream=st.ptr, **run), ref, "user stream, graphs=2")
    finally:
        st.destroy()


def test_one_and_two_passes_and_the_restart_lengths(E, gpu):
    """ortho_passes 1, 2 and 0 (= 2); restart 1, 64 and 0 (= 30)"""
    A = cd_matrix(100, 90, 2000, 9)
    s = System(E, A, lds_doubles=2048, sym_pairs=0)
    b = rhs(s.n)
    dinv = 1.0 / A.diagonal()
    counts = {}
    for passes in (1, 2):
        x, it, rel = s.solve(E, b, ortho_passes=passes, max_iter=2000, rtol=RTOL)
        assert 0 < it < 2000 and rel <= RTOL, (passes, it, rel)
        assert np.linalg.norm(b - A @ x) <= 10 * RTOL * np.linalg.norm(b), passes
        counts[passes] = it
    assert abs(counts[1] - counts[2]) <= 5, counts
    bp = E.vector_reorder(b, s.perm)
    _same_bits(s.plan.gmres(bp, ortho_passes=0, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag),
               s.plan.gmres(bp, ortho_passes=2, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag), "ortho_passes 0 is 2")
    _same_bits(s.plan.gmres(bp, restart=0, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag),
               s.plan.gmres(bp, restart=30, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag), "restart 0 is 30")
    for restart, max_iter in ((64, 2000), (1, 20000)):
        x, it, rel = s.solve(E, b, restart=restart, max_iter=max_iter, rtol=RTOL)
        _, it_cpu, _, status = cpu_gmres(A, b, restart=restart, max_iter=max_iter, rtol=RTOL, dinv=dinv)
        print("restart", restart, "device", it, rel, "cpu", it_cpu, status)
        assert status == "converged" and 0 < it < max_iter and rel <= RTOL, (restart, it, rel, status)
        assert abs(it - it_cpu) <= 5, (restart, it, it_cpu)
        assert np.linalg.norm(b - A @ x) <= 10 * RTOL * np.linalg.norm(b), restart


def test_max_iter_is_the_count(E, gpu):
    s = System(E, cd_matrix(100, 90, 2000, 9), lds_doubles=2048)
    b = E.vector_reorder(np.ones(s.n), s.perm)
    for restart in (1, 3, 7, 30):
        _, it, rel = s.plan.gmres(b, restart=restart, max_iter=7, rtol=1e-30, inv_diag=s.inv_diag)
        assert it == 7 and 0 < rel < 1, (restart, it, rel)
    x, it, rel = s.plan.gmres(b, max_iter=0, rtol=1e-30)
    assert it == 0 and rel == 1.0 and not x.any(), (it, rel)


def test_nothing_to_do_leaves_x_alone(E, gpu):
    """integer matrix and integer x0: A x0 is exact on both sides, so r = 0 and nothing may move; b = 0 likewise"""
    rng = np.random.default_rng(10)
    A = cd_matrix(90, 80, 1500, 10, pe_max=3.0)
    A.data = np.round(A.data * 4)
    A.eliminate_zeros()
    s = System(E, A, lds_doubles=2048, sym_pairs=0)
    x0 = rng.integers(-50, 50, s.n).astype(np.float64)
    b = A @ x0
    x, it, rel = s.plan.gmres(E.vector_reorder(b, s.perm), x0=E.vector_reorder(x0, s.perm), rtol=1e-12, inv_diag=s.inv_diag)
    assert it == 0 and rel == 0.0, (it, rel)
    assert np.array_equal(E.vector_recover(x, s.perm).view(np.int64), x0.view(np.int64))
    x, it, rel = s.plan.gmres(np.zeros(s.n), rtol=0.0)
    assert it == 0 and rel == 0.0 and np.array_equal(x.view(np.int64), np.zeros(s.n).view(np.int64))


def test_nan_in_b_is_a_breakdown_and_x_stays(E, gpu):
    s = System(E, cd_matrix(100, 90, 2000, 11), lds_doubles=2048)
    rng = np.random.default_rng(12)
    b = rng.uniform(-1, 1, s.n)
    b[s.n // 3] = np.nan
    x0 = rng.uniform(-1, 1, s.n)
    with pytest.raises(E.EhybError) as ei:
        s.plan.gmres(b, x0=x0, inv_diag=s.inv_diag)
    assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value)
    x, it, rel = s.plan.gmres(b, x0=x0, inv_diag=s.inv_diag, allow_breakdown=True)
    assert it == 0 and np.isnan(rel)
    assert np.array_equal(x.view(np.int64), x0.view(np.int64))
    b[s.n // 3] = 0.5
    x0[5] = np.nan
    x, it, rel = s.plan.gmres(b, x0=x0, inv_diag=s.inv_diag, allow_breakdown=True)
    assert it == 0 and np.isnan(rel)
    assert np.array_equal(x.view(np.int64), x0.view(np.int64))


def test_a_singular_matrix_meets_the_breakdown_rule(E, gpu):
    """row and column k are zero (stored zeros) and b = e_k: v_0 = e_k, w = A v_0 = 0, so h = (0, 0) and gamma = 0 -- a breakdown
    before the step counts, x finite and unchanged.  With b = A y + e_k the solver may not report convergence either."""
    A = cd_matrix(60, 50, 500, 12).tocoo()
    n, k = A.shape[0], 1234
    data = A.data.copy()
    data[(A.row == k) | (A.col == k)] = 0.0
    A = sp.csr_matrix((data, (A.row, A.col)), shape=(n, n))
    s = System(E, A, lds_doubles=2048, sym_pairs=0)
    b = np.zeros(n)
    b[k] = 3.0
    assert cpu_gmres(A, b, max_iter=50)[3] == "breakdown"
    bp = E.vector_reorder(b, s.perm)
    with pytest.raises(E.EhybError) as ei:
        s.plan.gmres(bp, max_iter=50, rtol=RTOL)
    assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value)
    x, it, rel = s.plan.gmres(bp, max_iter=50, rtol=RTOL, allow_breakdown=True)
    assert it == 0 and rel == 1.0 and np.array_equal(x.view(np.int64), np.zeros(n).view(np.int64)), (it, rel)
    b = A @ np.linspace(-1, 1, n) + b
    x, it, rel = s.plan.gmres(E.vector_reorder(b, s.perm), restart=20, max_iter=60, rtol=RTOL, allow_breakdown=True)
    assert np.isfinite(x).all() and it <= 60 and rel > RTOL, (it, rel)


def test_null_outputs_and_the_c_abi(E, gpu):
    s = System(E, cd_matrix(100, 90, 2000, 13), lds_doubles=2048, sym_pairs=0)
    b = E.vector_reorder(rhs(s.n), s.perm)
    want = s.plan.gmres(b, rtol=RTOL)
    db, dx = E.DeviceBuffer(s.n).upload(b), E.DeviceBuffer(s.n).upload(np.zeros(s.n))
    lib = E.host._lib.load()
    assert lib.ehyb_gmres(s.plan.h, None, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), 30, 2, 1000, RTOL, None, None, None) == 0
    assert np.array_equal(dx.download().view(np.int64), want[0].view(np.int64))
    assert np.array_equal(db.download(), b)


def test_val_f32_equals_the_fp64_plan_of_the_rounded_matrix(E, gpu):
    A = cd_matrix(120, 100, 3000, 14)
    A.data *= 1.0 + 2.0 ** -30
    f32 = lambda v: v.astype(np.float32).astype(np.float64)             # noqa: E731
    assert (f32(A.data) != A.data).mean() > 0.9
    kw = dict(window_mode=2, lds_doubles=2048, direct=2, sym_pairs=0)
    cfg1, cfg0 = E.make_config(val_f32=1, **kw), E.make_config(**kw)
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg1, symmetric=False)
    m.reorder(cfg1)
    perm = m.reorder_list.copy()
    p32 = E.Plan(m, cfg1)
    m.V[:] = f32(m.V)
    p64 = E.Plan(m, cfg0)
    assert p32.stats == p64.stats and p32.stats["sym_pairs"] == 0
    b = E.vector_reorder(rhs(A.shape[0]), perm)
    dinv = E.vector_reorder(1.0 / f32(A.diagonal()), perm)
    got = p32.gmres(b, max_iter=2000, rtol=RTOL, inv_diag=dinv)
    assert 3 < got[1] < 2000 and got[2] <= RTOL, got[1:]
    _same_bits(got, p64.gmres(b, max_iter=2000, rtol=RTOL, inv_diag=dinv), "val_f32 against the rounded fp64 plan")
    p32.destroy(), p64.destroy()


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
    x, it, rel = plan.gmres(E.vector_reorder(b, perm), max_iter=500, rtol=1e-8, inv_diag=E.vector_reorder(1.0 / A.diagonal(), perm))
    x = E.vector_recover(x, perm)
    assert 0 < it < 500 and rel <= 1e-8, (it, rel)
    assert np.linalg.norm(b - A @ x) <= 10 * 1e-8 * np.linalg.norm(b)
