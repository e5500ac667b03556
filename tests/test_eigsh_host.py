"""ehyb_eigsh on the host: the dense eigensolver ehyb_sym_eig against numpy.linalg.eigh, every argument check of ehyb_eigsh and of
the three step calls in the order the header states (on plans that were never uploaded: EHYB_ERR_STATE comes last), how basis = 0
resolves, and the numpy restatement cpu_eigsh -- the yardstick of test_gpu_eigsh.py -- against dense eigenvalues.  Nothing here
needs a GPU.

ehyb_sym_eig: with r(Y, theta) = max_i ||T y_i - theta_i y_i||_2 and o(Y) = max |Y^T Y - I|, the library may leave at most 4 x what
numpy's own result leaves, numpy's figure floored at m 2^-52 ||T||_F (the residual) and m 2^-52 (the orthogonality); the
eigenvalues are rising and within the residual bound of numpy's.  The worst ratio to the bound over all inputs is printed
(DESIGN.md section 18 quotes it)."""
import ctypes as C

import numpy as np
import pytest

import eigsh_cases as ec

ERR_ARG, ERR_STATE = 1, 8
SIZES = [1, 2, 3, 8, 33, 64, 65]
EPS = 2.0 ** -52
_dp = C.POINTER(C.c_double)


def sym_eig(lib, T):
    m = T.shape[0]
    Tf = np.asfortranarray(T, dtype=np.float64)
    ev, Y = np.full(m, np.nan), np.full(m * m, np.nan)
    rc = lib.ehyb_sym_eig(m, Tf.ctypes.data_as(_dp), m, ev.ctypes.data_as(_dp), Y.ctypes.data_as(_dp))
    assert rc == 0, lib.ehyb_last_error()
    return ev, Y.reshape(m, m).T


def inputs(m):
    rng = np.random.default_rng(m)
    R = rng.standard_normal((m, m))
    R = R + R.T
    k = m // 2                                   # as a restart leaves T: diag(theta), an arrow in column k, tridiagonal behind it
    Arrow = np.diag(np.sort(rng.uniform(-3, 40, m))[::-1].copy())
    if m > 1:
        Arrow[:k, k] = Arrow[k, :k] = rng.standard_normal(k) * 10.0 ** rng.integers(-12, 1, k)
        for i in range(k, m - 1):
            Arrow[i, i + 1] = Arrow[i + 1, i] = rng.uniform(0.1, 2.0)
    Rep = np.diag(np.repeat([2.0, -1.0, 2.0, 7.0], -(-m // 4))[:m])
    return {"random": R, "arrow": Arrow, "repeated-diagonal": Rep, "zero": np.zeros((m, m)), "scaled-up": R * 2.0 ** 200,
            "scaled-down": R * 2.0 ** -200}


WORST = {"residual": 0.0, "orthogonality": 0.0, "values": 0.0}


@pytest.mark.parametrize("m", SIZES)
def test_sym_eig_against_numpy(E, m):
    lib = E.host._lib.load()
    for name, T in inputs(m).items():
        ev, Y = sym_eig(lib, T)
        wn, Yn = np.linalg.eigh(T)
        fro = np.linalg.norm(T)
        res = lambda th, Z: np.linalg.norm(T @ Z - Z * th, axis=0).max()                  # noqa: E731
        orth = lambda Z: np.abs(Z.T @ Z - np.eye(m)).max()                                 # noqa: E731
        bound_r = 4 * max(res(wn, Yn), m * EPS * fro)
        bound_o = 4 * max(orth(Yn), m * EPS)
        got_r, got_o, got_v = res(ev, Y), orth(Y), np.abs(ev - wn).max()
        print(f"m={m} {name}: residual {got_r:.3e} / {bound_r:.3e}, orthogonality {got_o:.3e} / {bound_o:.3e}, values {got_v:.3e}")
        assert np.isfinite(ev).all() and np.isfinite(Y).all(), (m, name)
        assert (np.diff(ev) >= 0).all(), (m, name, "not rising")
        assert got_r <= bound_r, (m, name, got_r, bound_r)
        assert got_o <= bound_o, (m, name, got_o, bound_o)
        assert got_v <= bound_r, (m, name, got_v, bound_r)
        for key, ratio in (("residual", got_r / bound_r if bound_r else 0.0), ("orthogonality", got_o / bound_o),
                           ("values", got_v / bound_r if bound_r else 0.0)):
            WORST[key] = max(WORST[key], ratio)
    print("worst ratios to the bound so far:", WORST)


def test_sym_eig_reads_the_upper_triangle_and_is_deterministic(E):
    lib = E.host._lib.load()
    T = inputs(33)["random"]
    want = sym_eig(lib, T)
    junk = np.triu(T) + np.tril(np.full_like(T, np.nan), -1)
    got = sym_eig(lib, junk)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    wide = np.full((40, 33), np.nan, order="F")          # a leading dimension of its own
    wide[:33] = np.triu(T)
    ev, Y = np.zeros(33), np.zeros(33 * 33)
    assert lib.ehyb_sym_eig(33, wide.ctypes.data_as(_dp), 40, ev.ctypes.data_as(_dp), Y.ctypes.data_as(_dp)) == 0
    assert np.array_equal(ev.view(np.int64), want[0].view(np.int64))


def test_sym_eig_argument_errors(E):
    lib = E.host._lib.load()
    T, ev, Y = np.eye(3, order="F"), np.zeros(3), np.zeros(9)
    p = lambda a: a.ctypes.data_as(_dp)                  # noqa: E731
    assert lib.ehyb_sym_eig(0, p(T), 3, p(ev), p(Y)) == ERR_ARG
    assert lib.ehyb_sym_eig(66, p(T), 66, p(ev), p(Y)) == ERR_ARG
    assert lib.ehyb_sym_eig(3, p(T), 2, p(ev), p(Y)) == ERR_ARG
    assert lib.ehyb_sym_eig(3, None, 3, p(ev), p(Y)) == ERR_ARG
    assert lib.ehyb_sym_eig(3, p(T), 3, None, p(Y)) == ERR_ARG
    assert lib.ehyb_sym_eig(3, p(T), 3, p(ev), None) == ERR_ARG
    T[0, 2] = np.inf
    assert lib.ehyb_sym_eig(3, p(T), 3, p(ev), p(Y)) == ERR_ARG and b"finite" in lib.ehyb_last_error()


# ------------------------------------------------------------------ the argument checks and their order
FEM_SMALL = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))


def host_plan(E, half=False, **kw):
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(FEM_SMALL[0], *FEM_SMALL[1], cfg=cfg)
    m.reorder(cfg)
    pb = m.part_boundary
    return E.Plan(m, cfg, rows=(0, int(pb[len(pb) // 2])) if half else None, upload=False)


@pytest.fixture(scope="module")
def plan(E):
    return host_plan(E, direct=2)


@pytest.fixture(scope="module")
def part(E):
    p = host_plan(E, half=True, direct=2)
    assert 0 < p.rows[1] < p.n
    return p


X, S0, V0 = 0x10000, 0x20000, 0x30000            # never read: every call fails before device work


def call(lib, plan, scale=S0, v0=V0, nev=4, which=0, basis=0, max_restarts=10, tol=1e-8, evecs=X, ldv=None, outputs=True):
    n = plan.n if plan is not None else 0
    ldv = n + (n & 1) if ldv is None else ldv
    ints = [C.c_int(-5) for _ in range(4)]
    ev, rs = np.full(16, -5.0), np.full(16, -5.0)
    rc = lib.ehyb_eigsh(plan.h if plan is not None else None, C.c_void_p(scale) if scale else None, C.c_void_p(v0) if v0 else None, nev,
                        which, basis, max_restarts, tol, ev.ctypes.data_as(_dp) if outputs else None, C.c_void_p(evecs) if evecs else None,
                        ldv, None, *((C.byref(i) for i in ints) if outputs else (None,) * 4), rs.ctypes.data_as(_dp) if outputs else None)
    assert [i.value for i in ints] == [-5] * 4 and (ev == -5).all() and (rs == -5).all(), "an output was written before device work"
    return rc, lib.ehyb_last_error()


def test_never_uploaded_plan_is_a_state_error(E, plan):
    lib = E.host._lib.load()
    for kw in (dict(), dict(nev=1), dict(nev=16, basis=18), dict(which=1), dict(basis=64), dict(basis=6), dict(max_restarts=0), dict(tol=0.0),
               dict(scale=None, v0=None), dict(evecs=None, ldv=1), dict(outputs=False), dict(ldv=plan.n + (plan.n & 1) + 2)):
        rc, msg = call(lib, plan, **kw)
        assert rc == ERR_STATE and b"ehyb_eigsh:" in msg and b"upload" in msg, (kw, msg)


# in the order of the header; each entry: the fault, and a word of its message
STAGES = [(dict(nev=0), b"nev"), (dict(tol=float("nan")), b"tol"), ("part", b"all rows"), (dict(ldv=3), b"ldv"), (dict(evecs=X + 8), b"aligned")]
RANGES = [dict(nev=0), dict(nev=17), dict(nev=-1), dict(which=2), dict(which=-1), dict(basis=5), dict(basis=65), dict(basis=-1),
          dict(basis=1, nev=1), dict(max_restarts=-1)]


@pytest.mark.parametrize("bad", RANGES, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in RANGES])
def test_range_errors(E, plan, bad):
    lib = E.host._lib.load()
    assert call(lib, plan)[0] == ERR_STATE
    rc, msg = call(lib, plan, **bad)
    assert rc == ERR_ARG and b"ehyb_eigsh: nev" in msg, (bad, msg)


@pytest.mark.parametrize("bad,word", [(dict(tol=-1e-9), b"tol"), (dict(tol=float("nan")), b"tol"), (dict(tol=float("-inf")), b"tol"),
                                      (dict(ldv=1), b"ldv"), (dict(ldv=30001), b"ldv"), (dict(evecs=X + 8), b"aligned"),
                                      (dict(scale=S0 + 8), b"aligned"), (dict(v0=V0 + 8), b"aligned")])
def test_other_argument_errors(E, plan, bad, word):
    lib = E.host._lib.load()
    assert plan.n == 30000
    rc, msg = call(lib, plan, **bad)
    assert rc == ERR_ARG and word in msg and b"upload" not in msg, (bad, msg)


def test_null_plan_comes_first(E):
    lib = E.host._lib.load()
    rc, msg = call(lib, None, nev=0, tol=-1.0)
    assert rc == ERR_ARG and b"null argument" in msg, msg


def test_the_order_of_the_checks(E, plan, part):
    """all the faults from stage i on at once: stage i's message comes"""
    lib = E.host._lib.load()
    for first in range(len(STAGES)):
        kw, p = {}, plan
        for fault, _ in STAGES[first:]:
            if fault == "part":
                p = part
            else:
                kw.update(fault)
        if "ldv" not in kw:
            kw["ldv"] = None
        rc, msg = call(lib, p, **kw)
        assert rc == ERR_ARG and STAGES[first][1] in msg, (first, kw, msg)
    rc, msg = call(lib, part)
    assert rc == ERR_ARG and b"all rows" in msg


def test_step_calls_check_their_arguments(E):
    lib = E.host._lib.load()
    P = lambda a: C.c_void_p(a) if a else None          # noqa: E731
    V, W, Z, SL, SC, Y = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    nxt = lambda n=10, ld=10, v=V, w=W, sc=SC, z=Z, s=SL, j=0: lib.ehyb_eigsh_next_step(n, ld, P(v), P(w), P(sc), P(z), P(s), j, None)      # noqa: E731
    for kw in (dict(n=-1), dict(v=0), dict(w=0), dict(z=0), dict(s=0), dict(j=-2), dict(j=64), dict(ld=9), dict(ld=11), dict(n=11, ld=11),
               dict(v=V + 8), dict(w=W + 8), dict(sc=SC + 8), dict(z=Z + 8)):
        assert nxt(**kw) == ERR_ARG and b"ehyb_eigsh_next_step" in lib.ehyb_last_error(), kw
    # in the order of the gmres steps: null pointers, then the range, then the pairs
    assert nxt(v=0, j=99, ld=9) == ERR_ARG and b"bad arguments" in lib.ehyb_last_error() and b"j " not in lib.ehyb_last_error()
    assert nxt(j=99, ld=9) == ERR_ARG and b"j 99" in lib.ehyb_last_error()
    assert nxt(ld=9) == ERR_ARG and b"leading dimension" in lib.ehyb_last_error()
    scl = lambda n=10, sc=SC, w=W, s=SL: lib.ehyb_eigsh_scale_step(n, P(sc), P(w), P(s), None)          # noqa: E731
    for kw in (dict(n=-1), dict(sc=0), dict(w=0), dict(s=0), dict(sc=SC + 8), dict(w=W + 8)):
        assert scl(**kw) == ERR_ARG and b"ehyb_eigsh_scale_step" in lib.ehyb_last_error(), kw
    rot = lambda n=10, lds=10, src=V, ldd=12, dst=W, y=Y, mc=3, kc=2: lib.ehyb_eigsh_rotate_step(n, lds, P(src), ldd, P(dst), P(y), mc, kc, None)  # noqa: E731
    for kw in (dict(n=-1), dict(src=0), dict(dst=0), dict(y=0), dict(mc=0), dict(mc=66), dict(kc=0), dict(kc=65), dict(lds=9), dict(lds=8),
               dict(ldd=11), dict(ldd=8), dict(src=V + 8), dict(dst=W + 8)):
        assert rot(**kw) == ERR_ARG and b"ehyb_eigsh_rotate_step" in lib.ehyb_last_error(), kw


# ------------------------------------------------------------------ the layout
@pytest.mark.parametrize("nev,m,keep", [(1, 20, 10), (9, 20, 14), (10, 21, 15), (16, 33, 24)])
def test_basis_zero_resolves_as_stated(E, nev, m, keep):
    lib = E.host._lib.load()
    a, b = C.c_int(-1), C.c_int(-1)
    assert lib.ehyb_eigsh_basis(nev, 0, 10 ** 6, C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == (m, keep) == ec.resolve_basis(nev, 0, 10 ** 6)
    assert m == min(max(2 * nev + 1, 20), 64) and keep == nev + (m - nev) // 2


def test_basis_is_cut_to_n_and_given_ones_stand(E):
    lib = E.host._lib.load()
    for nev, basis, n in ((5, 64, 48), (16, 64, 48), (2, 0, 1), (2, 0, 2), (3, 5, 48), (16, 18, 2000), (4, 64, 10 ** 6)):
        a, b = C.c_int(-1), C.c_int(-1)
        assert lib.ehyb_eigsh_basis(nev, basis, n, C.byref(a), C.byref(b)) == 0
        assert (a.value, b.value) == ec.resolve_basis(nev, basis, n), (nev, basis, n)
    assert ec.resolve_basis(5, 64, 48) == (48, 26) and ec.resolve_basis(3, 5, 48) == (5, 4) and ec.resolve_basis(2, 0, 1) == (1, 2)
    assert lib.ehyb_eigsh_basis(3, 5, 48, None, None) == 0


# ------------------------------------------------------------------ the yardstick itself
def dense_inputs():
    """the inputs of test_gpu_eigsh.py with n <= 2000: (name, A, scale, nev, which, basis)"""
    rng = np.random.default_rng(3)
    import scipy.sparse as sp

    B = (ec.sym_grid(50, 40, 3, False) + sp.diags(rng.uniform(0, 30, 2000))).tocsr()
    s = 1.0 / np.sqrt(B.diagonal())
    out = [("n48-la", ec.sym_grid(8, 6, 2, True), None, 5, "LA", 64), ("n48-sa", ec.sym_grid(8, 6, 2, True), None, 16, "SA", 64),
           ("basis5-la", ec.sym_grid(8, 6, 2), None, 3, "LA", 5), ("basis5-sa", ec.sym_grid(8, 6, 2), None, 3, "SA", 5),
           ("nev16-la", ec.sym_grid(50, 40, 4, True), None, 16, "LA", 64), ("nev16-sa", ec.sym_grid(50, 40, 4, True), None, 16, "SA", 64),
           ("scale-la", B, s, 2, "LA", 0), ("scale-sa", B, s, 2, "SA", 0),
           ("n1", sp.csr_matrix(np.array([[3.5]])), None, 2, "LA", 0), ("n2", sp.csr_matrix(np.array([[2.0, 1.0], [1.0, -1.0]])), None, 2, "LA", 0)]
    return out


def test_cpu_eigsh_on_an_invariant_subspace_smaller_than_nev():
    import scipy.sparse as sp

    A = sp.diags(np.r_[np.ones(20), 2 * np.ones(20), 5 * np.ones(20)]).tocsr()
    ev, X, info = ec.cpu_eigsh(A, 4, "LA")
    assert (info["found"], info["nconv"], info["multiplies"], info["restarts"], info["status"]) == (3, 3, 3, 0, "ok"), info
    assert np.abs(ev - [5.0, 2.0, 1.0]).max() <= 1e-9 * 5.0
    assert np.abs(X @ X.T - np.eye(3)).max() <= 1e-12


def test_cpu_eigsh_reports_a_breakdown():
    A = ec.sym_grid(8, 6, 2)
    v0 = np.ones(48)
    v0[5] = np.nan
    assert ec.cpu_eigsh(A, 3, "LA", v0=v0)[2]["status"] == "breakdown"
    B = A.copy()
    B.data[0] = np.nan
    info = ec.cpu_eigsh(B, 3, "LA")[2]
    assert info["status"] == "breakdown" and info["found"] == info["nconv"] == info["multiplies"] == 0


@pytest.mark.parametrize("case", dense_inputs(), ids=[c[0] for c in dense_inputs()])
def test_cpu_eigsh_against_dense_eigenvalues(case):
    name, A, scale, nev, which, basis = case
    tol = 1e-10
    ev, X, info = ec.cpu_eigsh(A, nev, which, basis=basis, tol=tol, scale=scale)
    D = A.toarray() if scale is None else scale[:, None] * A.toarray() * scale[None, :]
    lam = np.linalg.eigvalsh(D)
    want = min(nev, A.shape[0])
    ref = lam[::-1][:want] if which == "LA" else lam[:want]
    nrm = np.abs(ev).max()
    print(name, info["multiplies"], info["restarts"], info["nconv"], np.abs(ev - ref).max() / nrm)
    assert info["status"] == "ok" and info["found"] == info["nconv"] == want, info
    assert np.abs(ev - ref).max() <= 10 * tol * nrm
    assert max(np.linalg.norm(D @ X[i] - ev[i] * X[i]) for i in range(want)) <= 10 * tol * nrm
    assert np.abs(X @ X.T - np.eye(want)).max() <= 1e-12
