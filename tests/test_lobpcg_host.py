"""ehyb_lobpcg on the host: the Rayleigh-Ritz step ehyb_lobpcg_rr against scipy.linalg.eigh(H, G), every argument check of
ehyb_lobpcg and of its step calls that needs no device, and the numpy restatement lobpcg_cases.cpu_lobpcg against eigvalsh.

ehyb_lobpcg_rr.  With lam the nb lowest eigenvalues of the pencil from scipy.linalg.eigh(H, G) and, for a result (theta, Y),
    e = max |theta - lam| / max |lam|,   r = max_i ||H y_i - theta_i G y_i||_2 / ||H||_2,   o = max |Y^T G Y - I|,
the library may leave at most TEN TIMES what lobpcg_cases.numpy_rr -- the same rules with numpy.linalg.eigh for the two dense
problems -- leaves on the same input, figure by figure, both measured against the same scipy result.  Where numpy_rr leaves exactly
zero (mc = 1: theta = H / G in the same operations) 4 eps = 8.9e-16, the size of one rounding of theta, stands in for it.  Figures
of numpy_rr and of the library, the largest over the five seeds, mc = 24: e 1.2e-15 and 3.3e-15, r 2.4e-17 and 3.6e-17, o 2.7e-15
and 8.7e-15; mc = 8: e 1.5e-15 and 1.8e-15, r 1.8e-17 and 2.4e-17, o 2.4e-15 and 2.7e-15."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla

import eigsh_cases as ec
import lobpcg_cases as lc

ERR_ARG, ERR_STATE = 1, 8
FLOOR = 4 * np.finfo(np.float64).eps
_dp = C.POINTER(C.c_double)


def pencil(mc, seed, n=200):
    """a well-conditioned pencil: G = S^T S, H = S^T A S for a random n x mc S with columns of mixed length and a random symmetric A"""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n, mc)) * rng.uniform(0.1, 10.0, mc)[None, :]
    A = rng.standard_normal((n, n))
    A = (A + A.T) / 2
    return S.T @ S, S.T @ (A @ S)


def figures(G, H, theta, Y, lam):
    nb = len(theta)
    e = np.abs(theta - lam[:nb]).max() / np.abs(lam).max()
    r = max(np.linalg.norm(H @ Y[:, i] - theta[i] * (G @ Y[:, i])) for i in range(nb)) / np.linalg.norm(H, 2)
    o = np.abs(Y.T @ G @ Y - np.eye(nb)).max()
    return np.array([e, r, o])


@pytest.mark.parametrize("mc", [1, 2, 8, 17, 24])
def test_rr_against_scipy(E, mc):
    nb = min(mc, 8)
    cases = [pencil(mc, 10 * mc + s) for s in range(5)]
    lams = [sla.eigh(lc.mirror(H), lc.mirror(G), eigvals_only=True) for G, H in cases]
    for (G, H), lam in zip(cases, lams):
        yard = figures(G, H, *lc.numpy_rr(G, H, nb)[:2], lam)
        bound = 10 * np.where(yard == 0, FLOOR, yard)
        theta, Y, rank = E.lobpcg_rr(G, H, nb)
        got = figures(G, H, theta, Y, lam)
        print(f"mc={mc} numpy_rr {yard} library {got}")
        assert rank == mc and (np.diff(theta) >= 0).all()
        assert (got <= bound).all(), (mc, got, bound)


def test_rr_drops_a_zero_column(E):
    """column 3 of S is zero: row 3 of Y is zero and the rest is the pencil without it"""
    mc, nb, z = 9, 4, 3
    G, H = pencil(mc, 7)
    G[z, :] = G[:, z] = H[z, :] = H[:, z] = 0.0
    theta, Y, rank = E.lobpcg_rr(G, H, nb)
    rest = [i for i in range(mc) if i != z]
    Gr, Hr = G[np.ix_(rest, rest)], H[np.ix_(rest, rest)]
    lam = sla.eigh(Hr, Gr, eigvals_only=True)
    yard = figures(Gr, Hr, *lc.numpy_rr(Gr, Hr, nb)[:2], lam)
    assert rank == mc - 1 and (Y[z] == 0).all()
    assert (figures(Gr, Hr, theta, Y[rest], lam) <= 10 * np.where(yard == 0, FLOOR, yard)).all()
    t2, Y2, r2 = lc.numpy_rr(G, H, nb)
    assert r2 == rank and (Y2[z] == 0).all()


def test_rr_numerical_rank(E):
    """S = B with nb (then nb - 1) rows and 12 columns: G = B^T B has rank nb exactly and, in fp64, eigenvalues of the scaled G at
    1e-16 of the largest, far below the 2^-40 cut.  With rank nb the Ritz values are the eigenvalues of the small A itself; with
    rank nb - 1 the step must refuse with "rank"."""
    mc, nb = 12, 4
    rng = np.random.default_rng(3)
    for k in (nb, nb - 1):
        B = rng.standard_normal((k, mc))
        A = rng.standard_normal((k, k))
        A = (A + A.T) / 2
        G, H = B.T @ B, B.T @ A @ B
        if k == nb:
            theta, Y, rank = E.lobpcg_rr(G, H, nb)
            lam = np.linalg.eigvalsh(A)
            tn, Yn, rn = lc.numpy_rr(G, H, nb)
            assert rank == rn == nb
            assert np.abs(tn - lam).max() > 0 and np.abs(Yn.T @ G @ Yn - np.eye(nb)).max() > 0
            assert np.abs(theta - lam).max() <= 10 * np.abs(tn - lam).max(), (theta, tn, lam)
            assert np.abs(Y.T @ G @ Y - np.eye(nb)).max() <= 10 * np.abs(Yn.T @ G @ Yn - np.eye(nb)).max()
        else:
            with pytest.raises(E.EhybError) as ei:
                E.lobpcg_rr(G, H, nb)
            assert ei.value.code == ERR_ARG and "rank" in str(ei.value)
            with pytest.raises(lc.RRError, match="rank"):
                lc.numpy_rr(G, H, nb)


def test_rr_reads_the_upper_triangles_and_is_deterministic(E):
    G, H = pencil(17, 5)
    want = E.lobpcg_rr(G, H, 6)
    junk_g, junk_h = np.triu(G) + np.tril(np.full_like(G, np.nan), -1), np.triu(H) + np.tril(np.full_like(H, 1e300), -1)
    for got in (E.lobpcg_rr(G, H, 6), E.lobpcg_rr(junk_g, junk_h, 6)):
        assert np.array_equal(got[0].view(np.int64), want[0].view(np.int64)) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
        assert got[2] == want[2] == 17


def test_rr_argument_errors(E):
    lib = E.host._lib.load()
    G, H = (np.asfortranarray(m) for m in pencil(5, 1))
    theta, Y, rank = np.zeros(8), np.zeros(40), C.c_int(-1)
    p = lambda a: a.ctypes.data_as(_dp)          # noqa: E731
    rr = lambda mc=5, g=G, h=H, nb=3, t=theta, y=Y: lib.ehyb_lobpcg_rr(mc, p(g) if g is not None else None, p(h) if h is not None else None,  # noqa: E731
                                                                      nb, p(t) if t is not None else None, p(y) if y is not None else None, C.byref(rank))
    assert rr() == 0 and rank.value == 5
    assert lib.ehyb_lobpcg_rr(5, p(G), p(H), 3, p(theta), p(Y), None) == 0
    for kw in (dict(mc=0), dict(mc=25), dict(nb=0), dict(nb=9), dict(nb=6), dict(g=None), dict(h=None), dict(t=None), dict(y=None)):
        assert rr(**kw) == ERR_ARG and b"ehyb_lobpcg_rr" in lib.ehyb_last_error(), kw
    for bad in (np.nan, np.inf):
        for which in (0, 1):
            M = [G.copy(order="F"), H.copy(order="F")]
            M[which][1, 3] = bad                                     # an entry of the upper triangle
            assert rr(g=M[0], h=M[1]) == ERR_ARG and b"finite" in lib.ehyb_last_error()
    Gn = G.copy(order="F")
    Gn[2, 2] = -1.0
    assert rr(g=Gn) == ERR_ARG and b"negative" in lib.ehyb_last_error()
    with pytest.raises(lc.RRError):
        lc.numpy_rr(Gn, H, 3)


# ------------------------------------------------------------------ the argument checks of the solver and their order
FEM_SMALL = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))
X, D0, V0 = 0x10000, 0x20000, 0x30000            # never read: every call fails before device work


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


@pytest.fixture(scope="module")
def other_coarse(E):
    """a coarse object of 10 rows, not uploaded"""
    return E.Coarse.raw(10, np.arange(10) // 5, np.eye(2), upload=False)


def call(lib, plan, coarse=None, dinv=D0, x0=V0, ldx0=None, nev=4, block=0, max_iter=10, tol=1e-8, anorm=0.0, evecs=X, ldv=None, outputs=True):
    n = plan.n if plan is not None else 0
    ldv = n + (n & 1) if ldv is None else ldv
    ldx0 = n + (n & 1) if ldx0 is None else ldx0
    ints = [C.c_int(-5) for _ in range(3)]
    ev, rs = np.full(8, -5.0), np.full(8, -5.0)
    rc = lib.ehyb_lobpcg(plan.h if plan is not None else None, coarse.h if coarse is not None else None, C.c_void_p(dinv) if dinv else None,
                         C.c_void_p(x0) if x0 else None, ldx0, nev, block, max_iter, tol, anorm, ev.ctypes.data_as(_dp) if outputs else None,
                         C.c_void_p(evecs) if evecs else None, ldv, None, *((C.byref(i) for i in ints) if outputs else (None,) * 3),
                         rs.ctypes.data_as(_dp) if outputs else None)
    assert [i.value for i in ints] == [-5] * 3 and (ev == -5).all() and (rs == -5).all(), "an output was written before device work"
    return rc, lib.ehyb_last_error()


def test_never_uploaded_plan_is_a_state_error(E, plan):
    lib = E.host._lib.load()
    for kw in (dict(), dict(nev=1), dict(nev=8), dict(nev=3, block=8), dict(block=4), dict(max_iter=0), dict(tol=0.0), dict(anorm=5.0),
               dict(dinv=None, x0=None), dict(evecs=None, ldv=1), dict(x0=None, ldx0=1), dict(outputs=False), dict(ldv=plan.n + 2)):
        rc, msg = call(lib, plan, **kw)
        assert rc == ERR_STATE and b"ehyb_lobpcg:" in msg and b"upload" in msg, (kw, msg)


RANGES = [dict(nev=0), dict(nev=9), dict(nev=-1), dict(nev=4, block=3), dict(block=9), dict(block=-1), dict(nev=9, block=9), dict(max_iter=-1)]


@pytest.mark.parametrize("bad", RANGES, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in RANGES])
def test_range_errors(E, plan, bad):
    lib = E.host._lib.load()
    rc, msg = call(lib, plan, **bad)
    assert rc == ERR_ARG and b"ehyb_lobpcg: nev" in msg, (bad, msg)


@pytest.mark.parametrize("bad,word", [(dict(tol=-1e-9), b"tol"), (dict(tol=float("nan")), b"tol"), (dict(anorm=-1.0), b"anorm"),
                                      (dict(anorm=float("nan")), b"anorm"), (dict(anorm=float("inf")), b"anorm"), (dict(ldv=1), b"ldv"),
                                      (dict(ldv=30001), b"ldv"), (dict(ldx0=29998), b"ldx0"), (dict(ldx0=30001), b"ldx0"),
                                      (dict(evecs=X + 8), b"aligned"), (dict(dinv=D0 + 8), b"aligned"), (dict(x0=V0 + 8), b"aligned")])
def test_other_argument_errors(E, plan, bad, word):
    lib = E.host._lib.load()
    assert plan.n == 30000
    rc, msg = call(lib, plan, **bad)
    assert rc == ERR_ARG and word in msg and b"upload" not in msg, (bad, msg)


def test_null_plan_comes_first(E):
    rc, msg = call(E.host._lib.load(), None, nev=0, tol=-1.0)
    assert rc == ERR_ARG and b"null argument" in msg, msg


def test_a_block_wider_than_the_matrix(E):
    cfg = E.make_config(direct=1)
    A = ec.sym_grid(2, 2, 1, plant=False)
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=False)
    m.reorder(cfg)
    p = E.Plan(m, cfg, upload=False)
    lib = E.host._lib.load()
    rc, msg = call(lib, p, nev=5)
    assert rc == ERR_ARG and b"block of 5" in msg, msg
    assert call(lib, p, nev=4)[0] == ERR_STATE


# in the order of the header; each entry: the fault, and a word of its message
STAGES = [(dict(nev=0), b"nev"), (dict(tol=float("nan")), b"tol"), ("part", b"all rows"), (dict(ldv=3), b"ldv"), (dict(evecs=X + 8), b"aligned"),
          ("coarse", b"coarse object has 10 rows")]


def test_the_order_of_the_checks(E, plan, part, other_coarse):
    """all the faults from stage i on at once: stage i's message comes; a coarse object with another row count is an argument error
    that comes before the state of the plan, a coarse object never uploaded a state error that comes after it"""
    lib = E.host._lib.load()
    for first in range(len(STAGES)):
        kw, p = {}, plan
        for fault, _ in STAGES[first:]:
            if fault == "part":
                p = part
            elif fault == "coarse":
                kw["coarse"] = other_coarse
            else:
                kw.update(fault)
        if "ldv" not in kw:
            kw["ldv"] = None
        rc, msg = call(lib, p, **kw)
        assert rc == ERR_ARG and STAGES[first][1] in msg, (first, kw, msg)
    same_rows = E.Coarse.raw(plan.n, np.arange(plan.n) % 3, np.eye(3), upload=False)
    rc, msg = call(lib, plan, coarse=same_rows)
    assert rc == ERR_STATE and b"plan not uploaded" in msg, msg


def test_step_calls_check_their_arguments(E):
    lib = E.host._lib.load()
    P = lambda a: C.c_void_p(a) if a else None          # noqa: E731
    S, AS, G, H, SC, TH, DI, W, R2 = (0x10000 * k for k in range(1, 10))
    gram = lambda n=10, ld=10, s=S, a=AS, mc=3, g=G, h=H, sc=SC: lib.ehyb_lobpcg_gram_step(n, ld, P(s), P(a), mc, P(g), P(h), P(sc), None)    # noqa: E731
    for kw in (dict(n=-1), dict(s=0), dict(a=0), dict(g=0), dict(h=0), dict(sc=0), dict(mc=0), dict(mc=25), dict(ld=9), dict(ld=11), dict(ld=8),
               dict(s=S + 8), dict(a=AS + 8)):
        assert gram(**kw) == ERR_ARG and b"ehyb_lobpcg_gram_step" in lib.ehyb_last_error(), kw
    assert gram(s=0, mc=99, ld=9) == ERR_ARG and b"bad arguments" in lib.ehyb_last_error() and b"mc " not in lib.ehyb_last_error()
    assert gram(mc=99, ld=9) == ERR_ARG and b"mc 99" in lib.ehyb_last_error()
    assert gram(ld=9) == ERR_ARG and b"leading dimension" in lib.ehyb_last_error()
    res = lambda n=10, ld=10, x=S, ax=AS, nb=3, th=TH, di=DI, mask=5, ldw=12, w=W, r2=R2, sc=SC: lib.ehyb_lobpcg_resid_step(    # noqa: E731
        n, ld, P(x), P(ax), nb, P(th), P(di), mask, ldw, P(w), P(r2), P(sc), None)
    for kw in (dict(n=-1), dict(x=0), dict(ax=0), dict(th=0), dict(r2=0), dict(sc=0), dict(nb=0), dict(nb=9), dict(mask=8), dict(w=0),
               dict(ld=9), dict(ld=8), dict(ldw=11), dict(ldw=8), dict(x=S + 8), dict(ax=AS + 8), dict(di=DI + 8), dict(w=W + 8)):
        assert res(**kw) == ERR_ARG and b"ehyb_lobpcg_resid_step" in lib.ehyb_last_error(), kw


# ------------------------------------------------------------------ the yardstick itself
def test_start_block_is_the_hash_of_the_header():
    X0 = lc.start_block(1000, 8)
    for i, j in ((0, 0), (999, 7), (123, 4)):
        h = ((i + 1) * 2654435761 + (j + 1) * 40503) & 0xFFFFFFFF
        h ^= h >> 15
        h = (h * 2246822519) & 0xFFFFFFFF
        h ^= h >> 13
        assert X0[j, i] == ((h & 2047) - 1023.5) / 1024
    assert np.abs(X0).max() < 1 and np.linalg.matrix_rank(X0) == 8


@pytest.mark.parametrize("nev,block", [(3, 0), (1, 0), (2, 5)])
def test_cpu_lobpcg_against_eigvalsh(nev, block):
    """the restatement on the 8 x 6 grid: converged, the true residual and the eigenvalue error within the bounds the device tests use"""
    A, tol = ec.sym_grid(8, 6, 2), 1e-10
    lam = np.linalg.eigvalsh(A.toarray())
    ev, Xv, info = lc.cpu_lobpcg(A, nev, block=block, tol=tol)
    nrm = np.abs(ev).max()
    assert info["status"] == "ok" and info["nconv"] == nev and 0 < info["iters"] < 100, info
    assert np.abs(ev - lam[:nev]).max() <= 10 * tol * nrm
    assert max(np.linalg.norm(A @ Xv[i] - ev[i] * Xv[i]) for i in range(nev)) <= 10 * tol * nrm
    assert np.abs(Xv @ Xv.T - np.eye(nev)).max() <= 1e-12 and info["orth"] <= 1e-12


def test_cpu_lobpcg_breakdown_and_max_iter():
    A = ec.sym_grid(8, 6, 2)
    X0 = lc.start_block(48, 3)
    X0[1, 5] = np.nan
    assert lc.cpu_lobpcg(A, 3, X0=X0)[2]["status"] == "breakdown"
    info = lc.cpu_lobpcg(A, 3, max_iter=0)[2]
    assert info["status"] == "ok" and info["iters"] == 0 and info["multiplies"] == 3 and info["nconv"] < 3
    info = lc.cpu_lobpcg(A, 3, max_iter=2, tol=1e-12)[2]
    assert info["iters"] == 2 and info["multiplies"] == 9 and info["nconv"] < 3
