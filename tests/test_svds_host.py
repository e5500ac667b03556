"""ehyb_svds on the host: the dense SVD ehyb_small_svd against numpy.linalg.svd, every argument check of ehyb_svds and of
ehyb_svds_next_step in the order the header states (on plans that were never uploaded: EHYB_ERR_STATE comes last, and what is
wrong with a plan_t is said in ehyb_lsqr's words), how basis = 0 resolves, and the numpy restatement cpu_svds -- the yardstick of
test_gpu_svds.py -- against dense singular values.  Nothing here needs a GPU.

ehyb_small_svd, the bound of test_eigsh_host.py for ehyb_sym_eig: with r(X, sigma, Y) = max_i ||M y_i - sigma_i x_i||_2,
l = max_i ||M^T x_i - sigma_i y_i||_2 and o(Z) = max |Z^T Z - I| for X and for Y, the library may leave at most 4 x what numpy's
own result leaves, numpy's figure floored at rows 2^-52 ||M||_F (the residuals) and rows 2^-52 (the orthogonality); sigma is
falling and within the residual bound of numpy's.  The worst ratio to the bound over all inputs is printed (DESIGN.md section 27
quotes it).

The restatement, tol = 1e-10 (the margins of test_gpu_eigsh.py): |sigma_i - dense| <= 10 tol sigma_0, both residuals
<= 10 tol sigma_0, max |U U^T - I| and max |V V^T - I| <= 1e-12.  cpu_svds leaves at most 8e-15 sigma_0 of error in a value and
2e-14 of orthogonality; the left residual is what the stop rule lets through, up to tol sigma_0.  Multiplies, restarts and the kind
of collapse are those of svds_cases.systems().  Every collapse test of
test_gpu_svds.py counts multiplies exactly, so on its inputs every deciding ratio must be above 2^-60 or below 2^-100: then the
device's order of summation cannot flip a decision."""
import ctypes as C

import numpy as np
import pytest

import eigsh_cases as ec
import svds_cases as sv

ERR_ARG, ERR_STATE = 1, 8
EPS = 2.0 ** -52
TOL = 1e-10
_dp = C.POINTER(C.c_double)

SQUARE = [1, 2, 3, 8, 33, 64]
TALL = [(2, 1), (9, 8), (65, 64)]
SHAPES = [(m, m) for m in SQUARE] + TALL


def small_svd(lib, M, ldm=None):
    rows, cols = M.shape
    ldm = rows if ldm is None else ldm
    Mf = np.full((ldm, cols), np.nan, order="F")
    Mf[:rows] = M
    sg, X, Y = np.full(cols, np.nan), np.full(rows * cols, np.nan), np.full(cols * cols, np.nan)
    rc = lib.ehyb_small_svd(rows, cols, Mf.ctypes.data_as(_dp), ldm, sg.ctypes.data_as(_dp), X.ctypes.data_as(_dp), Y.ctypes.data_as(_dp))
    assert rc == 0, lib.ehyb_last_error()
    return X.reshape(cols, rows).T, sg, Y.reshape(cols, cols).T


def with_sigma(rng, rows, cols, sigma):
    Qx = np.linalg.qr(rng.standard_normal((rows, cols)))[0]
    Qy = np.linalg.qr(rng.standard_normal((cols, cols)))[0]
    return (Qx * sigma) @ Qy.T


def inputs(rows, cols):
    rng = np.random.default_rng(100 * rows + cols)
    R = rng.standard_normal((rows, cols))
    rank = max(cols // 2, 1) if cols > 1 else 1
    Low = rng.standard_normal((rows, rank)) @ rng.standard_normal((rank, cols))
    Zero = R.copy()
    Zero[:, ::2] = 0.0                                         # exactly zero columns: zero sigmas whose x must be completed
    rep = np.repeat([3.0, 3.0, 1.0, 0.25], -(-cols // 4))[:cols]
    # as the driver hands them over: B^T for B = diag(sigma) with an arrow column at k and a bidiagonal behind it
    k = cols // 2
    Bm = np.diag(np.sort(rng.uniform(0.5, 40, cols))[::-1].copy())
    if cols > 1:
        Bm[:k, k] = rng.standard_normal(k) * 10.0 ** rng.integers(-12, 1, k)
        for i in range(k, cols - 1):
            Bm[i, i + 1] = rng.uniform(0.1, 2.0)
    Arrow = np.zeros((rows, cols))
    Arrow[:cols] = Bm.T
    if rows > cols:                                            # a left collapse: one more column of B (row of B^T), no diagonal entry
        Arrow[cols] = rng.standard_normal(cols)
    return {"random": R, "graded": with_sigma(rng, rows, cols, np.logspace(0, -12, cols)), "rank-deficient": Low, "zero-columns": Zero,
            "repeated": with_sigma(rng, rows, cols, rep), "arrow": Arrow, "zero": np.zeros((rows, cols)), "scaled-up": R * 2.0 ** 200,
            "scaled-down": R * 2.0 ** -200}


WORST = {"right": 0.0, "left": 0.0, "orth-x": 0.0, "orth-y": 0.0, "values": 0.0}


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_small_svd_against_numpy(E, rows, cols):
    lib = E.host._lib.load()
    for name, M in inputs(rows, cols).items():
        X, sg, Y = small_svd(lib, M)
        Xn, sn, Ytn = np.linalg.svd(M, full_matrices=False)
        Yn = Ytn.T
        fro = np.linalg.norm(M)
        right = lambda Xs, s, Ys: np.linalg.norm(M @ Ys - Xs * s, axis=0).max()                 # noqa: E731
        left = lambda Xs, s, Ys: np.linalg.norm(M.T @ Xs - Ys * s, axis=0).max()                # noqa: E731
        orth = lambda Z: np.abs(Z.T @ Z - np.eye(Z.shape[1])).max()                              # noqa: E731
        floor_r, floor_o = rows * EPS * fro, rows * EPS
        bounds = {"right": 4 * max(right(Xn, sn, Yn), floor_r), "left": 4 * max(left(Xn, sn, Yn), floor_r),
                  "orth-x": 4 * max(orth(Xn), floor_o), "orth-y": 4 * max(orth(Yn), floor_o)}
        bounds["values"] = max(bounds["right"], bounds["left"])
        got = {"right": right(X, sg, Y), "left": left(X, sg, Y), "orth-x": orth(X), "orth-y": orth(Y), "values": np.abs(sg - sn).max()}
        print(f"{rows}x{cols} {name}: " + ", ".join(f"{k} {got[k]:.3e} / {bounds[k]:.3e}" for k in got))
        assert np.isfinite(sg).all() and np.isfinite(X).all() and np.isfinite(Y).all(), (rows, cols, name)
        assert (np.diff(sg) <= 0).all() and (sg >= 0).all(), (rows, cols, name, "not falling")
        for key in got:
            assert got[key] <= bounds[key], (rows, cols, name, key, got[key], bounds[key])
            WORST[key] = max(WORST[key], got[key] / bounds[key] if bounds[key] else 0.0)
    print("worst ratios to the bound so far:", WORST)


def test_small_svd_keeps_a_small_sigma_that_the_normal_equations_lose(E):
    """sigma = (1, 1e-5, 1e-10, 1e-12) times rotations: M^T M holds the last two at 1e-20 and 1e-24 beside 1, below its rounding"""
    lib = E.host._lib.load()
    rng = np.random.default_rng(4)
    sigma = np.array([1.0, 1e-5, 1e-10, 1e-12])
    M = with_sigma(rng, 6, 4, sigma)
    sg = small_svd(lib, M)[1]
    assert np.abs(sg - sigma).max() <= 4 * 6 * EPS
    gram = np.sqrt(np.abs(np.linalg.eigvalsh(M.T @ M))[::-1])
    assert abs(gram[3] - 1e-12) > 1e-10, "the route through M^T M must lose it, else this test shows nothing"


def test_small_svd_is_deterministic_and_takes_a_leading_dimension(E):
    lib = E.host._lib.load()
    M = inputs(33, 33)["random"]
    want = small_svd(lib, M)
    for got in (small_svd(lib, M), small_svd(lib, M, ldm=40)):
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.int64), b.view(np.int64))
    X, sg, Y = E.small_svd(inputs(9, 8)["random"])
    for a, b in zip((X, sg, Y), small_svd(lib, inputs(9, 8)["random"])):
        assert np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))
    with pytest.raises(E.EhybError):
        E.small_svd(np.zeros((3, 4)))


def test_small_svd_argument_errors(E):
    lib = E.host._lib.load()
    M, sg, X, Y = np.asfortranarray(np.arange(12.0).reshape(4, 3)), np.zeros(3), np.zeros(12), np.zeros(9)
    p = lambda a: a.ctypes.data_as(_dp)                  # noqa: E731
    assert lib.ehyb_small_svd(4, 3, p(M), 4, p(sg), p(X), p(Y)) == 0
    for rows, cols, ldm in ((4, 0, 4), (0, 0, 1), (3, 4, 4), (66, 3, 66), (66, 66, 66), (4, 3, 3), (4, -1, 4)):
        assert lib.ehyb_small_svd(rows, cols, p(M), ldm, p(sg), p(X), p(Y)) == ERR_ARG, (rows, cols, ldm)
        assert b"ehyb_small_svd" in lib.ehyb_last_error()
    assert lib.ehyb_small_svd(4, 3, None, 4, p(sg), p(X), p(Y)) == ERR_ARG
    assert lib.ehyb_small_svd(4, 3, p(M), 4, None, p(X), p(Y)) == ERR_ARG
    assert lib.ehyb_small_svd(4, 3, p(M), 4, p(sg), None, p(Y)) == ERR_ARG
    assert lib.ehyb_small_svd(4, 3, p(M), 4, p(sg), p(X), None) == ERR_ARG
    for bad in (np.inf, np.nan):
        M[1, 2] = bad
        assert lib.ehyb_small_svd(4, 3, p(M), 4, p(sg), p(X), p(Y)) == ERR_ARG and b"finite" in lib.ehyb_last_error()


# ------------------------------------------------------------------ the argument checks and their order
FEM_SMALL = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))
FEM_OTHER = ("fem3d", (12000, 3, 22, 22, 13500, 1, 1))


def host_plan(E, gen=FEM_SMALL, half=False, **kw):
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
    m.reorder(cfg)
    pb = m.part_boundary
    return E.Plan(m, cfg, rows=(0, int(pb[len(pb) // 2])) if half else None, upload=False)


@pytest.fixture(scope="module")
def plan(E):
    p = host_plan(E, direct=2, sym_pairs=0)
    assert p.spmv_t_supported and p.n == 30000
    return p


@pytest.fixture(scope="module")
def part(E):
    p = host_plan(E, half=True, direct=2, sym_pairs=0)
    assert 0 < p.rows[1] < p.n
    return p


@pytest.fixture(scope="module")
def other(E):
    return host_plan(E, gen=FEM_OTHER, direct=2, sym_pairs=0)


@pytest.fixture(scope="module")
def pairs(E):
    p = host_plan(E, direct=2, sym_pairs=1)
    assert not p.spmv_t_supported
    return p


UD, VD, V0 = 0x10000, 0x20000, 0x30000            # never read: every call fails before device work


def call(lib, plan, plan_t=None, v0=V0, nsv=4, basis=0, max_restarts=10, tol=1e-8, U=UD, ldu=None, V=VD, ldv=None, outputs=True):
    n = plan.n if plan is not None else 0
    ldu = n + (n & 1) if ldu is None else ldu
    ldv = n + (n & 1) if ldv is None else ldv
    ints = [C.c_int(-5) for _ in range(4)]
    sg, rs = np.full(16, -5.0), np.full(16, -5.0)
    P = lambda a: C.c_void_p(a) if a else None          # noqa: E731
    rc = lib.ehyb_svds(plan.h if plan is not None else None, plan_t.h if plan_t is not None else None, P(v0), nsv, basis, max_restarts, tol,
                       sg.ctypes.data_as(_dp) if outputs else None, P(U), ldu, P(V), ldv, None,
                       *((C.byref(i) for i in ints) if outputs else (None,) * 4), rs.ctypes.data_as(_dp) if outputs else None)
    assert [i.value for i in ints] == [-5] * 4 and (sg == -5).all() and (rs == -5).all(), "an output was written before device work"
    return rc, lib.ehyb_last_error()


def test_never_uploaded_plans_are_state_errors(E, plan, pairs):
    lib = E.host._lib.load()
    for kw in (dict(), dict(nsv=1), dict(nsv=16, basis=18), dict(basis=64), dict(basis=6), dict(max_restarts=0), dict(tol=0.0), dict(v0=None),
               dict(U=None, ldu=1), dict(V=None, ldv=3), dict(U=None, V=None, ldu=0, ldv=0), dict(outputs=False),
               dict(ldu=plan.n + 2, ldv=plan.n + 4), dict(plan_t=plan)):
        rc, msg = call(lib, plan, **kw)
        assert rc == ERR_STATE and b"ehyb_svds:" in msg and b"plan not uploaded" in msg, (kw, msg)
    rc, msg = call(lib, pairs, plan_t=pairs)             # the caller's statement that A is symmetric: pair storage goes through
    assert rc == ERR_STATE and b"ehyb_svds: plan not uploaded" in msg, msg


RANGES = [dict(nsv=0), dict(nsv=17), dict(nsv=-1), dict(basis=5), dict(basis=65), dict(basis=-1), dict(basis=1, nsv=1), dict(max_restarts=-1)]


@pytest.mark.parametrize("bad", RANGES, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in RANGES])
def test_range_errors(E, plan, bad):
    lib = E.host._lib.load()
    assert call(lib, plan)[0] == ERR_STATE                      # a different error first: a stale text would show
    rc, msg = call(lib, plan, **bad)
    assert rc == ERR_ARG and b"ehyb_svds: nsv" in msg, (bad, msg)


@pytest.mark.parametrize("bad,word", [(dict(tol=-1e-9), b"tol"), (dict(tol=float("nan")), b"tol"), (dict(tol=float("-inf")), b"tol"),
                                      (dict(ldu=1), b"ldu"), (dict(ldu=30001), b"ldu"), (dict(ldv=1), b"ldv"), (dict(ldv=30001), b"ldv"),
                                      (dict(U=UD + 8), b"aligned"), (dict(V=VD + 8), b"aligned"), (dict(v0=V0 + 8), b"aligned")])
def test_other_argument_errors(E, plan, bad, word):
    lib = E.host._lib.load()
    rc, msg = call(lib, plan, **bad)
    assert rc == ERR_ARG and word in msg and b"ehyb_svds:" in msg and b"upload" not in msg, (bad, msg)


def test_the_order_of_the_checks(E, plan, part, other, pairs):
    """a null plan; the ranges; tol; a plan over all rows; the plan_t's dimension and rows; the refusal of ehyb_spmv_t; the
    leading dimensions; the alignment; then the uploads.  The plan_t refusals are ehyb_lsqr's texts under the name ehyb_svds."""
    lib = E.host._lib.load()
    late = dict(ldu=3, U=UD + 8)
    rc, msg = call(lib, None, nsv=0, tol=-1.0)
    assert rc == ERR_ARG and b"ehyb_svds: null argument" in msg, msg
    rc, msg = call(lib, part, plan_t=other, nsv=0, tol=-1.0, **late)
    assert rc == ERR_ARG and b"ehyb_svds: nsv" in msg, msg
    rc, msg = call(lib, part, plan_t=other, tol=float("nan"), **late)
    assert rc == ERR_ARG and b"ehyb_svds: tol" in msg, msg
    rc, msg = call(lib, part, plan_t=other, **late)
    assert rc == ERR_ARG and msg == b"ehyb_svds: needs a plan over all rows", msg
    rc, msg = call(lib, plan, plan_t=other, **late)
    assert rc == ERR_ARG and msg == b"ehyb_svds: plan_t has 12000 rows, plan 30000 (pad a rectangular matrix to square)", msg
    rc, msg = call(lib, plan, plan_t=part, **late)
    assert rc == ERR_ARG and msg == b"ehyb_svds: needs a plan_t over all rows", msg
    rc, msg = call(lib, pairs, **late)
    assert rc == ERR_ARG and b"ehyb_spmv_t: not built for" in msg and pairs.spmv_t_refusal[1].encode() == msg, msg
    rc, msg = call(lib, plan, **late)
    assert rc == ERR_ARG and b"ldu" in msg, msg
    rc, msg = call(lib, plan, U=UD + 8)
    assert rc == ERR_ARG and b"aligned" in msg, msg
    rc, msg = call(lib, plan, ldu=3, U=None)                    # a leading dimension is looked at only with its array
    assert rc == ERR_STATE, msg
    # the same refusals out of ehyb_lsqr, word for word but for the name
    B, X = C.c_void_p(0x10000), C.c_void_p(0x20000)
    for p, pt, ours in ((part, other, call(lib, part, plan_t=other)), (plan, other, call(lib, plan, plan_t=other)),
                        (plan, part, call(lib, plan, plan_t=part)), (pairs, None, call(lib, pairs)), (plan, None, call(lib, plan))):
        rc = lib.ehyb_lsqr(p.h, pt.h if pt is not None else None, B, X, 0.0, 1e-8, 1e-8, 50, 10, None, None)
        assert rc == ours[0] and lib.ehyb_last_error().replace(b"ehyb_lsqr", b"ehyb_svds") == ours[1], (ours, lib.ehyb_last_error())


def test_next_step_checks_its_arguments(E):
    lib = E.host._lib.load()
    P = lambda a: C.c_void_p(a) if a else None          # noqa: E731
    D, W, SL = 0x10000, 0x20000, 0x40000
    nxt = lambda n=10, ld=10, d=D, w=W, s=SL, side=0, j=0: lib.ehyb_svds_next_step(n, ld, P(d), P(w), P(s), side, j, None)      # noqa: E731
    for kw in (dict(n=-1), dict(d=0), dict(w=0), dict(s=0), dict(side=2), dict(side=-1), dict(j=-1), dict(j=-2, side=1), dict(j=64),
               dict(j=64, side=1), dict(ld=9), dict(ld=11), dict(n=11, ld=11), dict(d=D + 8), dict(w=W + 8)):
        assert nxt(**kw) == ERR_ARG and b"ehyb_svds_next_step" in lib.ehyb_last_error(), kw
    # null pointers, then the range, then the pairs
    assert nxt(d=0, j=99, ld=9) == ERR_ARG and b"bad arguments" in lib.ehyb_last_error() and b"j " not in lib.ehyb_last_error()
    assert nxt(j=99, ld=9) == ERR_ARG and b"j 99" in lib.ehyb_last_error()
    assert nxt(ld=9) == ERR_ARG and b"leading dimension" in lib.ehyb_last_error()


# ------------------------------------------------------------------ the basis
def test_the_basis_rule_is_that_of_eigsh(E):
    lib = E.host._lib.load()
    for nsv, basis, n in ((1, 0, 10 ** 6), (9, 0, 10 ** 6), (10, 0, 10 ** 6), (16, 0, 10 ** 6), (5, 64, 48), (16, 64, 48), (2, 0, 1), (2, 0, 2),
                          (3, 5, 48), (16, 18, 2000), (4, 64, 10 ** 6), (16, 40, 1440), (8, 24, 1440), (3, 0, 30), (1, 0, 6)):
        a, b, c, d = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        assert lib.ehyb_svds_basis(nsv, basis, n, C.byref(a), C.byref(b)) == 0
        assert lib.ehyb_eigsh_basis(nsv, basis, n, C.byref(c), C.byref(d)) == 0
        assert (a.value, b.value) == (c.value, d.value) == ec.resolve_basis(nsv, basis, n), (nsv, basis, n)
    assert lib.ehyb_svds_basis(3, 5, 48, None, None) == 0
    assert ec.resolve_basis(4, 0, 1440) == (20, 12) and ec.resolve_basis(16, 40, 1440) == (40, 28)


# ------------------------------------------------------------------ the yardstick itself
SYSTEMS = sv.systems()


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_cpu_svds_against_dense_singular_values(name):
    s = SYSTEMS[name]
    A, nsv = s["A"], s["nsv"]
    trace = []
    sg, U, V, info = sv.cpu_svds(A, nsv, basis=s["basis"], tol=TOL, trace=trace)
    dense = np.linalg.svd(A.toarray(), compute_uv=False)
    want = s.get("found", nsv)
    if want is None:
        want = nsv
    print(name, info["multiplies"], info["restarts"], info["nconv"], info["collapse"])
    assert info["status"] == "ok" and info["found"] == info["nconv"] == want == len(sg), info
    assert (info["multiplies"], info["restarts"], info["collapse"]) == s["expect"], (info, s["expect"])
    if want == 0:
        assert dense.max() == 0.0
        return
    s0 = sg[0]
    err = np.abs(sg - dense[:want]).max()
    right = max(np.linalg.norm(A @ V[i] - sg[i] * U[i]) for i in range(want))
    left = max(np.linalg.norm(A.T @ U[i] - sg[i] * V[i]) for i in range(want))
    ou, ov = np.abs(U @ U.T - np.eye(want)).max(), np.abs(V @ V.T - np.eye(want)).max()
    print(f"  err/s0 {err / s0:.2e} right/s0 {right / s0:.2e} left/s0 {left / s0:.2e} orth {ou:.1e} {ov:.1e}")
    # (repeated-diagonal: 5 and 1 are double and the Krylov space of an exact run holds each once; this run nearly ends at j = 6 with
    # beta^2 at 2^-62 of its column, goes on, and rounding brings the second copy of 5 in -- a true triplet, which dense lists too)
    assert err <= 10 * TOL * s0, err / s0
    assert right <= 10 * TOL * s0 and left <= 10 * TOL * s0, (right / s0, left / s0)
    assert ou <= 1e-12 and ov <= 1e-12, (ou, ov)
    if name in sv.COLLAPSE_SYSTEMS and name != "repeated-diagonal":
        near = [(side, j, r) for side, j, r in trace if 2.0 ** -100 <= r <= 2.0 ** -60]
        assert not near, f"a deciding ratio near the threshold: {near}"
        assert any(r < 2.0 ** -100 for _, _, r in trace) or name == "zero"


def test_cpu_svds_nsv_beyond_the_rank_found():
    """7 x 30 has seven singular values: a left collapse leaves Jl = 7 triplets, whatever nsv asks for"""
    A = SYSTEMS["wide-7x30"]["A"]
    sg, U, V, info = sv.cpu_svds(A, 10, tol=TOL)
    dense = np.linalg.svd(A.toarray(), compute_uv=False)
    assert (info["found"], info["nconv"], info["multiplies"], info["restarts"], info["collapse"]) == (7, 7, 15, 0, "left"), info
    assert np.abs(sg - dense[:7]).max() <= 10 * TOL * sg[0] and (info["resid"] == 0).all()


def test_cpu_svds_on_a_symmetric_matrix_gives_the_largest_magnitudes():
    A = ec.sym_grid(24, 20, 1)
    sg, U, V, info = sv.cpu_svds(A, 4, tol=TOL)
    lam = np.sort(np.abs(np.linalg.eigvalsh(A.toarray())))[::-1]
    assert info["nconv"] == 4 and np.abs(sg - lam[:4]).max() <= 10 * TOL * sg[0]


def test_cpu_svds_reports_a_breakdown():
    A = SYSTEMS["convection-4"]["A"]
    v0 = np.ones(A.shape[0])
    v0[5] = np.nan
    assert sv.cpu_svds(A, 3, v0=v0)[3]["status"] == "breakdown"
    assert sv.cpu_svds(A, 3, v0=np.zeros(A.shape[0]))[3]["status"] == "breakdown"
    B = A.copy()
    B.data[0] = np.nan
    info = sv.cpu_svds(B, 3)[3]
    assert info["status"] == "breakdown" and info["found"] == info["nconv"] == info["multiplies"] == 0


def test_the_exact_cases_build_at_every_size():
    """every case asserts its own exactness while it is built (Fx.f, _ex, exact)"""
    for n in (1, 2, 7, 257):
        sv.start_case(n)
        for side in (sv.LEFT, sv.RIGHT):
            for j in sv.NEXT_J:
                c = sv.next_case(n, side, j, seed=j)
                assert len(c["h"]) == c["count"] == (j if side == sv.LEFT else j + 1) and c["norm"] == 6.0
