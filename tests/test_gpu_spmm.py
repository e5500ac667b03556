"""ehyb_spmm: Y = A X for k columns per pass over the matrix, on the device.

Every kernel path is checked column by column against the EXACT product (exact_cases.py: integer values and x, so
the product is one number whatever the order of summation), for k = 1..8 (several passes where k > k_max) and both
explicit walks; the layout (leading dimensions, gaps, rows outside the plan) is pinned, plain storage is checked to
do the one-vector kernel's arithmetic bit for bit on real data, and the non-finite contract of ehyb_spmv per column.
Everything runs in the permuted numbering: X is drawn there and the exact reference is the permuted matrix's product."""
import ctypes as C

import numpy as np
import pytest

from exact_cases import assert_exact, exact_reference, integer_values, integer_x, nonfinite_reference, value_class
from fuzz_cases import build, random_config_kwargs, random_matrix
from util import Case, fem_plus_rmat

pytestmark = pytest.mark.gpu

LDS_MAX = 20480
FEM = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))
STENCIL = ("stencil2d", (150, 150, 5, 3000, 1))
RMAT11 = ("rmat", (11, 1 << 17, 3))
KS = (1, 2, 3, 4, 5, 8)


def _sync(E):
    assert E.host._lib.load().ehyb_dev_sync() == 0


def spmm(E, plan, X, ldx=None, ldy=None, walk=None, x_gap=np.nan, Y0=None):
    """One ehyb_spmm of the k columns X[j] (length n) -> Y as a (k, ldy) array.  The gaps between the X columns hold x_gap,
    Y starts as Y0 (default: NaN everywhere)."""
    X = np.atleast_2d(X)
    k, n = X.shape
    ldx = n if ldx is None else ldx
    ldy = n if ldy is None else ldy
    Xb = np.full((k, ldx), x_gap)
    Xb[:, :n] = X
    Yb = np.full((k, ldy), np.nan) if Y0 is None else np.array(Y0, dtype=np.float64).reshape(k, ldy)
    dx, dy = E.DeviceBuffer(k * ldx).upload(Xb.ravel()), E.DeviceBuffer(k * ldy).upload(Yb.ravel())
    plan.spmm(dx.ptr, dy.ptr, k, ldx=ldx, ldy=ldy, walk=walk)
    _sync(E)
    Y = dy.download().reshape(k, ldy)
    dx.free(), dy.free()
    return Y


def spmv(E, plan, x, walk):
    n = len(x)
    dx, dy = E.DeviceBuffer(n).upload(x), E.DeviceBuffer(n).upload(np.full(n, np.nan))
    plan.spmv(dx.ptr, dy.ptr, walk=walk)
    _sync(E)
    y = dy.download()
    dx.free(), dy.free()
    return y


class IntCase:
    """generate -> integer values -> reorder; k integer columns (seeds 1..k) in the permuted numbering and their exact products."""

    def __init__(self, E, O, gen, cfg, symmetric=True, k=max(KS)):
        m = fem_plus_rmat(E, cfg) if gen == "fem_plus_rmat" else E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
        m.V[:] = integer_values(m.I, m.J, symmetric)
        m.reorder(cfg)
        self.m, self.n = m, m.n
        self.X = np.stack([integer_x(m.n, j + 1) for j in range(k)])
        self.Y = np.stack([exact_reference(m.n, m.I, m.J, m.V, x) for x in self.X])


def is_direct(plan, n):
    st = plan.stats
    return st["nnz_ell"] == 0 and st["nnz_er"] == st["nnz"] and st["er_segments"] == n


def _split_rows(plan):
    return bool((plan.array("er_seg_row") < 0).any())


def _slab_words(plan):
    return plan.array("slab_meta").reshape(-1, 4)[:, 3]


# (id, matrix, config, symmetric values, what the stats must show, k_max)
PATHS = [
    ("plain-shared-columns", FEM, dict(lds_doubles=LDS_MAX // 4, direct=2), True,
     lambda p, n: p.stats["nnz_ell"] > 0 and p.stats["sym_pairs"] == 0 and (_slab_words(p) & 0x3f).max() > 0, 4),
    ("plain-relative-columns", ("banded", (1024 * 64, 32, 1024)), dict(lds_doubles=LDS_MAX // 2, direct=2, threads=512), True,
     lambda p, n: bool(np.any(_slab_words(p) & 0x80)) and p.stats["nnz_er"] == 0, 2),
    ("halo-t512-lds64", STENCIL, dict(window_mode=2, threads=512, lds_doubles=64), True,
     lambda p, n: p.stats["nnz_ell"] > 0, 4),
    ("refwindow-t256-csr", FEM, dict(window_mode=1, threads=256, lds_doubles=LDS_MAX // 2, fuse_er=2), True,
     lambda p, n: p.stats["nnz_ell"] > 0 and p.stats["nnz_er"] > 0 and p.stats["er_inline"] == 0, 2),
    ("sym-pairs", FEM, dict(lds_doubles=LDS_MAX // 4, sym_pairs=1), True,
     lambda p, n: p.stats["sym_pairs"] > 0.2 * p.stats["nnz"] and {1, 2} <= set(np.unique(p.array("lane_group") >> 6).tolist()), 4),
    ("sym-pairs-t512-k3", FEM, dict(lds_doubles=LDS_MAX // 3, threads=512, sym_pairs=1), True,
     lambda p, n: p.stats["sym_pairs"] > 0.2 * p.stats["nnz"], 3),
    ("inline-residual", FEM, dict(window_mode=1, lds_doubles=LDS_MAX // 4, fuse_er=1), True,
     lambda p, n: p.stats["er_inline"] > 0 and p.stats["nnz_er"] > 0, 4),
    ("csr-split-rows", RMAT11, dict(window_mode=1, lds_doubles=256, er_seg_len=16, er_mode=1, fuse_er=2), False,
     lambda p, n: _split_rows(p) and p.stats["er_inline"] == 0 and p.stats["er_partials"] == 0, 4),
    ("direct", ("rmat", (13, 1 << 18, 3)), dict(), False, lambda p, n: is_direct(p, n), 4),
    ("panel-fallback", "fem_plus_rmat", dict(partitioner=1, er_mode=2, lds_doubles=4096), False,
     lambda p, n: p.stats["er_partials"] > 0 and p.stats["nnz_ell"] > 0, 1),
]


@pytest.mark.parametrize("name,gen,kw,sym,taken,kmax", PATHS, ids=[p[0] for p in PATHS])
def test_exact_every_path(E, O, gpu, name, gen, kw, sym, taken, kmax):
    cfg = E.make_config(**kw)
    c = IntCase(E, O, gen, cfg, symmetric=sym)
    plan = E.Plan(c.m, cfg)
    assert taken(plan, c.n), (name, plan.stats)
    if kmax == 1:
        assert plan.spmm_max_k == 1, name
    else:
        assert plan.spmm_max_k >= kmax, (name, plan.spmm_max_k)
    for k in KS:
        for walk in (0, 1):
            Y = spmm(E, plan, c.X[:k], walk=walk)
            for j in range(k):
                assert_exact(Y[j], c.Y[j], f"{name} k={k} walk={walk} column {j}")


@pytest.mark.parametrize("sym", [0, 1])
def test_layout_gaps_and_rows_outside_the_plan(E, O, gpu, sym):
    """ldx = n + 7, ldy = n + 5, NaN in every gap of X and Y; a plan of the middle partitions only: its rows are the exact
    product, every other row of every column and every Y gap is what it was."""
    cfg = E.make_config(lds_doubles=LDS_MAX // 4, sym_pairs=sym, direct=2)
    c = IntCase(E, O, FEM, cfg, k=4)
    pb = c.m.part_boundary
    assert len(pb) >= 5
    r0, r1 = int(pb[1]), int(pb[-2])
    n = c.n
    for rows in ((0, n), (r0, r1)):
        plan = E.Plan(c.m, cfg, rows=rows)
        assert plan.spmm_max_k >= 4
        for k in (3, 4):
            Y0 = np.full((k, n + 5), np.nan)
            Y0[:, :n] = np.arange(n) * 0.5 + 3.0            # what rows outside the plan keep
            for walk in (0, 1):
                Y = spmm(E, plan, c.X[:k], ldx=n + 7, ldy=n + 5, walk=walk, Y0=Y0)
                assert np.isnan(Y[:, n:]).all(), "a gap of Y was written"
                inside = np.zeros(n, dtype=bool)
                inside[rows[0]:rows[1]] = True
                for j in range(k):
                    assert np.array_equal(Y[j, :n][~inside], Y0[j, :n][~inside]), f"rows {rows}: a row outside the plan changed"
                    assert_exact(Y[j, :n][inside], c.Y[j][inside], f"rows {rows} k={k} walk={walk} column {j}")
        plan.destroy()


@pytest.mark.parametrize("name,kw", [
    ("window-csr-residual", dict(window_mode=1, lds_doubles=LDS_MAX // 4, fuse_er=2)),
    ("window-halo", dict(lds_doubles=LDS_MAX // 4, direct=2)),
    ("inline-residual", dict(window_mode=1, lds_doubles=LDS_MAX // 4, fuse_er=1)),
    ("direct", dict(direct=1)),
], ids=lambda v: v if isinstance(v, str) else None)
def test_plain_storage_is_the_one_vector_arithmetic(E, O, gpu, name, kw):
    """Real-valued data: column j of a plain-storage multiply is ehyb_spmv of X[:, j] on the same plan, bit for bit."""
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(FEM[0], *FEM[1], cfg=cfg)
    m.reorder(cfg)
    plan = E.Plan(m, cfg)
    assert plan.stats["sym_pairs"] == 0 and not _split_rows(plan)
    assert plan.spmm_max_k == 4
    X = np.random.default_rng(5).standard_normal((5, m.n))
    for walk in (0, 1):
        ys = [spmv(E, plan, x, walk) for x in X]
        for k in (2, 3, 4, 5):
            Y = spmm(E, plan, X[:k], walk=walk)
            for j in range(k):
                assert np.array_equal(Y[j], ys[j]), f"{name} k={k} walk={walk} column {j}: not the one-vector result"


def test_symmetric_pairs_agree_with_the_one_vector_multiply(E, O, gpu):
    """Symmetric pair storage: the order of the LDS adds is free -- agreement within the tolerance of the sym tests."""
    cfg = E.make_config(lds_doubles=LDS_MAX // 4, sym_pairs=1)
    c = Case(E, O, *FEM, cfg)
    plan = E.Plan(c.m, cfg)
    assert plan.stats["sym_pairs"] > 0 and plan.spmm_max_k == 4
    rng = np.random.default_rng(9)
    X = np.stack([c.xp] + [rng.uniform(-1, 1, c.n) for _ in range(3)])
    Y = spmm(E, plan, X, walk=1)
    for j in range(4):
        y1 = spmv(E, plan, X[j], 1)
        scale = O.abs_rowsum(c.n, c.m.I, c.m.J, c.m.V, X[j])      # (c.m was reordered in place: the permuted numbering)
        bad, worst = O.check_strict(Y[j], y1, scale)
        assert bad == 0, f"column {j}: worst {worst:.3e}"
    bad, worst = c.check(Y[0])
    assert bad == 0, f"column 0 against the CPU product: worst {worst:.3e}"


@pytest.mark.parametrize("seed", range(300, 330))
def test_exact_random_plans(E, O, gpu, seed):
    """The fuzz configurations with lds_doubles divided by a random k in {2, 3, 4}: exact on integer data for k and k + 1."""
    rng = np.random.default_rng(seed)
    random_matrix(rng)
    lds = random_config_kwargs(rng)["lds_doubles"]     # what build() draws for this seed
    kdiv = int(np.random.default_rng(seed + 1000).integers(2, 5))
    m, cfg, kw, x, y_ref, scale = build(E, O, seed, exact=True, lds_doubles=max(64, lds // kdiv))
    plan = E.Plan(m, cfg)
    xp = E.vector_reorder(x, m.reorder_list)
    X = np.stack([xp] + [integer_x(m.n, seed * 10 + j) for j in range(1, kdiv + 1)])
    Yref = np.stack([E.vector_reorder(y_ref, m.reorder_list)] + [exact_reference(m.n, m.I, m.J, m.V, xj) for xj in X[1:]])
    if m.nnz:
        assert np.array_equal(exact_reference(m.n, m.I, m.J, m.V, xp), Yref[0])   # the permuted matrix's product is the permuted y
    for k in (kdiv, kdiv + 1):
        for walk in (0, 1):
            Y = spmm(E, plan, X[:k], walk=walk)
            for j in range(k):
                assert_exact(Y[j], Yref[j], f"{kw} k_max={plan.spmm_max_k} k={k} walk={walk} column {j}")


NONFINITE = [("plain", dict(lds_doubles=LDS_MAX // 4, direct=2)), ("sym", dict(lds_doubles=LDS_MAX // 4, sym_pairs=1)),
             ("csr-residual", dict(window_mode=1, lds_doubles=LDS_MAX // 4, fuse_er=2))]


@pytest.mark.parametrize("name,kw", NONFINITE, ids=[v[0] for v in NONFINITE])
def test_nonfinite_x_stays_in_its_column(E, O, gpu, name, kw):
    """NaN / inf in column 1 of X: column 1 follows the ehyb_spmv contract (rows that store such a column are non-finite, the
    others exact or NaN through padding); columns 0, 2, 3 are exact."""
    cfg = E.make_config(**kw)
    c = IntCase(E, O, FEM, cfg, k=4)
    plan = E.Plan(c.m, cfg)
    rng = np.random.default_rng(11)
    X = c.X[:4].copy()
    cols = np.unique(np.concatenate([[0], rng.choice(np.arange(1, c.n), 6, replace=False)]))
    X[1, cols] = np.resize([np.nan, np.inf, -np.inf], len(cols))
    y_ref = nonfinite_reference(c.n, c.m.I, c.m.J, c.m.V, X[1])
    stores = np.zeros(c.n, dtype=bool)
    stores[c.m.I[np.isin(c.m.J, cols)]] = True
    for walk in (0, 1):
        Y = spmm(E, plan, X, walk=walk)
        for j in (0, 2, 3):
            assert_exact(Y[j], c.Y[j], f"{name} walk={walk}: column {j} was reached from column 1")
        y = Y[1]
        assert not np.isfinite(y[stores]).any(), (name, walk, "a non-finite x was lost")
        assert np.isnan(y[stores & np.isnan(y_ref)]).all(), (name, walk, "a NaN turned into something else")
        other = ~stores
        assert ((y[other] == y_ref[other]) | np.isnan(y[other])).all(), (name, walk, "a row without a non-finite column is neither exact nor NaN")


@pytest.mark.parametrize("name,kw", NONFINITE, ids=[v[0] for v in NONFINITE])
def test_nonfinite_matrix_reaches_the_same_rows_in_every_column(E, O, gpu, name, kw):
    cfg = E.make_config(**kw)
    c = IntCase(E, O, FEM, cfg, k=4)
    rng = np.random.default_rng(13)
    picks = rng.choice(c.m.nnz, 9, replace=False)
    c.m.V[picks] = np.resize([np.nan, np.inf, -np.inf], len(picks))
    plan = E.Plan(c.m, cfg)
    refs = [nonfinite_reference(c.n, c.m.I, c.m.J, c.m.V, x) for x in c.X[:4]]
    nan_rows = np.zeros(c.n, dtype=bool)
    nan_rows[c.m.I[picks[0::3]]] = True
    for walk in (0, 1):
        Y = spmm(E, plan, c.X[:4], walk=walk)
        for j in range(4):
            assert np.array_equal(value_class(Y[j]), value_class(refs[j])), (name, walk, j)
            assert_exact(Y[j], refs[j], f"{name} walk={walk} column {j}")
            assert np.isnan(Y[j][nan_rows]).all()


def _hip():
    hip = C.CDLL("libamdhip64.so")
    for f in ("hipStreamBeginCapture", "hipStreamEndCapture", "hipGraphInstantiate", "hipGraphLaunch", "hipStreamSynchronize",
              "hipGraphExecDestroy", "hipGraphDestroy"):
        getattr(hip, f).restype = C.c_int
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphInstantiate.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    hip.hipGraphLaunch.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipGraphExecDestroy.argtypes = [C.c_void_p]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    return hip


@pytest.mark.parametrize("name,kw,k", [("sym-k4", dict(lds_doubles=LDS_MAX // 4, sym_pairs=1, ell_alternate=1), 4),
                                       ("plain-k5", dict(lds_doubles=LDS_MAX // 4, direct=2, ell_alternate=1), 5)],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_captured_multiplies(E, O, gpu, name, kw, k):
    """Four ehyb_spmm calls on one stream captured into a hipGraph with explicit alternating walks; every replay exact."""
    cfg = E.make_config(**kw)
    c = IntCase(E, O, FEM, cfg, k=k)
    plan = E.Plan(c.m, cfg)
    n = c.n
    hip = _hip()
    st = E.Stream()
    dx = E.DeviceBuffer(k * n).upload(c.X[:k].ravel())
    dys = [E.DeviceBuffer(k * n) for _ in range(4)]
    graph, exe = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamBeginCapture(st.ptr, 1) == 0                     # hipStreamCaptureModeThreadLocal
    try:
        for i, dy in enumerate(dys):
            plan.spmm(dx.ptr, dy.ptr, k, stream=st.ptr, walk=i & 1)
    finally:
        assert hip.hipStreamEndCapture(st.ptr, C.byref(graph)) == 0
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
    try:
        for rep in range(3):
            for dy in dys:
                dy.upload(np.full(k * n, np.nan))
            assert hip.hipGraphLaunch(exe, st.ptr) == 0
            assert hip.hipStreamSynchronize(st.ptr) == 0
            for i, dy in enumerate(dys):
                Y = dy.download().reshape(k, n)
                for j in range(k):
                    assert_exact(Y[j], c.Y[j], f"{name} replay {rep} multiply {i} column {j}")
    finally:
        hip.hipGraphExecDestroy(exe)
        hip.hipGraphDestroy(graph)


def test_full_size_symmetric_pairs_k4(E, O, gpu):
    """The audikw_1-like matrix, symmetric pair storage built for k = 4 (lds_doubles = 5120): every column of one k = 4 pass
    within 1e-12 of the CPU product, relative to sum_j |a_ij x_j|."""
    cfg = E.make_config(lds_doubles=LDS_MAX // 4, sym_pairs=1)
    c = Case(E, O, "fem3d", (943695, 3, 68, 68, 13500, 1, 1), cfg)
    plan = E.Plan(c.m, cfg)
    assert plan.stats["sym_pairs"] > 0.35 * c.nnz and plan.spmm_max_k == 4
    rng = np.random.default_rng(17)
    xs = [c.x] + [rng.uniform(-1, 1, c.n) for _ in range(3)]
    X = np.stack([E.vector_reorder(x, c.perm) for x in xs])
    for walk in (0, 1):
        Y = spmm(E, plan, X, walk=walk)
        for j, x in enumerate(xs):
            y_ref = c.y_ref if j == 0 else O.spmv_coo(c.n, c.m.I, c.m.J, c.m.V, X[j])
            scale = c.scale if j == 0 else O.abs_rowsum(c.n, c.m.I, c.m.J, c.m.V, X[j])
            y = c.recover(Y[j]) if j == 0 else Y[j]
            bad, worst = O.check_strict(y, y_ref, scale)
            assert bad == 0, f"walk={walk} column {j}: {bad} rows, worst {worst:.3e}"
