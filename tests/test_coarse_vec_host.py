"""The host side of the coarse space from near-null-space vectors (ehyb_coarse_create_host_vecs in coarse.cpp; no GPU): the
local bases against numpy's QR and the restatement of coarse_vec_cases.py, the rank cut as integer conditions, E and E^-1
against scipy and numpy, the same bits on 1 and 4 OpenMP threads, what a plain object of the same space computes, the errors,
and whether the vectors are worth having: on a 3-D spring network the restated PCG with the six rigid-body modes must need at
most two thirds of the iterations it needs with the three translations, and on the nearly singular grid [1, x, y] must beat the
constant."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest
import scipy.sparse as sp

import coarse_cases as kc
import coarse_vec_cases as vc

ERR_ARG = 1
RTOL = 1e-10


class Net:
    """a reordered matrix, near-null-space vectors B (nv, n) in the permuted numbering, b, the Jacobi diagonal"""

    def __init__(self, E, A, B_original, lds_doubles=2048):
        self.cfg = E.make_config(lds_doubles=lds_doubles, sym_pairs=0)
        self.m = E.Matrix.from_csr(A.indptr, A.indices, A.data, self.cfg, symmetric=True)
        self.m.reorder(self.cfg)
        self.A, self.n = self.m.to_scipy(), self.m.n
        self.B = np.stack([E.vector_reorder(v, self.m.reorder_list) for v in B_original])
        self.b = np.random.default_rng(3).uniform(-1, 1, self.n)
        self.dinv = 1.0 / self.A.diagonal()

    def restated(self, co, **kw):
        """iterations of the restated PCG with the library's agg, off, W and E^-1"""
        P = vc.prolongation(co.array("map"), co.array("off"), co.array("W"))
        x, it = vc.pcg(self.A, self.b, P, self.dinv, max_iter=5000, rtol=RTOL, einv=co.array("Einv"), **kw)
        assert np.linalg.norm(self.A @ x - self.b) <= 2 * RTOL * np.linalg.norm(self.b)
        return it


@pytest.fixture(scope="module")
def net(E):
    """the spring network of the issue: 16 x 12 x 10 nodes, shift 1e-3, with the six rigid-body modes"""
    K, coords = vc.spring_network(16, 12, 10, 1e-3, seed=1)
    modes = E.rigid_body_modes(coords, 3)
    assert modes.shape == (6, K.shape[0]) and np.abs((K - 1e-3 * sp.identity(K.shape[0])) @ modes.T).max() < 1e-12
    return Net(E, K, modes)


@pytest.fixture(scope="module")
def grid(E):
    """near_singular_grid(120, 100, 1, 0.0005) with [1, x, y]"""
    nx, ny = 120, 100
    i = np.arange(nx * ny)
    return Net(E, kc.near_singular_grid(nx, ny, 1, 0.0005), np.stack([np.ones(nx * ny), (i % nx).astype(float), (i // nx).astype(float)]))


@pytest.fixture(scope="module")
def small(E):
    """an 8 x 8 grid with aggregates of 1, 2, 18 and 43 rows and generic coordinates"""
    s = Net(E, kc.near_singular_grid(8, 8, 1, 0.5), np.ones((1, 64)), lds_doubles=1024)
    s.agg = np.repeat(np.arange(4, dtype=np.int32), [1, 2, 18, 43])
    rng = np.random.default_rng(8)
    s.x, s.y = rng.uniform(0, 8, 64), rng.uniform(0, 8, 64)
    return s


def test_rigid_body_modes(E):
    coords = np.random.default_rng(0).uniform(-1, 1, (5, 3))
    m3 = E.rigid_body_modes(coords, 3)
    assert m3.shape == (6, 15)
    for c in range(3):
        assert np.array_equal(m3[c].reshape(5, 3), np.eye(3)[c] * np.ones((5, 1)))
    axes = np.eye(3)
    for k in range(3):                      # omega x (x, y, z), omega the k-th axis
        assert np.array_equal(m3[3 + k].reshape(5, 3), np.cross(axes[k], coords))
    m2 = E.rigid_body_modes(coords[:, :2], 2)
    assert m2.shape == (3, 10) and np.array_equal(m2[2].reshape(5, 2), np.stack([-coords[:, 1], coords[:, 0]], axis=1))
    assert np.array_equal(m2[:2].reshape(2, 5, 2), np.eye(2)[:, None, :] * np.ones((1, 5, 1)))
    assert np.array_equal(E.rigid_body_modes(coords, 1), np.ones((1, 5)))


# ------------------------------------------------------------------ the local basis
def test_local_basis_against_qr(E, net):
    """Per aggregate the kept columns are orthonormal and span what numpy's QR of the restricted block spans, compared as
    projectors Q Q^T.  The margin is 4x what the restatement of coarse_vec_cases.py itself shows against np.linalg.qr on the
    same blocks.  Measured on the 46 aggregates of agg_rows = 128 (all of them keep six columns): max |Q^T Q - I| 1.3e-15 for the
    restatement and 1.3e-15 for the library; max |Q Q^T - QR's| 1.9e-15 for the restatement and 1.9e-15 for the library."""
    co = E.Coarse.from_vectors(net.m, net.B, agg_rows=128, upload=False)
    agg, off, W = co.array("map"), co.array("off"), co.array("W")
    off_r, W_r = vc.build_P(net.B, agg, co.nagg)
    assert np.array_equal(off, off_r) and (np.diff(off) == 6).all() and co.nc == 6 * co.nagg and W.shape == (6, net.n)
    assert np.array_equal(co.array("row_ptr"), kc.transpose(agg, co.nagg)[0]) and np.array_equal(co.array("rows"), kc.transpose(agg, co.nagg)[1])
    dev = {"library": [0.0, 0.0], "restatement": [0.0, 0.0]}
    for a in range(co.nagg):
        rows = np.flatnonzero(agg == a)
        Q = np.linalg.qr(net.B[:, rows].T)[0]
        for name, w in (("library", W), ("restatement", W_r)):
            q = w[:, rows].T
            dev[name][0] = max(dev[name][0], np.abs(q.T @ q - np.eye(6)).max())
            dev[name][1] = max(dev[name][1], np.abs(q @ q.T - Q @ Q.T).max())
    print(f"{co.nagg} aggregates: max |Q^T Q - I| and max |Q Q^T - QR's|: {dev}")
    assert dev["library"][0] <= 4 * dev["restatement"][0] and dev["library"][1] <= 4 * dev["restatement"][1]


def kept(co):
    return np.diff(co.array("off")).tolist()


def test_rank_cut(E, small):
    """integer conditions: which columns an aggregate keeps"""
    s = small
    one, zero = np.ones(s.n), np.zeros(s.n)

    def build(B):
        co = E.Coarse.from_vectors(s.m, np.stack(B), agg=s.agg, upload=False)
        off_r, W_r = vc.build_P(np.stack(B), s.agg, 4)
        assert np.array_equal(co.array("off"), off_r) and co.nc == off_r[-1] and co.nagg == 4
        W = co.array("W")
        assert ((W != 0) == (W_r != 0)).all() and np.abs(W - W_r).max() < 1e-12
        assert not W[np.arange(len(B))[:, None] >= np.diff(off_r)[s.agg][None, :]].any(), "a dropped column is not zero"
        return co

    assert kept(build([one, s.x, s.y])) == [1, 2, 3, 3]            # one row keeps one column, two rows two
    assert kept(build([one, s.x, one, s.y])) == [1, 2, 3, 3]       # a duplicated column is dropped
    assert kept(build([one, 2 * one + 3 * s.x, s.x])) == [1, 2, 2, 2]     # a combination of the columns before it
    assert kept(build([zero, one, s.x])) == [1, 2, 2, 2]           # a zero column is dropped
    gone = s.agg == 3
    co = build([np.where(gone, 0, one), np.where(gone, 0, s.x), np.where(gone, 0, s.y)])
    assert kept(co) == [1, 2, 3, 0] and co.nc == 6 and co.array("E").shape == (6, 6)      # an aggregate may keep none
    assert not co.array("W")[:, gone].any()
    gone = s.agg == 0                                                # the first one too: off starts 0, 0
    assert kept(build([np.where(gone, 0, one), s.x * ~gone])) == [0, 2, 2, 2]


# ------------------------------------------------------------------ E and its inverse
@pytest.mark.parametrize("name,agg_rows,nv", [("net", 64, 6), ("net", 256, 3), ("grid", 128, 3)])
def test_coarse_matrix_and_its_inverse(E, net, grid, name, agg_rows, nv):
    """the margins of test_coarse_host.test_coarse_matrix_and_its_inverse"""
    s = {"net": net, "grid": grid}[name]
    co = E.Coarse.from_vectors(s.m, s.B[:nv], agg_rows=agg_rows, upload=False)
    nc = co.nc
    Em, Einv = co.array("E"), co.array("Einv")
    assert Em.shape == (nc, nc) and Einv.shape == (nc, nc)
    assert np.array_equal(Em.view(np.int64), Em.T.view(np.int64)) and np.array_equal(Einv.view(np.int64), Einv.T.view(np.int64))
    P = vc.prolongation(co.array("map"), co.array("off"), co.array("W"))
    want = vc.coarse_matrix(s.A, P)
    scale = vc.coarse_matrix(abs(s.A), abs(P))                   # sum of |w_i a_ij w_j| of the block
    assert (np.abs(Em - want) <= 1e-13 * scale).all()
    ours = np.abs(Einv @ Em - np.eye(nc)).max()
    numpys = np.abs(np.linalg.inv(Em) @ Em - np.eye(nc)).max()
    print(f"{name} agg_rows={agg_rows} nv={nv}: nagg={co.nagg}, nc={nc}, cond(E)={np.linalg.cond(Em):.3e}, max|Einv E - I| = {ours:.3e}, "
          f"numpy.linalg.inv: {numpys:.3e}")
    assert ours <= 10 * numpys + nc * 2.0 ** -52


def test_the_same_bits_on_one_and_four_threads(E, net):
    omp = C.CDLL(ctypes.util.find_library("gomp") or "libgomp.so.1")
    before = omp.omp_get_max_threads()
    out = {}
    try:
        for threads in (1, 4):
            omp.omp_set_num_threads(threads)
            co = E.Coarse.from_vectors(net.m, net.B, agg_rows=64, upload=False)
            out[threads] = [co.array(k) for k in ("map", "row_ptr", "rows", "off", "W", "E", "Einv")]
    finally:
        omp.omp_set_num_threads(before)
    for a, b in zip(out[1], out[4]):
        kind = np.int64 if a.dtype == np.float64 else np.int32
        assert a.dtype == b.dtype and a.size and np.array_equal(a.view(kind), b.view(kind))


# ------------------------------------------------------------------ what a plain object of the same space computes
def test_one_constant_is_the_plain_object_scaled(E, net):
    """nv = 1, B = ones: P_vec = P_plain S with S = diag(1 / sqrt(rows per aggregate)), so E_vec = S E_plain S to rounding -- the
    margin of E itself: 1e-13 of the sum of the magnitudes of a block's terms"""
    plain = E.Coarse(net.m, agg_rows=128, upload=False)
    agg = plain.array("map")
    co = E.Coarse.from_vectors(net.m, np.ones((1, net.n)), agg=agg, upload=False)
    assert np.array_equal(co.array("map"), agg) and np.array_equal(co.array("off"), np.arange(plain.nc + 1)) and co.nc == plain.nc
    S = 1.0 / np.sqrt(np.bincount(agg))
    assert np.abs(co.array("W")[0] - S[agg]).max() <= 2.0 ** -52
    scale = S[:, None] * kc.coarse_matrix(abs(net.A), agg, plain.nc) * S[None, :]
    assert (np.abs(co.array("E") - S[:, None] * plain.array("E") * S[None, :]) <= 1e-13 * scale).all()
    for name in ("off", "W"):
        assert plain.array(name).size == 0


def test_the_translations_are_the_plain_dof_object(E, net):
    """B = the three translations on the aggregates of ehyb_coarse_map(m, a, 1) spans what the plain object of
    ehyb_coarse_map(m, a, 3) spans: the same apply, relative to ||z||, and the same solve to max(2, 5 %) iterations.  Both
    applies go through an inverse of their own E, each good to a few cond(E) 2^-52 (the object's E^-1 is tested to
    max|E^-1 E - I| <= 10 numpy's): the margin is 16 cond(E) 2^-52 ||z||."""
    a = 128
    ones = E.Coarse(net.m, agg_rows=a, dof=1, upload=False)
    agg, nagg = ones.array("map"), ones.nc
    plain = E.Coarse(net.m, agg_rows=a, dof=3, upload=False)
    co = E.Coarse.from_vectors(net.m, net.B[:3], agg_rows=a, upload=False)
    assert np.array_equal(co.array("map"), agg) and co.nc == plain.nc == 3 * nagg
    P = vc.prolongation(agg, co.array("off"), co.array("W"))
    cond = np.linalg.cond(plain.array("E"))
    r = np.random.default_rng(11).uniform(-1, 1, net.n)
    for dinv in (net.dinv, None):
        z = vc.apply(r, dinv, P, co.array("Einv"))
        want = kc.apply(r, dinv, plain.array("map"), plain.array("Einv"))
        err = np.linalg.norm(z - want) / np.linalg.norm(want)
        print(f"inv_diag {dinv is not None}: ||z_vec - z_plain|| / ||z|| = {err:.2e}, cond(E) = {cond:.2e}, margin {16 * cond * 2.0 ** -52:.2e}")
        assert err <= 16 * cond * 2.0 ** -52
    it_vec = net.restated(co)
    it_plain = kc.pcg(net.A, net.b, plain.array("map"), plain.nc, net.dinv, max_iter=5000, rtol=RTOL, einv=plain.array("Einv"))[1]
    print(f"{it_vec} iterations with the translations as vectors, {it_plain} with the plain dof = 3 object")
    assert abs(it_vec - it_plain) <= max(2, 0.05 * it_plain)


# ------------------------------------------------------------------ errors
def test_errors(E, small):
    lib = E.host._lib.load()
    s = small
    i32p, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    n = s.n
    agg = s.agg.copy()
    B = np.ascontiguousarray(np.stack([np.ones(n), s.x, s.y]))
    h = C.c_void_p()
    mp, ap, bp = C.byref(s.m.c), agg.ctypes.data_as(i32p), B.ctypes.data_as(dp)

    def call(m=mp, a=ap, nagg=4, b=bp, ldb=n, nv=3, out=C.byref(h)):
        rc = lib.ehyb_coarse_create_host_vecs(m, a, nagg, b, ldb, nv, out)
        return rc, lib.ehyb_last_error().decode()

    for kw in (dict(m=None), dict(a=None), dict(b=None), dict(out=None)):
        rc, msg = call(**kw)
        assert rc == ERR_ARG and "null" in msg, (kw, msg)
    for nv in (0, -1, vc.MAX_VECS + 1):
        rc, msg = call(nv=nv)
        assert rc == ERR_ARG and f"{nv} vectors" in msg and "1 .. 8" in msg, msg
    rc, msg = call(ldb=n - 1)
    assert rc == ERR_ARG and "ldb" in msg and str(n - 1) in msg, msg
    for bad in (4, -1):
        agg[17] = bad
        rc, msg = call()
        assert rc == ERR_ARG and f"agg[17] = {bad}" in msg, msg
    agg[:] = s.agg
    rc, msg = call(nagg=5)
    assert rc == ERR_ARG and "aggregate 4 holds no row" in msg, msg
    rc, msg = call(nagg=0)
    assert rc == ERR_ARG and "aggregates" in msg, msg
    for bad in (np.nan, np.inf):
        B[2, 40] = bad
        rc, msg = call()
        assert rc == ERR_ARG and "row 40" in msg and "column 2" in msg, msg
    B[2, 40] = s.y[40]
    zeros = np.zeros((2, n))
    rc, msg = call(b=zeros.ctypes.data_as(dp), nv=2)
    assert rc == ERR_ARG and "0 coarse unknowns" in msg, msg
    # nc > EHYB_COARSE_MAX: 64 aggregates of one row keep one column each -- use 2,049 rows of another matrix
    big = E.Matrix.generate("stencil2d", 50, 41, 5, 0, 1)
    ident = np.arange(big.n, dtype=np.int32)
    ones = np.ones(big.n)
    assert big.n == 2050
    rc = lib.ehyb_coarse_create_host_vecs(C.byref(big.c), ident.ctypes.data_as(i32p), big.n, ones.ctypes.data_as(dp), big.n, 1, C.byref(h))
    msg = lib.ehyb_last_error().decode()
    assert rc == ERR_ARG and "2050 coarse unknowns" in msg and "more than 2048" in msg and "fewer aggregates or vectors" in msg, msg
    assert not h.value
    # not positive definite: minus the matrix
    neg = Net(E, -kc.near_singular_grid(8, 8, 1, 0.5), np.ones((1, 64)), lds_doubles=1024)
    with pytest.raises(E.EhybError) as ei:
        E.Coarse.from_vectors(neg.m, neg.B, agg=s.agg, upload=False)
    assert ei.value.code == ERR_ARG and "not positive definite" in str(ei.value)
    # the raw constructor
    einv = np.eye(6)
    W = np.ones((3, n))
    off = np.array([0, 1, 3, 6, 6], dtype=np.int32)

    def raw(o=off, nv=3, ldw=n, nagg=4):
        rc = lib.ehyb_coarse_create_raw_vecs(n, ap, nagg, o.ctypes.data_as(i32p), W.ctypes.data_as(dp), ldw, nv, einv.ctypes.data_as(dp), C.byref(h))
        return rc, lib.ehyb_last_error().decode()

    assert raw(ldw=n - 1)[0] == ERR_ARG and raw(nv=9)[0] == ERR_ARG
    rc, msg = raw(o=np.array([0, 1, 5, 6, 6], dtype=np.int32))
    assert rc == ERR_ARG and "aggregate 1 keeps 4 columns" in msg, msg
    rc, msg = raw(o=np.array([0, 1, 0, 6, 6], dtype=np.int32))
    assert rc == ERR_ARG and "aggregate 1 keeps -1 columns" in msg, msg
    assert raw(o=np.array([1, 1, 3, 6, 6], dtype=np.int32))[0] == ERR_ARG and raw(o=np.zeros(5, dtype=np.int32))[0] == ERR_ARG
    assert not h.value
    co = E.Coarse.raw_vectors(n, agg, off, W, einv, upload=False)
    assert np.array_equal(co.array("off"), off) and np.array_equal(co.array("W"), W) and co.array("E").size == 0 and co.nc == 6
    # a vector object that was never uploaded is refused like a plain one
    p = C.c_void_p(0x10000)             # never read
    assert lib.ehyb_coarse_apply(co.h, None, p, p, None) == 8 and b"not uploaded" in lib.ehyb_last_error()
    assert lib.ehyb_coarse_restrict_step(co.h, p, p, None) == 8 and lib.ehyb_coarse_prolong_step(co.h, p, None, p, p, None, -1, None) == 8


def test_the_default_aggregates_leave_room(E, net):
    """agg_rows = 0: max(128, ceil(n nv / 1536)) rows, the rule of ehyb_coarse_map for dof"""
    auto = E.Coarse.from_vectors(net.m, net.B, upload=False)
    explicit = E.Coarse.from_vectors(net.m, net.B, agg_rows=kc.default_agg_rows(net.n, 6), upload=False)
    assert kc.default_agg_rows(net.n, 6) == 128 and np.array_equal(auto.array("map"), explicit.array("map")) and auto.nc <= kc.COARSE_MAX
    assert kc.default_agg_rows(943695, 6) == 3687


# ------------------------------------------------------------------ worth it?
def test_the_rotations_take_a_third_off_the_spring_network(E, net):
    """16 x 12 x 10 nodes, shift 1e-3, lds_doubles = 2048, b uniform in [-1, 1], rtol 1e-10, the library's aggregates for
    agg_rows = 64 and 128: the restated PCG with the six rigid-body modes needs at most two thirds of the iterations it needs
    with the three translations.  A prototype on box aggregates gave factors of 2.3 to 2.8; the factor 1.5 is a condition on
    the feature with room for the aggregates' shape, not a measurement."""
    for agg_rows in (64, 128):
        rbm = E.Coarse.from_vectors(net.m, net.B, agg_rows=agg_rows, upload=False)
        tr = E.Coarse.from_vectors(net.m, net.B[:3], agg_rows=agg_rows, upload=False)
        it_rbm, it_tr = net.restated(rbm), net.restated(tr)
        print(f"agg_rows={agg_rows}: {rbm.nagg} aggregates; six modes nc={rbm.nc}, {it_rbm} iterations; translations nc={tr.nc}, {it_tr} iterations")
        assert 3 * it_rbm <= 2 * it_tr, (agg_rows, it_rbm, it_tr)


def test_linear_functions_beat_the_constant_on_the_grid(E, grid):
    """near_singular_grid(120, 100, 1, 0.0005), agg_rows = 128: [1, x, y] against the constant (a prototype on 12 x 10 box
    aggregates: 81 against 131)"""
    vec = E.Coarse.from_vectors(grid.m, grid.B, agg_rows=128, upload=False)
    const = E.Coarse.from_vectors(grid.m, grid.B[:1], agg_rows=128, upload=False)
    it_vec, it_const = grid.restated(vec), grid.restated(const)
    print(f"{vec.nagg} aggregates: [1, x, y] nc={vec.nc}, {it_vec} iterations; the constant nc={const.nc}, {it_const} iterations")
    assert vec.nc == 3 * const.nc and it_vec < it_const
