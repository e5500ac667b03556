"""The host side of the two-level preconditioner (coarse.cpp; no GPU): the default map against the numpy restatement of
coarse_cases.py entry for entry, its invariants, E and E^-1 against scipy and numpy, the same bits on 1 and 8 OpenMP threads,
the errors, and whether the coarse space is worth having: on a nearly singular grid the restated PCG with the library's map
must need at most half of Jacobi's iterations."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

import cheb_cases as cc
import coarse_cases as kc

ERR_ARG, ERR_STATE = 1, 8
AGG_ROWS = (16, 64, 128, 10 ** 9)


class Input:
    """a reordered matrix, its CSR arrays and partitions"""

    def __init__(self, E, m, cfg):
        self.m = m
        m.reorder(cfg)
        self.A = m.to_scipy()
        self.pb = m.part_boundary.copy()
        self.perm = m.reorder_list.copy()
        self.n = m.n


def from_scipy(E, A, cfg):
    return E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=True)


@pytest.fixture(scope="module")
def inputs(E):
    cfg = E.make_config(lds_doubles=1024)
    fem = kc.spd_on_the_pattern(E.Matrix.generate("fem3d", 3000, 3, 10, 10, 13500, 1, 7, cfg=cfg).to_scipy(), 0.01)
    return {"grid": Input(E, from_scipy(E, kc.near_singular_grid(60, 50, 1, 0.0005), cfg), cfg),
            "fem3d": Input(E, from_scipy(E, fem, cfg), cfg),
            "rmat": Input(E, E.Matrix.generate("rmat", 10, 1 << 13, 1, cfg=cfg), cfg)}


CASES = [("grid", 1), ("fem3d", 1), ("fem3d", 3), ("rmat", 1)]


@pytest.fixture(scope="module")
def maps(E, inputs):
    """(input, dof, agg_rows) -> (the library's host object, the restatement's map and nc): computed once"""
    out = {}
    for name, dof in CASES:
        s = inputs[name]
        for agg_rows in AGG_ROWS:
            if name == "rmat":      # E of a graph's adjacency matrix need not be positive definite: the map alone
                cmap, nc = np.empty(s.n, dtype=np.int32), C.c_int(0)
                rc = E.host._lib.load().ehyb_coarse_map(C.byref(s.m.c), agg_rows, dof, cmap.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nc))
                assert rc == 0
                got = (cmap, nc.value, None)
            else:
                co = E.Coarse(s.m, agg_rows=agg_rows, dof=dof, upload=False)
                got = (co.array("map"), co.nc, co)
            out[name, dof, agg_rows] = got + kc.aggregate(s.A.indptr, s.A.indices, s.pb, agg_rows, dof, s.perm)
    return out


@pytest.mark.parametrize("name,dof", CASES)
def test_map_equals_the_restatement(inputs, maps, name, dof):
    assert len(inputs[name].pb) - 1 > 1, "more than one partition"
    for agg_rows in AGG_ROWS:
        cmap, nc, _, want, want_nc = maps[name, dof, agg_rows]
        print(f"{name} dof={dof} agg_rows={agg_rows}: n={len(cmap)}, {len(inputs[name].pb) - 1} partitions, nc={nc}")
        assert nc == want_nc and np.array_equal(cmap, want), (name, dof, agg_rows, nc, want_nc)


@pytest.mark.parametrize("name,dof", CASES)
def test_map_invariants(inputs, maps, name, dof):
    s = inputs[name]
    part_of_row = np.searchsorted(s.pb, np.arange(s.n), side="right") - 1
    for agg_rows in AGG_ROWS:
        cmap, nc, co, _, _ = maps[name, dof, agg_rows]
        assert cmap.shape == (s.n,) and cmap.min() == 0 and cmap.max() == nc - 1 and 1 <= nc <= kc.COARSE_MAX
        assert (np.bincount(cmap, minlength=nc) > 0).all(), "an empty unknown"
        for u_parts in (part_of_row[cmap == u] for u in range(nc)):
            assert (u_parts == u_parts[0]).all(), "an unknown across a partition boundary"
        if co is not None:
            row_ptr, rows = co.array("row_ptr"), co.array("rows")
            want_ptr, want_rows = kc.transpose(cmap, nc)
            assert np.array_equal(row_ptr, want_ptr) and np.array_equal(rows, want_rows)
            for u in range(nc):
                seg = rows[row_ptr[u]:row_ptr[u + 1]]
                assert (cmap[seg] == u).all() and (np.diff(seg) > 0).all()
        if agg_rows == 10 ** 9 and dof == 1:
            # growth takes a whole connected piece of a partition, and every piece with a neighbour merges: on a symmetric pattern
            # what is left is the pieces of the partitions' own graphs -- one per partition where the partitions are connected.
            # (The R-MAT's pattern is not symmetric: a piece that is only pointed AT by pieces already visited stays.)
            pieces = 0
            for p in range(len(s.pb) - 1):
                lo, hi = s.pb[p], s.pb[p + 1]
                pieces += csgraph.connected_components(s.A[lo:hi, lo:hi], directed=False)[0]
            symmetric = (s.A != 0).astype(np.int8)
            symmetric = (symmetric != symmetric.T).nnz == 0
            assert symmetric == (name != "rmat") and (nc == pieces if symmetric else nc >= pieces), (nc, pieces)
            if name == "grid":
                assert nc == len(s.pb) - 1, "a grid's partitions are connected"


def test_automatic_size(E, inputs):
    s = inputs["fem3d"]
    for dof in (1, 3):
        auto = E.Coarse(s.m, agg_rows=0, dof=dof, upload=False)
        explicit = E.Coarse(s.m, agg_rows=kc.default_agg_rows(s.n, dof), dof=dof, upload=False)
        assert kc.default_agg_rows(s.n, dof) == 128 and np.array_equal(auto.array("map"), explicit.array("map"))
    assert kc.default_agg_rows(943695, 1) == 615 and kc.default_agg_rows(943695, 3) == 1844


# ------------------------------------------------------------------ E and its inverse
@pytest.mark.parametrize("name,dof,agg_rows", [("grid", 1, 16), ("grid", 1, 128), ("fem3d", 3, 64), ("fem3d", 1, 10 ** 9)])
def test_coarse_matrix_and_its_inverse(inputs, maps, name, dof, agg_rows):
    s = inputs[name]
    cmap, nc, co, _, _ = maps[name, dof, agg_rows]
    Em, Einv = co.array("E"), co.array("Einv")
    assert Em.shape == (nc, nc) and Einv.shape == (nc, nc)
    assert np.array_equal(Em.view(np.int64), Em.T.view(np.int64)) and np.array_equal(Einv.view(np.int64), Einv.T.view(np.int64))
    want = kc.coarse_matrix(s.A, cmap, nc)
    scale = kc.coarse_matrix(abs(s.A), cmap, nc)             # sum of |a_ij| of the block
    assert (np.abs(Em - want) <= 1e-13 * scale).all()
    ours = np.abs(Einv @ Em - np.eye(nc)).max()
    numpys = np.abs(np.linalg.inv(Em) @ Em - np.eye(nc)).max()
    print(f"{name} dof={dof} agg_rows={agg_rows}: nc={nc}, cond(E)={np.linalg.cond(Em):.3e}, max|Einv E - I| = {ours:.3e}, numpy.linalg.inv: {numpys:.3e}")
    assert ours <= 10 * numpys + nc * 2.0 ** -52


def test_the_same_bits_on_one_and_eight_threads(E, inputs):
    """The host calls run on the calling thread's OpenMP setting: set through the OpenMP runtime the library is linked with."""
    omp = C.CDLL(ctypes.util.find_library("gomp") or "libgomp.so.1")
    before = omp.omp_get_max_threads()
    out = {}
    try:
        for threads in (1, 8):
            omp.omp_set_num_threads(threads)
            for name, dof, agg_rows in (("grid", 1, 16), ("fem3d", 3, 64)):
                co = E.Coarse(inputs[name].m, agg_rows=agg_rows, dof=dof, upload=False)
                out[threads, name] = (co.array("map"), co.array("E"), co.array("Einv"))
    finally:
        omp.omp_set_num_threads(before)
    for name in ("grid", "fem3d"):
        for a, b in zip(out[1, name], out[8, name]):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.int32),
                                                         b.view(np.int64 if b.dtype == np.float64 else np.int32)), name


# ------------------------------------------------------------------ errors
def test_errors(E, inputs):
    lib = E.host._lib.load()
    s = inputs["grid"]
    i32p = C.POINTER(C.c_int32)
    cmap, nc, h = np.zeros(s.n, dtype=np.int32), C.c_int(0), C.c_void_p()
    mp = C.byref(s.m.c)
    ptr = cmap.ctypes.data_as(i32p)
    # null arguments
    assert lib.ehyb_coarse_map(None, 64, 1, ptr, C.byref(nc)) == ERR_ARG and b"null" in lib.ehyb_last_error()
    assert lib.ehyb_coarse_map(mp, 64, 1, None, C.byref(nc)) == ERR_ARG
    assert lib.ehyb_coarse_map(mp, 64, 1, ptr, None) == ERR_ARG
    assert lib.ehyb_coarse_create_host(None, ptr, 1, C.byref(h)) == ERR_ARG
    assert lib.ehyb_coarse_create_host(mp, None, 1, C.byref(h)) == ERR_ARG
    assert lib.ehyb_coarse_create_host(mp, ptr, 1, None) == ERR_ARG
    assert lib.ehyb_coarse_upload(None) == ERR_ARG
    assert lib.ehyb_coarse_host_array(None, 0, C.byref(C.c_void_p()), C.byref(C.c_int64())) == ERR_ARG
    assert lib.ehyb_coarse_apply(None, None, None, None, None) == ERR_ARG
    lib.ehyb_coarse_destroy(None)
    # dof < 1, a matrix without partition data
    assert lib.ehyb_coarse_map(mp, 64, 0, ptr, C.byref(nc)) == ERR_ARG and b"dof" in lib.ehyb_last_error()
    fresh = E.Matrix.generate("stencil2d", 8, 8, 5, 0, 1)
    fresh.c.nParts = 0
    assert lib.ehyb_coarse_map(C.byref(fresh.c), 64, 1, ptr, C.byref(nc)) == ERR_ARG and b"partition" in lib.ehyb_last_error()
    # nc outside 1 .. 2048
    for bad in (0, -1, kc.COARSE_MAX + 1):
        assert lib.ehyb_coarse_create_host(mp, ptr, bad, C.byref(h)) == ERR_ARG and b"coarse unknowns" in lib.ehyb_last_error()
    # a map entry out of range, an empty unknown
    cmap[:] = np.arange(s.n) % 3
    cmap[17] = 3
    assert lib.ehyb_coarse_create_host(mp, ptr, 3, C.byref(h)) == ERR_ARG and b"map[17]" in lib.ehyb_last_error()
    cmap[17] = -1
    assert lib.ehyb_coarse_create_host(mp, ptr, 3, C.byref(h)) == ERR_ARG and b"map[17]" in lib.ehyb_last_error()
    cmap[:] = np.arange(s.n) % 3
    assert lib.ehyb_coarse_create_host(mp, ptr, 4, C.byref(h)) == ERR_ARG and b"unknown 3 holds no row" in lib.ehyb_last_error()
    assert not h.value
    # a default map that would exceed 2048: one row per aggregate; the message names an agg_rows
    assert lib.ehyb_coarse_map(mp, 1, 1, ptr, C.byref(nc)) == ERR_ARG
    msg = lib.ehyb_last_error().decode()
    assert "more than 2048" in msg and "agg_rows" in msg and "would fit" in msg, msg
    fits = int(msg.split("agg_rows")[-1].split()[0])
    assert lib.ehyb_coarse_map(mp, fits, 1, ptr, C.byref(nc)) == 0 and 1 <= nc.value <= kc.COARSE_MAX
    # host arrays: an unknown one
    co = E.Coarse(s.m, agg_rows=128, upload=False)
    assert lib.ehyb_coarse_host_array(co.h, 5, C.byref(C.c_void_p()), C.byref(C.c_int64())) == ERR_ARG


def test_an_indefinite_matrix_is_refused(E):
    """ehyb_gen_kkt3d (a saddle-point matrix) with its partitions as the map"""
    cfg = E.make_config(lds_doubles=1024)
    m = E.Matrix.generate("kkt3d", 6, cfg=cfg)
    m.reorder(cfg)
    pb = m.part_boundary
    cmap = (np.searchsorted(pb, np.arange(m.n), side="right") - 1).astype(np.int32)
    assert np.linalg.eigvalsh(m.to_scipy().toarray()).min() < 0
    with pytest.raises(E.EhybError) as ei:
        E.Coarse(m, map=cmap, upload=False)
    assert ei.value.code == ERR_ARG and "not positive definite" in str(ei.value)


def test_solver_argument_order(E, inputs):
    """what shows without a device: everything up to the uploads, which come last"""
    lib = E.host._lib.load()
    s = inputs["grid"]
    cfg = E.make_config(lds_doubles=1024)
    plan = E.Plan(s.m, cfg, upload=False)
    co = E.Coarse(s.m, agg_rows=128, upload=False)
    other = E.Coarse.raw(s.n - 1, np.zeros(s.n - 1, dtype=np.int32), np.ones((1, 1)), upload=False)
    p = C.c_void_p(0x10000)             # never read: every call fails before device work
    one = lambda plan_h, c_h, b=p, x=p, max_iter=10, rtol=1e-8: lib.ehyb_pcg_coarse(plan_h, c_h, None, b, x, max_iter, rtol, 10, None, None, None)  # noqa: E731
    multi = lambda plan_h, c_h, ldb=s.n, k=2, max_iter=10: lib.ehyb_pcg_coarse_multi(plan_h, c_h, None, p, ldb, p, s.n, k, max_iter, 1e-8, 10, None,  # noqa: E731
                                                                                      None, None)
    # 1. what ehyb_pcg rejects -- before the coarse object is looked at
    assert one(None, None) == ERR_ARG and b"null argument" in lib.ehyb_last_error()
    assert one(plan.h, None, b=None) == ERR_ARG and b"null argument" in lib.ehyb_last_error()
    assert one(plan.h, None, max_iter=-1) == ERR_ARG and b"max_iter" in lib.ehyb_last_error()
    assert one(plan.h, None, rtol=float("nan")) == ERR_ARG and b"rtol" in lib.ehyb_last_error()
    assert multi(plan.h, None, k=0) == ERR_ARG and b"right-hand sides" in lib.ehyb_last_error()
    assert multi(plan.h, None, ldb=s.n - 1) == ERR_ARG and b"ldb" in lib.ehyb_last_error()
    assert multi(plan.h, None, max_iter=-1) == ERR_ARG and b"max_iter" in lib.ehyb_last_error()
    # 2. the coarse object: null, another n -- before the plan's upload is looked at
    for call in (one, multi):
        assert call(plan.h, None) == ERR_ARG and b"null coarse object" in lib.ehyb_last_error()
        assert call(plan.h, other.h) == ERR_ARG and f"{s.n - 1} rows".encode() in lib.ehyb_last_error()
        # 3. the plan never uploaded (the coarse object neither: the plan comes first)
        assert call(plan.h, co.h) == ERR_STATE and b"plan not uploaded" in lib.ehyb_last_error()
    # the step calls and apply on an object never uploaded
    assert lib.ehyb_coarse_apply(co.h, None, p, p, None) == ERR_STATE
    assert lib.ehyb_coarse_restrict_step(co.h, p, p, None) == ERR_STATE
    assert lib.ehyb_coarse_solve_step(co.h, p, p, None) == ERR_STATE
    assert lib.ehyb_coarse_prolong_step(co.h, p, None, p, p, None, -1, None) == ERR_STATE
    assert lib.ehyb_coarse_prolong_step(co.h, p, None, p, p, None, 0, None) == ERR_ARG      # rz = 0 needs s
    assert lib.ehyb_coarse_prolong_step(co.h, p, None, p, p, p, 2, None) == ERR_ARG


# ------------------------------------------------------------------ worth it?
def test_the_coarse_space_halves_the_iterations_of_a_nearly_singular_grid(E):
    """near_singular_grid(120, 100, 1, 0.0005), lds_doubles = 2048, b uniform in [-1, 1] in the permuted numbering, rtol 1e-10:
    the restated PCG with the library's map for agg_rows = 128 needs at most half the iterations of Jacobi-PCG.  A prototype of
    the specification gave 187 against 674, and 131 with agg_rows = 64; the factor 2 is a condition on the aggregation, not a
    measurement of it."""
    cfg = E.make_config(lds_doubles=2048, sym_pairs=0)
    m = from_scipy(E, kc.near_singular_grid(120, 100, 1, 0.0005), cfg)
    m.reorder(cfg)
    A = m.to_scipy()
    b = np.random.default_rng(3).uniform(-1, 1, m.n)
    dinv = 1.0 / A.diagonal()
    it_jacobi = cc.jacobi_pcg(A, b, dinv, max_iter=5000, rtol=1e-10)
    its = {}
    for agg_rows in (128, 64):
        co = E.Coarse(m, agg_rows=agg_rows, upload=False)
        x, its[agg_rows] = kc.pcg(A, b, co.array("map"), co.nc, dinv, max_iter=5000, rtol=1e-10)
        assert np.linalg.norm(A @ x - b) <= 2e-10 * np.linalg.norm(b)
        print(f"agg_rows={agg_rows}: nc={co.nc} over {len(m.part_boundary) - 1} partitions, {its[agg_rows]} iterations; Jacobi-PCG {it_jacobi}")
    assert 2 * its[128] <= it_jacobi, (its, it_jacobi)
