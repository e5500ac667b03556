"""ehyb_lobpcg_gen on the host: ehyb_matrix_reorder_like against scipy's M[p][:, p], the numpy restatement
lobpcg_gen_cases.cpu_lobpcg_gen against scipy.linalg.eigh(K, M), and every argument check of ehyb_lobpcg_gen that needs no
device, in the order of the header."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import eigsh_cases as ec
import lobpcg_cases as lc
import lobpcg_gen_cases as lg

ERR_ARG, ERR_STATE = 1, 8
_dp = C.POINTER(C.c_double)


# ------------------------------------------------------------------ ehyb_matrix_reorder_like
def reordered(E, A, **kw):
    cfg = E.make_config(**kw)
    A = A.tocsr()
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=False)
    m.reorder(cfg)
    return m, cfg


def unsymmetric(n, seed):
    """a sparse matrix without symmetry of pattern or value, rows of unequal length, unsorted columns in a row, one empty row"""
    rng = np.random.default_rng(seed)
    M = sp.random(n, n, density=0.05, random_state=rng, format="lil")
    M[n // 2, :] = 0
    M = M.tocsr()
    M.eliminate_zeros()
    for i in range(n):                                            # stored order: columns falling
        a, b = M.indptr[i], M.indptr[i + 1]
        M.indices[a:b], M.data[a:b] = M.indices[a:b][::-1].copy(), M.data[a:b][::-1].copy()
    return M


@pytest.mark.parametrize("what", ["symmetric", "unsymmetric"])
def test_reorder_like_is_the_symmetric_permutation(E, what):
    """new = reorder_list[old]: entry (i, j) of M sits at (list[i], list[j]) -- the direction of vector_reorder, so that
    (M_new)(reorder x) = reorder (M x); rows grouped, columns of a row rising; the partition fields are K's"""
    K = ec.sym_grid(30, 20, 5)
    n = K.shape[0]
    M = lg.mass_grid(30, 20, 5)[0] if what == "symmetric" else unsymmetric(n, 3)
    k, cfg = reordered(E, K, window_mode=2, lds_doubles=512, sym_pairs=0)
    lst = k.reorder_list.copy()
    assert not np.array_equal(lst, np.arange(n)) and k.c.nParts > 1, "the case must permute"
    m = E.Matrix.from_csr(M.indptr, M.indices, M.data, cfg, symmetric=False)
    assert m.reorder_like(k) is m
    old_of = np.empty(n, dtype=np.int64)
    old_of[lst] = np.arange(n)
    want = sp.csr_matrix(M)[old_of][:, old_of].tocsr()            # row t of the new matrix is old row old_of[t]
    want.sort_indices()
    assert m.n == n and m.nnz == M.nnz
    assert np.array_equal(m.row_idx, want.indptr) and np.array_equal(m.J, want.indices)
    assert np.array_equal(m.V.view(np.int64), want.data.view(np.int64)), "entry for entry"
    assert np.array_equal(m.I, np.repeat(np.arange(n), np.diff(want.indptr)))
    assert np.array_equal(m.num_in_row, np.diff(want.indptr)) and m.c.maxCol == np.diff(want.indptr).max()
    wrong = sp.csr_matrix(M)[lst][:, lst].tocsr()
    assert (abs(wrong - want)).sum() > 0, "the other direction is another matrix: the test tells them apart"
    # the statement for vectors
    x = np.random.default_rng(1).standard_normal(n)
    assert np.allclose(m.to_scipy() @ E.vector_reorder(x, lst), E.vector_reorder(M @ x, lst), rtol=0, atol=1e-13)
    # the partition fields
    assert m.c.nParts == k.c.nParts and m.c.vectorCacheSize == k.c.vectorCacheSize and m.c.kernelPerPart == k.c.kernelPerPart
    assert np.array_equal(m.part_boundary, k.part_boundary) and np.array_equal(m.reorder_list, lst)
    assert C.addressof(m.c.partBoundary.contents) != C.addressof(k.c.partBoundary.contents), "copies, not k's arrays"
    pb, cache = k.part_boundary, int(k.c.vectorCacheSize)
    start = np.repeat(pb[:-1], np.diff(pb))
    inside = (want.indices >= np.repeat(start, np.diff(want.indptr))) & (want.indices < np.repeat(start, np.diff(want.indptr)) + cache)
    assert np.array_equal(m.num_in_row2, np.add.reduceat(np.append(inside, False), want.indptr[:-1]) * (np.diff(want.indptr) > 0))


def test_a_plan_builds_on_the_reordered_mass_and_multiplies_by_it(E, O):
    """Plan(..., upload=False) on the partitions of K; the layout walked as the kernels index it (oracle.walk_plan, as
    test_layout.py) writes every row once and gives M_new x"""
    K, (M, _) = ec.sym_grid(30, 20, 5), lg.mass_grid(30, 20, 5)
    k, cfg = reordered(E, K, window_mode=2, lds_doubles=512, sym_pairs=0)
    m = E.Matrix.from_csr(M.indptr, M.indices, M.data, cfg, symmetric=False).reorder_like(k)
    plan = E.Plan(m, E.make_config(window_mode=2, lds_doubles=512, sym_pairs=2), upload=False)
    assert np.array_equal(plan.array("part_boundary"), k.part_boundary)
    x = np.random.default_rng(2).standard_normal(m.n)
    y, written = O.walk_plan(plan, x)
    assert (written == 1).all()
    want = m.to_scipy() @ x
    assert np.abs(y - want).max() <= 1e-13 * np.abs(want).max()


def test_reorder_like_refusals(E):
    lib = E.host._lib.load()
    K, (M, _) = ec.sym_grid(8, 6, 2), lg.mass_grid(8, 6, 2)
    k, cfg = reordered(E, K, direct=1, sym_pairs=0)
    fresh = lambda A: E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=False)   # noqa: E731
    m = fresh(M)
    before = m.to_scipy()
    assert lib.ehyb_matrix_reorder_like(None, C.byref(k.c)) == ERR_ARG and b"null" in lib.ehyb_last_error()
    assert lib.ehyb_matrix_reorder_like(C.byref(m.c), None) == ERR_ARG and b"null" in lib.ehyb_last_error()
    other = fresh(lg.mass_grid(8, 5, 2)[0])
    with pytest.raises(E.EhybError) as ei:
        other.reorder_like(k)
    assert ei.value.code == ERR_ARG and "40 rows" in str(ei.value)
    never = fresh(K)                                               # not reordered: no partition data
    with pytest.raises(E.EhybError) as ei:
        m.reorder_like(never)
    assert ei.value.code == ERR_ARG and "partition data" in str(ei.value)
    assert (m.to_scipy() != before).nnz == 0, "a refused call leaves the matrix as it was"
    m.reorder_like(k)


# ------------------------------------------------------------------ the yardstick itself
def pencil_grid(nx, ny, seed):
    K = ec.sym_grid(nx, ny, seed)
    M, lumped = lg.mass_grid(nx, ny, seed)
    return K, M, lumped


def test_mass_grid_is_spd_and_its_lumped_form_the_row_sums():
    M, lumped = lg.mass_grid(8, 6, 2)
    d, off = M.diagonal(), np.asarray(abs(M).sum(axis=1)).ravel() - M.diagonal()
    assert (abs(M - M.T)).sum() == 0 and (d > 2 * off - 1e-15).all() and (off > 0).all() and (M.data > 0).all()
    assert np.linalg.eigvalsh(M.toarray()).min() > 0 and np.array_equal(lumped, np.asarray(M.sum(axis=1)).ravel())
    assert M.nnz == 48 + 2 * (7 * 6 + 8 * 5)


@pytest.mark.parametrize("lumped", [False, True], ids=["consistent", "lumped"])
@pytest.mark.parametrize("grid,nev,block", [((8, 6, 2), 3, 0), ((8, 6, 2), 1, 0), ((30, 20, 5), 4, 6)])
def test_cpu_lobpcg_gen_against_scipy_eigh(grid, nev, block, lumped):
    """the restatement: converged, and the true residual, the eigenvalue error and M-orthonormality within the bounds the device
    tests use"""
    K, Mc, Ml = pencil_grid(*grid)
    M, tol = (Ml if lumped else Mc), 1e-10
    lam = sla.eigh(K.toarray(), lg.mass_dense(M), eigvals_only=True)
    ev, X, info = lg.cpu_lobpcg_gen(K, M, nev, block=block, tol=tol)
    Md = lg.mass_dense(M)
    nrm = np.abs(ev).max()
    assert info["status"] == "ok" and info["nconv"] == nev and 0 < info["iters"] < 200, info
    assert np.abs(ev - lam[:nev]).max() <= 10 * tol * nrm
    assert max(np.linalg.norm(K @ X[i] - ev[i] * (Md @ X[i])) for i in range(nev)) <= 10 * tol * nrm
    assert np.abs(X @ Md @ X.T - np.eye(nev)).max() <= 1e-12 and info["orth"] <= 1e-12
    assert info["mass_multiplies"] == (0 if lumped else info["multiplies"])


def test_cpu_lobpcg_gen_with_the_identity_is_cpu_lobpcg():
    K = ec.sym_grid(8, 6, 2)
    a, b = lc.cpu_lobpcg(K, 3, tol=1e-10), lg.cpu_lobpcg_gen(K, np.ones(48), 3, tol=1e-10, bnorm=1.0)
    # (not the same bits: numpy forms S S^T of one array with another BLAS routine than S BS^T of two)
    assert a[2]["iters"] == b[2]["iters"] and a[2]["multiplies"] == b[2]["multiplies"]
    assert np.abs(a[0] - b[0]).max() <= 1e-12 * np.abs(a[0]).max()


def test_cpu_lobpcg_gen_bnorm_breakdown_and_max_iter():
    K, Mc, Ml = pencil_grid(8, 6, 2)
    bad = Ml.copy()
    bad[5] = -bad[5] * 40
    assert lg.cpu_lobpcg_gen(K, bad, 3, X0=np.eye(48)[[5, 6, 7]])[2]["status"] == "breakdown", "a negative G_ii"
    info = lg.cpu_lobpcg_gen(K, Mc, 3, max_iter=0)[2]
    assert info["status"] == "ok" and info["iters"] == 0 and info["multiplies"] == 3 == info["mass_multiplies"] and info["nconv"] < 3
    loose = lg.cpu_lobpcg_gen(K, Mc, 3, tol=1e-10, bnorm=1e4)[2]["iters"]
    assert loose < lg.cpu_lobpcg_gen(K, Mc, 3, tol=1e-10)[2]["iters"], "a larger scale of M loosens the test of convergence"


# ------------------------------------------------------------------ the argument checks of the solver and their order
FEM_SMALL = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))
X, D0, V0, MD = 0x10000, 0x20000, 0x30000, 0x40000            # never read: every call fails before device work


def host_plan(E, half=False, gen=FEM_SMALL, **kw):
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
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
def smaller(E):
    return host_plan(E, gen=("fem3d", (6000, 3, 12, 12, 20000, 1, 5)), direct=2)


@pytest.fixture(scope="module")
def other_coarse(E):
    return E.Coarse.raw(10, np.arange(10) // 5, np.eye(2), upload=False)


def call(lib, plan, mass_plan=None, mdiag=MD, coarse=None, dinv=D0, x0=V0, ldx0=None, nev=4, block=0, max_iter=10, tol=1e-8, anorm=0.0,
         bnorm=0.0, evecs=X, ldv=None):
    n = plan.n if plan is not None else 0
    ldv = n + (n & 1) if ldv is None else ldv
    ldx0 = n + (n & 1) if ldx0 is None else ldx0
    ints = [C.c_int(-5) for _ in range(4)]
    ev, rs = np.full(8, -5.0), np.full(8, -5.0)
    rc = lib.ehyb_lobpcg_gen(plan.h if plan is not None else None, mass_plan.h if mass_plan is not None else None,
                             C.c_void_p(mdiag) if mdiag else None, coarse.h if coarse is not None else None, C.c_void_p(dinv) if dinv else None,
                             C.c_void_p(x0) if x0 else None, ldx0, nev, block, max_iter, tol, anorm, bnorm, ev.ctypes.data_as(_dp),
                             C.c_void_p(evecs) if evecs else None, ldv, None, *(C.byref(i) for i in ints), rs.ctypes.data_as(_dp))
    assert [i.value for i in ints] == [-5] * 4 and (ev == -5).all() and (rs == -5).all(), "an output was written before device work"
    return rc, lib.ehyb_last_error()


def test_never_uploaded_plans_are_state_errors_the_plan_first(E, plan):
    lib = E.host._lib.load()
    for kw in (dict(), dict(bnorm=3.0), dict(mass_plan=plan, mdiag=0), dict(nev=3, block=8), dict(max_iter=0)):
        rc, msg = call(lib, plan, **kw)
        assert rc == ERR_STATE and b"ehyb_lobpcg_gen: plan not uploaded" in msg, (kw, msg)


@pytest.mark.parametrize("bad,word", [(dict(nev=0), b"nev"), (dict(block=9), b"nev"), (dict(max_iter=-1), b"nev"), (dict(tol=-1e-9), b"tol"),
                                      (dict(anorm=-1.0), b"anorm"), (dict(bnorm=-1.0), b"bnorm"), (dict(bnorm=float("nan")), b"bnorm"),
                                      (dict(bnorm=float("inf")), b"bnorm"), (dict(mdiag=0), b"exactly one"), (dict(mdiag=MD + 8), b"mass_diag_dev"),
                                      (dict(ldv=1), b"ldv"), (dict(ldx0=30001), b"ldx0"), (dict(evecs=X + 8), b"aligned"),
                                      (dict(dinv=D0 + 8), b"aligned")])
def test_argument_errors(E, plan, bad, word):
    rc, msg = call(E.host._lib.load(), plan, **bad)
    assert rc == ERR_ARG and b"ehyb_lobpcg_gen" in msg and word in msg and b"upload" not in msg, (bad, msg)


def test_the_mass_choice_and_the_mass_plan(E, plan, part, smaller):
    lib = E.host._lib.load()
    rc, msg = call(lib, plan, mass_plan=plan)                      # both
    assert rc == ERR_ARG and b"exactly one" in msg, msg
    rc, msg = call(lib, plan, mass_plan=part, mdiag=0)
    assert rc == ERR_ARG and b"mass plan must cover all rows" in msg, msg
    rc, msg = call(lib, plan, mass_plan=smaller, mdiag=0)
    assert rc == ERR_ARG and b"mass plan must cover all rows" in msg and b"6000" in msg, msg
    assert call(lib, None, nev=0, mdiag=0)[1].find(b"null argument") >= 0


# in the order of the header; each entry: the fault, and a word of its message
STAGES = [(dict(nev=0), b"nev"), (dict(bnorm=-2.0), b"bnorm"), ("part", b"needs a plan over all rows"), (dict(mdiag=0), b"exactly one"),
          ("mass part", b"mass plan must cover"), (dict(ldv=3), b"ldv"), (dict(evecs=X + 8), b"aligned"), ("coarse", b"coarse object has 10 rows")]


def test_the_order_of_the_checks(E, plan, part, other_coarse):
    """all the faults from stage i on at once: stage i's message comes.  (Both "exactly one" and a bad mass plan cannot be had at
    once: from the mass-choice stage on, the later stages carry the mass plan alone.)  A misaligned mass_diag_dev comes before ldv."""
    lib = E.host._lib.load()
    for first in range(len(STAGES)):
        kw, p = {}, plan
        for fault, _ in STAGES[first:]:
            if fault == "part":
                p = part
            elif fault == "coarse":
                kw["coarse"] = other_coarse
            elif fault == "mass part":
                if first > 3:
                    kw.update(mass_plan=part, mdiag=0)
            else:
                kw.update(fault)
        if first <= 3:
            kw["mdiag"], kw["mass_plan"] = 0, None                 # neither: the mass-choice fault
        if "ldv" not in kw:
            kw["ldv"] = None
        rc, msg = call(lib, p, **kw)
        assert rc == ERR_ARG and STAGES[first][1] in msg, (first, kw, msg)
    rc, msg = call(lib, plan, mdiag=MD + 8, ldv=3)
    assert rc == ERR_ARG and b"mass_diag_dev" in msg, msg
    rc, msg = call(lib, part, mdiag=MD + 8)
    assert rc == ERR_ARG and b"all rows" in msg, msg
