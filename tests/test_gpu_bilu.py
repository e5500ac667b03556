"""ehyb_gmres_bilu, ehyb_bicgstab_bilu and ehyb_bicgstab_bilu_multi on the device: GMRES and BiCGSTAB right-preconditioned with the
block ILU(0) of ehyb_bilu, on the convection-diffusion systems and the five plan shapes of test_gpu_gmres.py.

bilu_cases.py restates both solvers step for step around the library's own factors; the device must agree with it to the few steps
the Jacobi solvers' tests allow (5), reach the true residual, and agree with scipy's direct solve -- and on the first shape need
at most half of the steps the device's own Jacobi solvers need.  With plain storage the device decides everything, so x, the count
and the relative residual are the same bits from run to run, for graphs and plain launches, on a given and a private stream, for
every check_every, and column j of a k-column solve equals the single solve of b_j.  Everything runs in the permuted numbering."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import bilu_cases as lc
from test_gpu_gmres import SHAPES, System, cd_matrix, panel_matrix, rhs

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 8
RTOL = 1e-10
ORDERS = ("stored", "colour")
PLAIN = dict(window_mode=2, lds_doubles=2048, sym_pairs=0)


class BiluSystem(System):
    """System in the permuted numbering: A as the reordered matrix holds it, b, and the Bilu objects by (order, block_rows)"""

    def __init__(self, E, A, **kw):
        super().__init__(E, A, **kw)
        self.E = E
        self.Ap = self.m.to_scipy()
        self.b = E.vector_reorder(rhs(self.n), self.perm)
        self.factors = {}

    def bilu(self, order="stored", block_rows=0):
        if (order, block_rows) not in self.factors:
            self.factors[order, block_rows] = self.E.Bilu(self.m, block_rows=block_rows, order=order)
        return self.factors[order, block_rows]

    def solver(self, order="stored", block_rows=0):
        return lc.Solver(lc.from_library(self.bilu(order, block_rows)))


@pytest.fixture(scope="module")
def main(E):
    """the first shape of test_gpu_gmres.py with plain storage"""
    return BiluSystem(E, cd_matrix(120, 100, 3000, 1), **PLAIN)


def same_bits(got, want, what):
    x, it, rel = got
    xw, itw, relw = want
    assert np.array_equal(np.atleast_1d(it), np.atleast_1d(itw)), (what, it, itw)
    assert np.array_equal(np.atleast_1d(rel), np.atleast_1d(relw), equal_nan=True), (what, rel, relw)
    assert np.array_equal(x.view(np.int64), xw.view(np.int64)), (what, np.abs(x - xw).max())


# ------------------------------------------------------------------ the plan shapes
@pytest.mark.parametrize("name,make,taken", SHAPES, ids=[s[0] for s in SHAPES])
def test_plan_shapes_against_the_restatement_and_scipy(E, gpu, name, make, taken):
    """Measured counts, the device's and the restatement's alike: halo-window GMRES(30) 89, GMRES(20) 92, BiCGSTAB 44 against the
    device's own Jacobi 428 and 191 (12 blocks, 64 levels); reference window 97 / 99 / 49; direct 86 / 86 / 44; panel residual
    11 / 11 / 6; symmetric pairs 30 / 30 / 16."""
    A, kw = make(E)
    if A is None:
        A = panel_matrix(E, E.make_config(**kw))
    s = BiluSystem(E, A, **kw)
    assert taken(s.plan.stats), (name, s.plan.stats)
    f, solve = s.bilu(), s.solver()
    assert f.fallback_blocks == 0
    x_ref = spla.spsolve(s.Ap.tocsc(), s.b)
    bnorm, xnorm = np.linalg.norm(s.b), np.linalg.norm(x_ref)
    counts = {}
    for restart in (30, 20):
        x, it, rel = s.plan.gmres_bilu(s.b, f, restart=restart, max_iter=2000, rtol=RTOL)
        _, it_cpu, rel_cpu, status = lc.gmres(s.Ap, s.b, solve, restart=restart, max_iter=2000, rtol=RTOL)
        print(name, f"GMRES({restart})", "device", it, rel, "restated", it_cpu, rel_cpu, status)
        assert 0 < it and rel <= RTOL, (name, restart, it, rel)
        assert np.linalg.norm(s.b - s.Ap @ x) <= 10 * RTOL * bnorm, (name, restart)
        assert status == "converged" and abs(it - it_cpu) <= 5, (name, restart, it, it_cpu, rel, rel_cpu)
        assert np.linalg.norm(x - x_ref) <= 1e-6 * xnorm, (name, restart, np.linalg.norm(x - x_ref))
        counts[restart] = it
    x, it, rel = s.plan.bicgstab_bilu(s.b, f, max_iter=2000, rtol=RTOL, check_every=1)
    _, it_cpu, rel_cpu, status = lc.bicgstab(s.Ap, s.b, solve, max_iter=2000, rtol=RTOL)
    print(name, "BiCGSTAB", "device", it, rel, "restated", it_cpu, rel_cpu, status)
    assert 0 < it and rel <= RTOL, (name, it, rel)
    assert np.linalg.norm(s.b - s.Ap @ x) <= 10 * RTOL * bnorm, name
    assert status == "converged" and abs(it - it_cpu) <= 5, (name, it, it_cpu, rel, rel_cpu)
    assert np.linalg.norm(x - x_ref) <= 1e-6 * xnorm, (name, np.linalg.norm(x - x_ref))
    if name == SHAPES[0][0]:
        _, g_jacobi, g_rel = s.plan.gmres(s.b, restart=30, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag)
        _, b_jacobi, b_rel = s.plan.bicgstab(s.b, max_iter=2000, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
        print(name, f"{f.blocks} blocks, {f.levels} levels; Jacobi on the device: GMRES(30)", g_jacobi, "BiCGSTAB", b_jacobi)
        assert g_rel <= RTOL and b_rel <= RTOL
        assert 2 * counts[30] <= g_jacobi and 2 * it <= b_jacobi, (counts, g_jacobi, it, b_jacobi)


@pytest.mark.parametrize("order", ORDERS)
def test_more_blocks_than_partitions_and_the_coloured_order(E, gpu, main, order):
    s = main
    f = s.bilu(order, 256)
    assert f.blocks > len(s.m.part_boundary) - 1 and np.diff(f.array("block_ptr")).max() <= 256
    solve = s.solver(order, 256)
    x, it, rel = s.plan.gmres_bilu(s.b, f, max_iter=2000, rtol=RTOL)
    _, it_cpu, _, status = lc.gmres(s.Ap, s.b, solve, max_iter=2000, rtol=RTOL)
    xb, itb, relb = s.plan.bicgstab_bilu(s.b, f, max_iter=2000, rtol=RTOL)
    _, itb_cpu, _, statusb = lc.bicgstab(s.Ap, s.b, solve, max_iter=2000, rtol=RTOL)
    print(f"block_rows 256, {order}: {f.blocks} blocks, {f.levels} levels; GMRES(30) {it} (restated {it_cpu}), BiCGSTAB {itb} (restated {itb_cpu})")
    assert rel <= RTOL and relb <= RTOL and status == statusb == "converged"
    assert abs(it - it_cpu) <= 5 and abs(itb - itb_cpu) <= 5
    for v in (x, xb):
        assert np.linalg.norm(s.b - s.Ap @ v) <= 10 * RTOL * np.linalg.norm(s.b)


# ------------------------------------------------------------------ reproducibility (plain storage)
@pytest.mark.parametrize("max_iter,restart", [(2000, 30), (47, 10)], ids=["converges", "partial-last-cycle"])
def test_gmres_is_exact_for_graph_stream_and_run(E, gpu, main, max_iter, restart):
    s = main
    f = s.bilu()
    plain = E.Plan(s.m, E.make_config(graphs=2, **PLAIN))
    run = dict(restart=restart, max_iter=max_iter, rtol=RTOL if max_iter == 2000 else 1e-30)
    ref = s.plan.gmres_bilu(s.b, f, **run)
    if max_iter == 2000:
        assert 0 < ref[1] < max_iter and ref[2] <= RTOL, ref[1:]
    else:
        assert ref[1] == max_iter and 0 < ref[2] < 1, ref[1:]
    same_bits(s.plan.gmres_bilu(s.b, f, **run), ref, "second run")
    same_bits(plain.gmres_bilu(s.b, f, **run), ref, "graphs=2")
    st = E.Stream()
    try:
        same_bits(s.plan.gmres_bilu(s.b, f, stream=st.ptr, **run), ref, "user stream")
        same_bits(plain.gmres_bilu(s.b, f, stream=st.ptr, **run), ref, "user stream, graphs=2")
    finally:
        st.destroy()


def test_bicgstab_is_exact_for_check_every_graph_stream_and_run(E, gpu, main):
    s = main
    f = s.bilu()
    plain = E.Plan(s.m, E.make_config(graphs=2, **PLAIN))
    st = E.Stream()
    try:
        kw = dict(max_iter=2000, rtol=RTOL)
        ref = s.plan.bicgstab_bilu(s.b, f, check_every=1, **kw)
        assert 0 < ref[1] < 2000 and ref[2] <= RTOL
        same_bits(s.plan.bicgstab_bilu(s.b, f, check_every=1, **kw), ref, "second run")
        same_bits(s.plan.bicgstab_bilu(s.b, f, check_every=8, **kw), ref, "check_every 8")
        same_bits(plain.bicgstab_bilu(s.b, f, check_every=1, **kw), ref, "graphs=2")
        same_bits(plain.bicgstab_bilu(s.b, f, check_every=8, stream=st.ptr, **kw), ref, "graphs=2, check_every 8, user stream")
        same_bits(s.plan.bicgstab_bilu(s.b, f, check_every=8, stream=st.ptr, **kw), ref, "user stream")
        # a fixed number of iterations, odd: the last burst ends on a single iteration
        fixed = [p.bicgstab_bilu(s.b, f, rtol=1e-30, max_iter=13, check_every=ce) for ce in (1, 8) for p in (s.plan, plain)]
        for got in fixed[1:]:
            same_bits(got, fixed[0], "13 iterations")
        assert fixed[0][1] == 13 and 0 < fixed[0][2] < 1
    finally:
        st.destroy()


def test_multi_is_the_single_solve_column_by_column(E, gpu):
    """k = 5: the apply goes in passes of four and one column, the vector kernels three and two wide, on a plan whose multiplies
    serve four.  A zero b (done at 0 iterations), a nearly converged start and random b's: the columns stop at different
    iterations, and the applies and multiplies go on serving them."""
    s = BiluSystem(E, cd_matrix(120, 100, 3000, 1), lds_doubles=20480 // 4, sym_pairs=0, direct=2)
    f = s.bilu()
    assert s.plan.spmm_max_k == 4 and f.max_k == 4
    rng = np.random.default_rng(5)
    B = np.stack([s.b, np.zeros(s.n), s.b, rng.uniform(-1, 1, s.n), s.Ap @ rng.uniform(-1, 1, s.n)])
    X0 = np.zeros_like(B)
    X0[2] = spla.spsolve(s.Ap.tocsc(), s.b) + 1e-7 * rng.uniform(-1, 1, s.n)
    for ce in (1, 8):
        kw = dict(max_iter=2000, rtol=RTOL, check_every=ce)
        singles = [s.plan.bicgstab_bilu(B[j], f, x0=X0[j], **kw) for j in range(5)]
        want = (np.stack([o[0] for o in singles]), np.array([o[1] for o in singles]), np.array([o[2] for o in singles]))
        got = s.plan.bicgstab_bilu_multi(B, f, X0=X0, **kw)
        print(f"check_every {ce}: iterations per column {list(got[1])}")
        same_bits(got, want, f"k=5, check_every {ce}")
        assert got[1][1] == 0 and got[2][1] == 0.0 and not got[0][1].any() and (got[2] <= RTOL).all()
        assert 0 < got[1][2] < got[1][0] and len(set(got[1].tolist())) >= 3, (got[1], got[2])


# ------------------------------------------------------------------ edge cases
def test_x0_given(E, gpu, main):
    s = main
    f, solve = s.bilu(), s.solver()
    x0 = np.random.default_rng(3).uniform(-1, 1, s.n)
    for name, dev, cpu in (("gmres", s.plan.gmres_bilu, lc.gmres), ("bicgstab", s.plan.bicgstab_bilu, lc.bicgstab)):
        x, it, rel = dev(s.b, f, x0=x0, max_iter=2000, rtol=RTOL)
        _, it_cpu, _, status = cpu(s.Ap, s.b, solve, x0=x0, max_iter=2000, rtol=RTOL)
        print(name, "x0 given: device", it, "restated", it_cpu)
        assert rel <= RTOL and status == "converged" and abs(it - it_cpu) <= 5
        assert np.linalg.norm(s.b - s.Ap @ x) <= 10 * RTOL * np.linalg.norm(s.b)


def test_nothing_to_do_leaves_x_alone(E, gpu, main):
    s = main
    f = s.bilu()
    for solve in (s.plan.gmres_bilu, s.plan.bicgstab_bilu):
        x, it, rel = solve(np.zeros(s.n), f, rtol=0.0)
        assert it == 0 and rel == 0.0 and np.array_equal(x.view(np.int64), np.zeros(s.n).view(np.int64))
        x0 = np.random.default_rng(4).uniform(-1, 1, s.n)
        x, it, rel = solve(s.b, f, x0=x0, max_iter=0, rtol=RTOL)
        assert it == 0 and rel > RTOL and np.array_equal(x.view(np.int64), x0.view(np.int64))


def test_nan_in_b_is_a_breakdown_and_x_stays(E, gpu, main):
    s = main
    f = s.bilu()
    rng = np.random.default_rng(12)
    b = rng.uniform(-1, 1, s.n)
    b[s.n // 3] = np.nan
    x0 = rng.uniform(-1, 1, s.n)
    for solve in (s.plan.gmres_bilu, s.plan.bicgstab_bilu):
        with pytest.raises(E.EhybError) as ei:
            solve(b, f, x0=x0)
        assert ei.value.code == ERR_ARG and "breakdown" in str(ei.value) and solve.__name__.replace("_bilu", "") in str(ei.value)
        x, it, rel = solve(b, f, x0=x0, allow_breakdown=True)
        assert it == 0 and np.isnan(rel)
        assert np.array_equal(x.view(np.int64), x0.view(np.int64))


def test_max_iter_is_the_count(E, gpu, main):
    s = main
    f = s.bilu()
    for restart in (1, 3, 7, 30):
        _, it, rel = s.plan.gmres_bilu(s.b, f, restart=restart, max_iter=7, rtol=1e-30)
        assert it == 7 and 0 < rel < 1, (restart, it, rel)
    for max_iter in (1, 6, 7):
        _, it, rel = s.plan.bicgstab_bilu(s.b, f, max_iter=max_iter, rtol=1e-30)
        assert it == max_iter and 0 < rel < 1, (max_iter, it, rel)


def test_null_outputs_and_the_c_abi(E, gpu, main):
    s = main
    f = s.bilu()
    lib = E.host._lib.load()
    want = s.plan.gmres_bilu(s.b, f, rtol=RTOL)
    db, dx = E.DeviceBuffer(s.n).upload(s.b), E.DeviceBuffer(s.n).upload(np.zeros(s.n))
    assert lib.ehyb_gmres_bilu(s.plan.h, f.h, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), 30, 2, 1000, RTOL, None, None, None) == 0
    assert np.array_equal(dx.download().view(np.int64), want[0].view(np.int64)) and np.array_equal(db.download(), s.b)
    want = s.plan.bicgstab_bilu(s.b, f, rtol=RTOL)
    dx.upload(np.zeros(s.n))
    assert lib.ehyb_bicgstab_bilu(s.plan.h, f.h, C.c_void_p(db.ptr), C.c_void_p(dx.ptr), 1000, RTOL, 10, None, None, None) == 0
    assert np.array_equal(dx.download().view(np.int64), want[0].view(np.int64)) and np.array_equal(db.download(), s.b)
    want = s.plan.bicgstab_bilu_multi(np.stack([s.b, -s.b]), f, rtol=RTOL)
    dB, dX = E.DeviceBuffer(2 * s.n).upload(np.concatenate([s.b, -s.b])), E.DeviceBuffer(2 * s.n).upload(np.zeros(2 * s.n))
    assert lib.ehyb_bicgstab_bilu_multi(s.plan.h, f.h, C.c_void_p(dB.ptr), s.n, C.c_void_p(dX.ptr), s.n, 2, 1000, RTOL, 10, None, None, None) == 0
    assert np.array_equal(dX.download().view(np.int64), want[0].ravel().view(np.int64))


def test_another_systems_factor(E, gpu, main):
    """The factor of another matrix of the same size (other values, another reordering) is still a preconditioner of sorts: the
    solve converges or stops by the rules -- max_iter or a breakdown -- and every output is what the rules say."""
    s = main
    other = BiluSystem(E, cd_matrix(120, 100, 3000, 6, pe_max=2.0), **PLAIN)
    f = other.bilu()
    assert f.n == s.n
    for solve in (s.plan.gmres_bilu, s.plan.bicgstab_bilu):
        x, it, rel = solve(s.b, f, max_iter=300, rtol=RTOL, allow_breakdown=True)
        print(solve.__name__, "with another system's factor:", it, rel)
        assert 0 <= it <= 300
        if rel <= RTOL:
            assert np.linalg.norm(s.b - s.Ap @ x) <= 10 * RTOL * np.linalg.norm(s.b)


def test_a_fallback_block(E, gpu):
    """rows of a zero diagonal in blocks of one row: s_i = 0, no alpha helps, the block takes its Jacobi form with U_DINV = 1.  The
    component [[0, 2], [2, 0]] is such a pair; GMRES solves the system all the same, and the restatement agrees."""
    A = sp.block_diag([cd_matrix(40, 30, 300, 7), sp.csr_matrix(np.array([[0.0, 2.0], [2.0, 0.0]]))]).tocsr()
    s = BiluSystem(E, A, lds_doubles=512, sym_pairs=0)
    f = s.bilu("stored", 1)
    assert f.blocks == s.n and f.fallback_blocks == 2 and f.shifted_blocks == 0
    g = lc.from_library(f)
    assert np.array_equal(g["u_dinv"][g["shift"] == lc.FALLBACK], [1.0, 1.0])
    x, it, rel = s.plan.gmres_bilu(s.b, f, max_iter=2000, rtol=RTOL)
    _, it_cpu, _, status = lc.gmres(s.Ap, s.b, s.solver("stored", 1), max_iter=2000, rtol=RTOL)
    print("fallback blocks: device", it, "restated", it_cpu)
    assert rel <= RTOL and status == "converged" and abs(it - it_cpu) <= 5
    assert np.linalg.norm(s.b - s.Ap @ x) <= 10 * RTOL * np.linalg.norm(s.b)
    x, it, rel = s.plan.bicgstab_bilu(s.b, f, max_iter=2000, rtol=RTOL, allow_breakdown=True)
    assert np.isfinite(x).all() and 0 <= it <= 2000


# ------------------------------------------------------------------ the apply
@pytest.mark.parametrize("order", ORDERS)
def test_apply(E, gpu, main, order):
    """the bar of test_gpu_bic.py's test_apply -- the same kernel, the same order of sums: componentwise within the substitution
    bound of bilu_cases.apply_bound around the apply in np.longdouble"""
    s = main
    f = s.bilu(order)
    g = lc.from_library(f)
    r = np.random.default_rng(11).uniform(-1, 1, s.n)
    z = f.apply(r)
    want = lc.apply_longdouble(g, r)
    bound = lc.apply_bound(g, r)
    err = np.abs(z - want).astype(np.float64)
    longest = int(max(np.diff(g["l_row_ptr"]).max(), np.diff(g["u_row_ptr"]).max()))
    print(f"{order}: max error / bound {np.max(err / bound):.3f}, max error {err.max():.2e}, max |z| {np.abs(z).max():.2e} "
          f"(rows of up to {longest} entries, {f.levels} levels)")
    assert (err <= bound).all()
    assert np.array_equal(z.view(np.int64), f.apply(r).view(np.int64))
    # and the compiled solves the restated solvers run on
    assert (np.abs(lc.Solver(g)(r) - want).astype(np.float64) <= bound).all()


# ------------------------------------------------------------------ refusals
def test_refusals(E, gpu, main):
    s = main
    lib = E.host._lib.load()
    small = BiluSystem(E, cd_matrix(12, 10, 20, 1), lds_doubles=512, sym_pairs=0)
    with pytest.raises(E.EhybError) as ei:
        s.plan.gmres_bilu(s.b, small.bilu())
    assert ei.value.code == ERR_ARG and f"{small.n} rows" in str(ei.value)
    p = C.c_void_p(0x10000)             # never read: the call fails before device work
    cold = E.Bilu(s.m, upload=False)
    cold_plan = E.Plan(s.m, s.cfg, upload=False)
    calls = {
        "gmres": lambda plan, f, max_iter=10: lib.ehyb_gmres_bilu(plan, f, p, p, 30, 2, max_iter, 1e-8, None, None, None),
        "bicgstab": lambda plan, f, max_iter=10: lib.ehyb_bicgstab_bilu(plan, f, p, p, max_iter, 1e-8, 10, None, None, None),
        "multi": lambda plan, f, max_iter=10: lib.ehyb_bicgstab_bilu_multi(plan, f, p, s.n, p, s.n, 2, max_iter, 1e-8, 10, None, None, None),
    }
    for name, call in calls.items():
        assert call(s.plan.h, None) == ERR_ARG and b"null bilu object" in lib.ehyb_last_error(), name
        assert call(s.plan.h, cold.h, max_iter=-1) == ERR_ARG and b"max_iter" in lib.ehyb_last_error(), name
        assert call(cold_plan.h, cold.h) == ERR_STATE and b"plan not uploaded" in lib.ehyb_last_error(), name
        assert call(s.plan.h, cold.h) == ERR_STATE and b"bilu object not uploaded" in lib.ehyb_last_error(), name
    assert lib.ehyb_bilu_apply(cold.h, p, s.n, p, s.n, 1, None) == ERR_STATE
    with pytest.raises(E.EhybError):
        cold.stream_info
