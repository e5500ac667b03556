"""ehyb_pcg_bic / ehyb_pcg_bic_multi / ehyb_bic_apply on the device: CG with the block incomplete Cholesky preconditioner against
the restatement of bic_cases.py, against a direct solve and against ehyb_pcg in the same process, on the two 120 x 100 systems
of test_gpu_coarse.py (the nearly singular grid and the diagonally dominant one) with plain storage, symmetric pairs and a
CSR-residual plan for A, in both local orders.  Then apply alone against the componentwise bound of the restatement, more blocks
than partitions, the fem3d pattern with three unknowns per node, reproducibility (runs, graphs against plain launches, a user
stream, check_every), k columns bit for bit against the one-vector solves, and the refusals.  Everything in the permuted
numbering."""
import ctypes as C

import numpy as np
import pytest

import bic_cases as bc
import coarse_cases as kc
from test_gpu_cg import spd_matrix
from test_gpu_cg_multi import assert_same_bits
from test_gpu_coarse import ARMS, RTOL, System

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 8
KW = dict(lds_doubles=2048, sym_pairs=0)
ORDERS = ("stored", "colour")


class BicSystem(System):
    """System with its Bic objects by (block_rows, order) and the restatement's numbers"""

    def __init__(self, E, A, **kw):
        super().__init__(E, A, **kw)
        self.bics, self.cpu_bic = {}, {}

    def bic(self, order="stored", block_rows=0):
        if (order, block_rows) not in self.bics:
            self.bics[order, block_rows] = self.E.Bic(self.m, block_rows=block_rows, order=order)
        return self.bics[order, block_rows]

    def restated_bic(self, order="stored", block_rows=0):
        """iterations of the restatement's PCG with the library's L (check_every = 1)"""
        if (order, block_rows) not in self.cpu_bic:
            f = bc.from_library(self.bic(order, block_rows))
            self.cpu_bic[order, block_rows] = bc.pcg(self.A, self.b, bc.Solver(f), max_iter=5000, rtol=RTOL)[1]
        return self.cpu_bic[order, block_rows]


@pytest.fixture(scope="module")
def hard(E):
    return BicSystem(E, kc.near_singular_grid(120, 100, 1, 0.0005), **KW)


@pytest.fixture(scope="module")
def easy(E):
    return BicSystem(E, spd_matrix(120, 100, 3000, 1), **KW)


@pytest.fixture(params=["hard", "easy"])
def system(request, hard, easy):
    return request.param, {"hard": hard, "easy": easy}[request.param]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name,plan_kw", ARMS, ids=[a[0] for a in ARMS])
def test_solve(E, gpu, system, name, plan_kw, order):
    which, s = system
    plan, f = s.plan(**plan_kw), s.bic(order)
    if name == "symmetric-pairs":
        assert plan.stats["sym_pairs"] > 0.25 * s.A.nnz
    if name == "csr-residual":
        assert plan.stats["nnz_er"] > 0
    assert f.shifted_blocks == 0 and f.fallback_blocks == 0 and f.blocks == len(s.m.part_boundary) - 1
    x, it, rel = plan.cg_bic(s.b, f, max_iter=5000, rtol=RTOL, check_every=1)
    _, it_jacobi, rel_jacobi = plan.cg(s.b, max_iter=5000, rtol=RTOL, check_every=1, inv_diag=s.inv_diag)
    print(f"{which}, {name}, {order}: {f.blocks} blocks, {f.levels} levels, Jacobi-PCG on the device {it_jacobi} iterations")
    s.check(f"{name}, {order}", x, it, rel, s.restated_bic(order))
    assert rel_jacobi <= RTOL
    if which == "hard":
        assert 1.5 * it <= it_jacobi, (it, it_jacobi)
    else:
        assert it <= it_jacobi, (it, it_jacobi)


@pytest.mark.parametrize("order", ORDERS)
def test_apply(E, gpu, system, order):
    which, s = system
    f = s.bic(order)
    g = bc.from_library(f)
    r = np.random.default_rng(11).uniform(-1, 1, s.n)
    z = f.apply(r)
    want = bc.apply_longdouble(g, r)
    bound = bc.apply_bound(g, r)
    err = np.abs(z - want).astype(np.float64)
    longest = int(np.diff(g["row_ptr"]).max())
    print(f"{which}, {order}: max error / bound {np.max(err / bound):.3f}, max error {err.max():.2e}, max |z| {np.abs(z).max():.2e} "
          f"(rows of up to {longest} entries, {f.levels} levels)")
    assert (err <= bound).all()
    assert np.array_equal(z.view(np.int64), f.apply(r).view(np.int64))
    # and the compiled solves the restatement's PCG runs on
    assert (np.abs(bc.apply(g, r) - want).astype(np.float64) <= bound).all()


@pytest.mark.parametrize("order", ORDERS)
def test_more_blocks_than_partitions(E, gpu, hard, order):
    s = hard
    f = s.bic(order, 256)
    assert f.blocks > len(s.m.part_boundary) - 1 and np.diff(f.array("block_ptr")).max() <= 256
    x, it, rel = s.plan().cg_bic(s.b, f, max_iter=5000, rtol=RTOL, check_every=1)
    print(f"block_rows 256, {order}: {f.blocks} blocks, {f.levels} levels; whole partitions take {s.restated_bic(order)} iterations")
    s.check(f"block_rows 256, {order}", x, it, rel, s.restated_bic(order, 256))


@pytest.mark.parametrize("order", ORDERS)
def test_three_unknowns_per_node(E, gpu, order):
    """the pattern of a small fem3d matrix with SPD values: longer rows, and blocks of 3 x 3 node couplings"""
    pattern = E.Matrix.generate("fem3d", 3000, 3, 10, 10, 13500, 1, 7).to_scipy()
    s = BicSystem(E, kc.spd_on_the_pattern(pattern, 0.01), lds_doubles=1024, sym_pairs=0)
    f = s.bic(order)
    g = bc.from_library(f)
    nbytes, entries, threads = f.stream_info
    print(f"fem3d pattern, {order}: {f.blocks} blocks, levels {f.levels} (forward {g['level_f'].max() + 1}, backward {g['level_b'].max() + 1}), "
          f"rows of up to {int(np.diff(g['row_ptr']).max())} entries, {entries} entries in {nbytes} bytes of streams, {threads} threads, "
          f"{f.shifted_blocks} shifted, {f.fallback_blocks} fallen back")
    x, it, rel = s.plan().cg_bic(s.b, f, rtol=RTOL, check_every=1)
    s.check(f"fem3d pattern, {order}", x, it, rel, s.restated_bic(order))


# ------------------------------------------------------------------ reproducibility (plain storage)
@pytest.mark.parametrize("order", ORDERS)
def test_runs_graphs_streams_and_check_every_agree_bit_for_bit(E, gpu, hard, order):
    s = hard
    plan, plain, f = s.plan(), s.plan(graphs=2), s.bic(order)
    kw = dict(max_iter=5000, rtol=RTOL, check_every=2)
    st = E.Stream()
    runs = [plan.cg_bic(s.b, f, **kw), plan.cg_bic(s.b, f, **kw), plain.cg_bic(s.b, f, **kw), plan.cg_bic(s.b, f, stream=st.ptr, **kw)]
    assert runs[0][2] <= RTOL
    for x, it, rel in runs[1:]:
        assert it == runs[0][1] and rel == runs[0][2] and np.array_equal(x.view(np.int64), runs[0][0].view(np.int64))
    # a fixed number of iterations, looked at after every one or once in seven
    fixed = [p.cg_bic(s.b, f, rtol=1e-30, max_iter=14, check_every=ce) for ce in (1, 7) for p in (plan, plain)]
    for x, it, rel in fixed[1:]:
        assert it == fixed[0][1] == 14 and rel == fixed[0][2] and 0 < rel < 1 and np.array_equal(x.view(np.int64), fixed[0][0].view(np.int64))
    st.destroy()


@pytest.mark.parametrize("order", ORDERS)
def test_multi_is_the_single_solve_column_by_column(E, gpu, order):
    """k = 5: the apply goes in passes of four and one column, r.z launches three and two wide, on a plan whose passes serve four.
    The bank of test_gpu_coarse.py's test of the same name -- a zero b (done at 0 iterations), a nearly converged start and random
    b's: the columns freeze at different check points, so the flags change while the solve runs."""
    s = BicSystem(E, kc.near_singular_grid(120, 100, 1, 0.0005), lds_doubles=20480 // 4, sym_pairs=0, direct=2)
    plan, f = s.plan(), s.bic(order)
    assert plan.spmm_max_k == 4 and f.max_k == 4
    assert (plan.array("er_seg_row") >= 0).all(), "no residual row may be split into segments"
    rng = np.random.default_rng(5)
    B = np.stack([s.b, np.zeros(s.n), s.b, rng.uniform(-1, 1, s.n), s.A @ rng.uniform(-1, 1, s.n)])
    X0 = np.zeros_like(B)
    X0[2] = s.solved()[0] + 1e-7 * rng.uniform(-1, 1, s.n)
    kw = dict(max_iter=5000, rtol=RTOL, check_every=2)
    singles = [plan.cg_bic(B[j], f, x0=X0[j], **kw) for j in range(5)]
    want = (np.stack([o[0] for o in singles]), np.array([o[1] for o in singles]), np.array([o[2] for o in singles]))
    got = plan.cg_bic_multi(B, f, X0=X0, **kw)
    print(f"{order}: iterations per column {list(got[1])}")
    assert_same_bits(got, want, f"k=5 {order}")
    assert got[1][1] == 0 and got[2][1] == 0.0 and not got[0][1].any() and (got[2] <= RTOL).all()
    assert 0 < got[1][2] < got[1][0] and len(set(got[1].tolist())) >= 3, (got[1], got[2])


# ------------------------------------------------------------------ refusals
def test_refusals(E, gpu, hard):
    s = hard
    lib = E.host._lib.load()
    small = BicSystem(E, kc.near_singular_grid(12, 10, 1, 0.0005), **KW)
    with pytest.raises(E.EhybError) as ei:
        s.plan().cg_bic(s.b, small.bic())
    assert ei.value.code == ERR_ARG and f"{small.n} rows" in str(ei.value)
    p = C.c_void_p(0x10000)             # never read: the call fails before device work
    cold = E.Bic(s.m, upload=False)
    cold_plan = E.Plan(s.m, s.cfg, upload=False)
    assert lib.ehyb_pcg_bic(s.plan().h, None, p, p, 10, 1e-8, 10, None, None, None) == ERR_ARG and b"null bic object" in lib.ehyb_last_error()
    assert lib.ehyb_pcg_bic(s.plan().h, cold.h, p, p, -1, 1e-8, 10, None, None, None) == ERR_ARG and b"max_iter" in lib.ehyb_last_error()
    assert lib.ehyb_pcg_bic(cold_plan.h, cold.h, p, p, 10, 1e-8, 10, None, None, None) == ERR_STATE and b"plan not uploaded" in lib.ehyb_last_error()
    assert lib.ehyb_pcg_bic(s.plan().h, cold.h, p, p, 10, 1e-8, 10, None, None, None) == ERR_STATE and b"bic object not uploaded" in lib.ehyb_last_error()
    assert lib.ehyb_pcg_bic_multi(s.plan().h, cold.h, p, s.n, p, s.n, 2, 10, 1e-8, 10, None, None, None) == ERR_STATE
    assert lib.ehyb_bic_apply(cold.h, p, s.n, p, s.n, 1, None) == ERR_STATE
    with pytest.raises(E.EhybError):
        cold.stream_info
