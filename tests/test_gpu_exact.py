"""Every kernel path against the EXACT product (exact_cases.py): integer values and x, so that the product is one
number in fp64 whatever the order of summation -- atomics, LDS adds, DPP group sums, split rows and the two passes
of the panel residual included -- and every multiply is compared bit for bit (np.array_equal), not to a tolerance.
y is filled with NaN before every multiply, so a row nobody writes shows.  Every case also asserts from the plan's
stats that the path it names was really taken.

The second half pins what the multiply does with non-finite values (the contract under ehyb_spmv in ehyb.h)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from exact_cases import assert_exact, exact_reference, integer_values, integer_x, nonfinite_reference, value_class
from fuzz_cases import build
from util import fem_plus_rmat

pytestmark = pytest.mark.gpu


class ExactCase:
    """generate -> integer values, integer x, exact y -> reorder (the flow of util.Case, exact)."""

    def __init__(self, E, O, gen, cfg, symmetric=True, salt=0, x_seed=1):
        self.E = E
        if gen == "fem_plus_rmat":
            m = fem_plus_rmat(E, cfg)
        else:
            m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
        self.m, self.n = m, m.n
        self.I0, self.J0, self.rp0 = m.I.copy(), m.J.copy(), m.row_idx.copy()
        m.V[:] = integer_values(m.I, m.J, symmetric, salt=salt)
        self.x = integer_x(m.n, x_seed)
        self.y_ref = exact_reference(m.n, m.I, m.J, m.V, self.x, O)
        m.reorder(cfg)
        self.perm = m.reorder_list.copy()
        self.xp = E.vector_reorder(self.x, self.perm)
        self.y_ref_p = E.vector_reorder(self.y_ref, self.perm)


def _sync(E):
    assert E.host._lib.load().ehyb_dev_sync() == 0


def multiply(E, plan, xp, phases=(0,), walk=None):
    """One multiply through plan.spmv into a y filled with NaN -> y (permuted numbering)."""
    n = len(xp)
    dx, dy = E.DeviceBuffer(n).upload(xp), E.DeviceBuffer(n).upload(np.full(n, np.nan))
    for ph in phases:
        if walk is None:
            plan.spmv(dx.ptr, dy.ptr, phase=ph)
        else:
            plan.spmv(dx.ptr, dy.ptr, walk=walk)
    _sync(E)
    y = dy.download()
    dx.free(), dy.free()
    return y


def is_direct(plan, n):
    st = plan.stats
    return st["nnz_ell"] == 0 and st["nnz_er"] == st["nnz"] and st["er_segments"] == n


def all_ways(E, plan, xp, y_ref_p, what):
    """phase 0, both explicit walk directions, and phase 1 + phase 2 where the plan has phases: all exact."""
    for walk in (None, 0, 1):
        assert_exact(multiply(E, plan, xp, walk=walk), y_ref_p, f"{what} walk={walk}")
    if not is_direct(plan, len(xp)):
        assert_exact(multiply(E, plan, xp, phases=(1, 2)), y_ref_p, f"{what} phases 1+2")


# ---------------------------------------------------------------------------------------------- fuzz seeds
@pytest.mark.parametrize("seed", range(100, 140))
def test_exact_random_plan(E, O, gpu, seed):
    """The seeds of test_gpu_fuzz.py, exact: every configuration knob drawn at random."""
    m, cfg, kw, x, y_ref, scale = build(E, O, seed, exact=True)
    plan = E.Plan(m, cfg)
    xp = E.vector_reorder(x, m.reorder_list)
    y_ref_p = E.vector_reorder(y_ref, m.reorder_list)
    for _ in range(2):                          # (an alternating walk: the second multiply walks back)
        assert_exact(multiply(E, plan, xp), y_ref_p, str(kw))
    if not is_direct(plan, m.n):
        assert_exact(multiply(E, plan, xp, phases=(1, 2)), y_ref_p, f"{kw} phases 1+2")


# ---------------------------------------------------------------------------------------------- named paths
FEM = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))
STENCIL = ("stencil2d", (150, 150, 5, 3000, 1))
RMAT11 = ("rmat", (11, 1 << 17, 3))
RMAT13 = ("rmat", (13, 1 << 16, 9))
RMAT14 = ("rmat", (14, 1 << 17, 1))
RMAT17 = ("rmat", (17, 1 << 20, 3))


def _split_rows(plan):
    return bool((plan.array("er_seg_row") < 0).any())


def _lane_codes(plan):
    return set(np.unique(plan.array("lane_group") >> 6).tolist())


# The arms of the panel residual that one vector reaches through configuration only.  RMAT14 with 2,048-column panels cut into
# seven items: 11 pass-1 units in 8 items (up to two units per item) of 1 to 298 64-entry chunks -- a 1024-thread workgroup takes
# 128 chunks per step, so the longest unit walks three steps with a ragged last one, at 512 threads five -- whose 1,880 chunks
# have longest pieces of 1, 2, 3-4, 5-8, 9-63 and 64 lanes: every early exit of the piece sums is taken, the plain wave sum
# included.  No partition keeps a window, so every pass-2 unit assigns.
PANEL_ARMS = dict(er_mode=2, fuse_er=2, direct=2, lds_doubles=512, er_panel_cols=2048, er_units1=7)


def _panel_arms(p, n):
    chunks = np.diff(p.array("pb_units1").reshape(-1, 4)[:, 2:4], axis=1) >> 6
    return p.stats["er_partials"] > 0 and chunks.max() > 128 and p.stats["nnz_ell"] == 0


def _panel_arms_two_blocks(p, n):
    """pass 2 in units of several steps (512 threads x 8 partial sums = 4,096 per step) beside units of a single partial sum"""
    sums = np.diff(p.array("pb_units2").reshape(-1, 4)[:, 0:2], axis=1)
    return _panel_arms(p, n) and sums.max() > 3 * 4096 and sums.min() == 1


# (id, matrix, config, symmetric values, what the stats must show)
PATHS = [
    ("refwindow-t256-lds1024", FEM, dict(window_mode=1, threads=256, lds_doubles=1024), True,
     lambda p, n: p.stats["nnz_ell"] > 0 and p.stats["nnz_er"] > 0),
    ("halo-t512-lds64", STENCIL, dict(window_mode=2, threads=512, lds_doubles=64), True,
     lambda p, n: p.stats["nnz_ell"] > 0),
    ("halo-t1024-lds20480", FEM, dict(window_mode=2, threads=1024, lds_doubles=20480, direct=2), True,
     lambda p, n: p.stats["nnz_ell"] > 0),
    ("refwindow-t1024-lds20480", FEM, dict(window_mode=1, threads=1024, lds_doubles=20480), True,
     lambda p, n: p.stats["nnz_ell"] > 0),
    ("inline-residual", FEM, dict(window_mode=1, lds_doubles=20480, fuse_er=1), True,
     lambda p, n: p.stats["er_inline"] > 0 and p.stats["nnz_er"] > 0),
    ("csr-split-16", RMAT11, dict(window_mode=1, lds_doubles=256, er_seg_len=16, er_mode=1, fuse_er=2), False,
     lambda p, n: _split_rows(p) and p.stats["er_inline"] == 0 and p.stats["er_partials"] == 0),
    ("csr-split-64", RMAT11, dict(window_mode=1, lds_doubles=256, er_seg_len=64, er_mode=1, fuse_er=2), False,
     lambda p, n: _split_rows(p) and p.stats["er_inline"] == 0 and p.stats["er_partials"] == 0),
    ("panel", RMAT14, dict(er_mode=2, fuse_er=2, lds_doubles=512, er_panel_cols=512, er_block_rows=300), False,
     lambda p, n: p.stats["er_partials"] > 0),
    ("panel-xcd-queues", RMAT17, dict(er_mode=2, fuse_er=2, direct=2, er_units1=3000, er_panel_cols=2048, er_queue=1), False,
     lambda p, n: p.stats["er_partials"] > 0),
    ("windowless-some", "fem_plus_rmat", dict(partitioner=1, er_mode=2, lds_doubles=4096), False,
     lambda p, n: bool(np.any(p.array("pb_units2").reshape(-1, 4)[:, 3] < 0)) and p.stats["nnz_ell"] > 0),
    ("windowless-all", ("rmat", (18, 1 << 21, 1)), dict(partitioner=1, er_mode=2, lds_doubles=4096), False,
     lambda p, n: bool(np.any(p.array("pb_units2").reshape(-1, 4)[:, 3] < 0)) and p.stats["nnz_ell"] == 0),
    ("direct-rmat", ("rmat", (13, 1 << 18, 3)), dict(), False, lambda p, n: is_direct(p, n)),
    ("direct-fem", ("fem3d", (10974, 3, 62, 59, 250000, 1, 17)), dict(), True, lambda p, n: is_direct(p, n)),
    ("sym-fem-3dof", FEM, dict(lds_doubles=4096, sym_pairs=1), True,
     lambda p, n: p.stats["sym_pairs"] > 0.2 * p.stats["nnz"] and {1, 2} <= _lane_codes(p)),
    ("sym-fem-3dof-t512-lds20480", FEM, dict(lds_doubles=20480, threads=512, sym_pairs=1), True,
     lambda p, n: p.stats["sym_pairs"] > 0.2 * p.stats["nnz"] and {1, 2} <= _lane_codes(p)),
    ("sym-fem-accidental-pairs", FEM, dict(lds_doubles=4096, sym_pairs=1), False,
     lambda p, n: 0 < p.stats["sym_pairs"] < 0.2 * p.stats["nnz"]),
    ("sym-rmat-accidental-pairs", RMAT13, dict(lds_doubles=2048, sym_pairs=1), False,
     lambda p, n: p.stats["sym_pairs"] > 0),
    ("relative-columns", ("banded", (1024 * 64, 32, 1024)), dict(direct=2), True,
     lambda p, n: bool(np.any(p.array("slab_meta").reshape(-1, 4)[:, 3] & 0x80)) and p.stats["nnz_er"] == 0),
    ("symbolic-device-panel", ("rmat", (15, 1 << 18, 1)), dict(er_mode=2, fuse_er=2, direct=2, lds_doubles=2048, symbolic=2), False,
     lambda p, n: p.stats["er_partials"] > 0 and p.stats["er_segments"] == 0),
    ("panel-scan-sums-t512", RMAT14, dict(er_sums=1, er_panel_threads=512, **PANEL_ARMS), False, _panel_arms),
    ("panel-scan-sums-t1024", RMAT14, dict(er_sums=1, er_panel_threads=1024, **PANEL_ARMS), False, _panel_arms),
    ("panel-lds-sums-t512", RMAT14, dict(er_sums=2, er_panel_threads=512, **PANEL_ARMS), False, _panel_arms),
    ("panel-lds-sums-t1024", RMAT14, dict(er_sums=2, er_panel_threads=1024, **PANEL_ARMS), False, _panel_arms),
    ("panel-pass2-streamed", RMAT14, dict(er_nt=1, **PANEL_ARMS), False, _panel_arms),
    ("panel-pass2-cached", RMAT14, dict(er_nt=2, **PANEL_ARMS), False, _panel_arms),
    ("panel-pass2-streamed-long-units", RMAT14, dict(er_nt=1, er_block_rows=16384, er_units2=2, **PANEL_ARMS), False, _panel_arms_two_blocks),
    ("panel-pass2-cached-long-units", RMAT14, dict(er_nt=2, er_block_rows=16384, er_units2=2, **PANEL_ARMS), False, _panel_arms_two_blocks),
]


@pytest.mark.parametrize("name,gen,kw,sym,taken", PATHS, ids=[p[0] for p in PATHS])
def test_exact_named_path(E, O, gpu, name, gen, kw, sym, taken):
    cfg = E.make_config(**kw)
    c = ExactCase(E, O, gen, cfg, symmetric=sym)
    plan = E.Plan(c.m, cfg)
    assert taken(plan, c.n), (name, plan.stats)
    assert plan.stats["nnz_ell"] + plan.stats["nnz_er"] == c.m.nnz
    all_ways(E, plan, c.xp, c.y_ref_p, name)
    if is_direct(plan, c.n):
        dx, dy = E.DeviceBuffer(c.n).upload(c.xp), E.DeviceBuffer(c.n)
        with pytest.raises(E.EhybError):
            plan.spmv(dx.ptr, dy.ptr, phase=1)


@pytest.mark.parametrize("threads", [512, 1024])
@pytest.mark.parametrize("er_sums", [1, 2])
def test_panel_times_probes_launch_and_leave_the_product(E, O, gpu, er_sums, threads):
    """ehyb_debug_panel_times (tools/panel_sweep.py) is the only caller of the PROBE instantiations of pass 1: with the probe values
    the tool uses it launches both passes and returns 0 (a probed result is wrong by design: nothing is asserted about it), and a
    call with probe 0 afterwards -- every row block of this plan assigns -- leaves y exactly the product.  The rows of no row block
    (they have no entry; the window launch writes them) start with their value, every other row with NaN."""
    cfg = E.make_config(er_sums=er_sums, er_panel_threads=threads, **PANEL_ARMS)
    c = ExactCase(E, O, RMAT14, cfg, symmetric=False)
    plan = E.Plan(c.m, cfg)
    assert _panel_arms(plan, c.n), plan.stats
    u2 = plan.array("pb_units2").reshape(-1, 4)
    assert bool(np.all(u2[:, 3] < 0))
    y0 = c.y_ref_p.copy()
    for first, rows in zip(u2[:, 2], -u2[:, 3]):
        y0[first:first + rows] = np.nan
    assert np.isnan(y0).sum() == -u2[:, 3].sum() > c.n // 2 and not np.any(y0[~np.isnan(y0)])
    lib = E.host._lib.load()
    lib.ehyb_debug_panel_times.restype = C.c_int
    lib.ehyb_debug_panel_times.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    dx, dy = E.DeviceBuffer(c.n).upload(c.xp), E.DeviceBuffer(c.n).upload(y0)
    plan.launched_clear()
    dpp = int(er_sums != 2)
    for probe, probed in ((0, 0), (2, 1), (0, 0)):                     # (panel_sweep.py --probes, then the product again)
        a, b = C.c_double(), C.c_double()
        assert lib.ehyb_debug_panel_times(plan.h, C.c_void_p(dx.ptr), C.c_void_p(dy.ptr), 1, probe, C.byref(a), C.byref(b)) == 0, probe
        # the launch log (rows of E.kernel_table("panel"): pass, threads, k, dpp, probe, nt): pass 1 in its plain and then its PROBE
        # instantiation, pass 2 -- whose probe is an argument, not an instantiation -- cached (these partial sums are far below the cache)
        assert (1, threads, 1, dpp, probed, 0) in plan.launched()["panel"], (probe, plan.launched())
    assert plan.launched() == dict(window=set(), er_csr=set(), panel={(1, threads, 1, dpp, 0, 0), (1, threads, 1, dpp, 1, 0), (2, 512, 1, 1, 0, 0)})
    _sync(E)
    assert_exact(dy.download(), c.y_ref_p, f"er_sums={er_sums} threads={threads} after the probes")
    dx.free(), dy.free()


@pytest.mark.parametrize("name,gen,kw,sym", [
    ("fem-plain", ("fem3d", (60000, 3, 28, 28, 13500, 1, 1)), dict(lds_doubles=4096), True),
    ("fem-symmetric-pairs", ("fem3d", (60000, 3, 28, 28, 13500, 1, 1)), dict(lds_doubles=4096, sym_pairs=1), True),
    ("rmat-panel-queues", RMAT17, dict(er_mode=2, fuse_er=2, direct=2, er_units1=3000, er_panel_cols=2048, er_queue=1), False),
], ids=lambda v: v if isinstance(v, str) else None)
def test_exact_alternating_walk(E, O, gpu, name, gen, kw, sym):
    """ell_alternate = 1: four multiplies of one plan, first to last, last to first and again -- all the exact product."""
    cfg = E.make_config(ell_alternate=1, **kw)
    c = ExactCase(E, O, gen, cfg, symmetric=sym)
    plan = E.Plan(c.m, cfg)
    n = c.n
    dx, dy = E.DeviceBuffer(n).upload(c.xp), E.DeviceBuffer(n)
    for k in range(4):
        dy.upload(np.full(n, np.nan))
        plan.spmv(dx.ptr, dy.ptr)
        _sync(E)
        assert_exact(dy.download(), c.y_ref_p, f"{name} multiply {k}")


def test_exact_tuned_plan(E, O, gpu):
    """After ehyb_plan_tune the items run on other workgroups (the tuned item map): still every entry exactly once."""
    cfg = E.make_config(sym_pairs=1)
    c = ExactCase(E, O, ("fem3d", (196608, 3, 42, 42, 13500, 1, 1)), cfg)
    plan = E.Plan(c.m, cfg)
    dx, dy = E.DeviceBuffer(c.n).upload(c.xp), E.DeviceBuffer(c.n)
    before, after = plan.tune(dx.ptr, dy.ptr, reps=3)
    assert before > 0 and 0 < after <= before
    n_items = plan.stats["n_items"]
    tuned, kept = plan.item_map()
    print(f"ehyb_plan_tune: {before:.1f} -> {after:.1f} us, {'a map was kept' if kept else 'no gain: no map'}")
    assert np.array_equal(np.sort(tuned), np.arange(n_items)), "the map in force takes every item once"
    for _ in range(2):
        assert_exact(multiply(E, plan, c.xp), c.y_ref_p, "tuned")
    # whatever the tuner found on this device: the same check under a map that is set, on every run
    shuffled = np.random.default_rng(1).permutation(n_items).astype(np.int32)
    plan.set_item_map(shuffled)
    got, installed = plan.item_map()
    assert installed and np.array_equal(got, shuffled)
    for _ in range(2):
        assert_exact(multiply(E, plan, c.xp), c.y_ref_p, "under a shuffled map")


# ---------------------------------------------------------------------------------------------- refill
def _device_set_values(plan, values, order):
    lib = plan.lib
    dv, do = C.c_void_p(), C.c_void_p()
    assert lib.ehyb_dev_alloc(values.nbytes, C.byref(dv)) == 0 and lib.ehyb_dev_alloc(order.nbytes, C.byref(do)) == 0
    try:
        assert lib.ehyb_h2d(dv, values.ctypes.data_as(C.c_void_p), values.nbytes) == 0
        assert lib.ehyb_h2d(do, order.ctypes.data_as(C.c_void_p), order.nbytes) == 0
        plan.set_values((dv.value, len(values)), entry_order=(do.value, len(order)))
        assert lib.ehyb_dev_sync() == 0
    finally:
        lib.ehyb_dev_free(dv), lib.ehyb_dev_free(do)


# (id, matrix, config, symmetric values): the plans a refill is tested on (test_gpu_range.py refills them too)
REFILL_PLANS = [
    ("plain", FEM, dict(lds_doubles=4096, direct=2), True),
    ("sym-pairs", FEM, dict(lds_doubles=4096, sym_pairs=1), True),
    ("csr-split", RMAT11, dict(window_mode=1, lds_doubles=256, er_seg_len=16, er_mode=1, fuse_er=2), False),
    ("panel", RMAT14, dict(er_mode=2, fuse_er=2, lds_doubles=512, er_panel_cols=512, er_block_rows=300), False),
    ("direct", ("rmat", (13, 1 << 18, 3)), dict(), False),
]


@pytest.mark.parametrize("name,gen,kw,sym", REFILL_PLANS, ids=lambda v: v if isinstance(v, str) else None)
@pytest.mark.parametrize("how", ["host", "device"])
def test_exact_refill(E, O, gpu, name, gen, kw, sym, how):
    """set_values with new integer values, from the host (reordered order) or the device (caller's order + entry_order):
    bit-equal to the exact product on the new values and to a plan built from scratch from them."""
    cfg = E.make_config(value_map=1, **kw)
    c = ExactCase(E, O, gen, cfg, symmetric=sym)
    plan = E.Plan(c.m, cfg)
    assert_exact(multiply(E, plan, c.xp), c.y_ref_p, f"{name} before the refill")
    V2 = integer_values(c.I0, c.J0, sym, salt=1)
    y2_ref_p = E.vector_reorder(exact_reference(c.n, c.I0, c.J0, V2, c.x), c.perm)
    order = E.entry_order(c.rp0, c.perm)
    if how == "host":
        plan.set_values(V2[order])
    else:
        _device_set_values(plan, V2, order)
    y2 = multiply(E, plan, c.xp)
    assert_exact(y2, y2_ref_p, f"{name}/{how} after the refill")
    if not is_direct(plan, c.n):
        assert_exact(multiply(E, plan, c.xp, phases=(1, 2)), y2_ref_p, f"{name}/{how} after the refill, phases 1+2")
    c.m.V[:] = V2[order]
    fresh = E.Plan(c.m, cfg)
    assert fresh.stats == plan.stats
    assert np.array_equal(multiply(E, fresh, c.xp), y2)


def _accidental_pair_plan(E, O):
    """Symmetric pair storage on a matrix that is not symmetric in value: the pairs it stores are accidental."""
    cfg = E.make_config(value_map=1, lds_doubles=4096, sym_pairs=1)
    c = ExactCase(E, O, FEM, cfg, symmetric=False)
    plan = E.Plan(c.m, cfg)
    src, src2 = plan.array("ell_src"), plan.array("ell_src2")
    paired = np.flatnonzero((src2 >= 0) & (src2 != src))
    assert len(paired) > 0 and plan.stats["sym_pairs"] > 0
    V = c.m.V.copy()
    assert np.array_equal(V[src[paired]], V[src2[paired]])         # paired by value equality
    assert not np.array_equal(V, integer_values(c.m.I, c.m.J, True))
    return c, plan, V, src[paired[len(paired) // 2]], src2[paired[len(paired) // 2]]


def test_refill_breaking_an_accidental_pair_is_refused(E, O, gpu):
    """A refill that makes an accidentally paired a_ij == a_ji unequal must be refused, not multiplied wrongly; the plan
    keeps its values (ehyb.h: left untouched).  A refill that keeps every pair equal is taken."""
    c, plan, V, a, b = _accidental_pair_plan(E, O)
    V2 = V.copy()
    V2[b] = V[b] + 1.0
    with pytest.raises(E.EhybError) as ei:
        plan.set_values(V2)
    assert ei.value.code == 1
    assert_exact(multiply(E, plan, c.xp), c.y_ref_p, "after the refused refill")
    # keeping the pairs equal: -V everywhere
    V3 = -V
    y3_ref_p = exact_reference(c.n, c.m.I, c.m.J, V3, c.xp)
    plan.set_values(V3)
    assert_exact(multiply(E, plan, c.xp), y3_ref_p, "after an accepted refill")


def test_refill_with_nan_in_a_pair_is_refused(E, O, gpu):
    """NaN never equals itself: a NaN on both sides of a stored pair counts as a pair that differs (!(V[a] == V[b]))."""
    c, plan, V, a, b = _accidental_pair_plan(E, O)
    V2 = V.copy()
    V2[a] = V2[b] = np.nan
    with pytest.raises(E.EhybError) as ei:
        plan.set_values(V2)
    assert ei.value.code == 1
    assert_exact(multiply(E, plan, c.xp), c.y_ref_p, "after the refused NaN refill")


# ---------------------------------------------------------------------------------------------- full size, CG
def test_exact_full_size_bench_configuration(E, O, gpu):
    """The bench matrix (fem3d, 943,695 rows) with symmetric integer values under bench.py --gpus 1's configuration:
    symmetric pair storage, the value stream read past the caches, an alternating walk -- two multiplies, both exact."""
    cfg = E.make_config(partitioner=E.EHYB_PART_AUTO, sym_pairs=1, value_map=1)
    c = ExactCase(E, O, ("fem3d", (943695, 3, 68, 68, 13500, 1, 1)), cfg)
    plan = E.Plan(c.m, cfg)
    st = plan.stats
    assert st["sym_pairs"] > 0.35 * st["nnz"]
    assert st["bytes_format_ell"] > (256 << 20)        # more than the Infinity Cache: non-temporal slabs, alternating walk
    dx, dy = E.DeviceBuffer(c.n).upload(c.xp), E.DeviceBuffer(c.n)
    for k in range(2):
        dy.upload(np.full(c.n, np.nan))
        plan.spmv(dx.ptr, dy.ptr)
        _sync(E)
        assert_exact(dy.download(), c.y_ref_p, f"full size, multiply {k}")


def _integer_spd(nx, ny, extra, seed):
    """The Laplacian of test_gpu_cg.py with integer couplings (-1..-3), strictly diagonally dominant: integer SPD."""
    rng = np.random.default_rng(seed)
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    r = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel(), rng.integers(0, n, extra)])
    c = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel(), rng.integers(0, n, extra)])
    keep = r != c
    r, c = r[keep], c[keep]
    v = -rng.integers(1, 4, len(r)).astype(np.float64)
    A = sp.coo_matrix((np.concatenate([v, v]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)).tocsr()
    A.sum_duplicates()
    d = np.asarray(abs(A).sum(axis=1)).ravel() + 1.0
    return (A + sp.diags(d)).tocsr()


@pytest.mark.parametrize("sym", [0, 1], ids=["plain", "symmetric-pairs"])
def test_exact_cg_first_step(E, O, gpu, sym):
    """One CG step from x = 0 on integer A and b: b.b and b.(Ab) are exact, alpha = (b.b) / (b.Ab) is one division
    (ehyb_cg.hip), so x_1 = alpha * b bit for bit, with the dot fused into the multiply (cg_fused_dot 0/1) or not (2)."""
    A = _integer_spd(120, 100, 3000, 1)
    n = A.shape[0]
    b = np.random.default_rng(3).integers(1, 16, n) * np.random.default_rng(4).choice([-1, 1], n)
    bb = int(b @ b)
    bab = int(b @ (A.astype(np.int64) @ b))
    alpha = float(Fraction(bb, bab))
    xs = []
    for fused in (0, 1, 2):
        cfg = E.make_config(window_mode=2, lds_doubles=2048, sym_pairs=sym, cg_fused_dot=fused, direct=2)
        m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=True)
        m.reorder(cfg)
        perm = m.reorder_list.copy()
        plan = E.Plan(m, cfg)
        assert plan.stats["nnz_er"] == 0 and (plan.stats["sym_pairs"] > 0) == bool(sym)
        xp, iters, rel = plan.cg(E.vector_reorder(b.astype(np.float64), perm), max_iter=1, rtol=1e-300, check_every=1)
        assert iters == 1
        xs.append(E.vector_recover(xp, perm))
    assert np.array_equal(xs[0], xs[1]) and np.array_equal(xs[1], xs[2])
    assert np.array_equal(xs[2], alpha * b.astype(np.float64))


# ---------------------------------------------------------------------------------------------- non-finite values
NONFINITE_PATHS = ["refwindow-t256-lds1024", "halo-t1024-lds20480", "inline-residual", "csr-split-16", "panel",
                   "windowless-some", "direct-rmat", "sym-fem-3dof", "sym-fem-accidental-pairs", "relative-columns",
                   "symbolic-device-panel"]
_BY_NAME = {p[0]: p for p in PATHS}


def _plant(plan, c, rng):
    """NaN, +inf and -inf at chosen entries of the reordered matrix (values stay integer elsewhere) -> entries changed.
    Entries are taken from the ELL stream, the residual (CSR segments or panel form) and a split row where the plan has
    them, and in symmetric pair storage a matched +inf pair and a NaN in place of one side of a pair."""
    m = c.m
    V = m.V
    I, J = m.I, m.J
    picks = []
    for name in ("ell_src", "er_src", "pb_src"):
        s = plan.array(name)
        s = s[s >= 0]
        if len(s):
            picks += list(rng.choice(s, min(3, len(s)), replace=False))
    seg_row = plan.array("er_seg_row")
    if (seg_row < 0).any():
        hub = int(seg_row[seg_row < 0][0] & 0x7FFFFFFF)
        picks += list(rng.choice(np.flatnonzero(I == hub), 2, replace=False))
    if not picks:                                      # direct shape: no slot maps kept
        picks = list(rng.choice(len(V), 9, replace=False))
    picks = [int(k) for k in picks]
    for k, v in zip(picks, [np.nan, np.inf, -np.inf] * len(picks)):
        V[k] = v
    src, src2 = plan.array("ell_src"), plan.array("ell_src2")
    paired = np.flatnonzero((src2 >= 0) & (src2 != src)) if len(src2) else np.zeros(0, dtype=np.int64)
    if len(paired) >= 2:
        a, b = int(src[paired[0]]), int(src2[paired[0]])
        V[a] = V[b] = np.inf                           # a matched pair: still a pair after the change
        picks += [a, b]
        a = int(src[paired[len(paired) // 2]])
        V[a] = np.nan                                  # what would otherwise be a pair
        picks.append(a)
    return picks


@pytest.mark.parametrize("name", NONFINITE_PATHS)
def test_nonfinite_matrix_values(E, O, gpu, name):
    """NaN / +inf / -inf in A, finite x: every row's class (finite, NaN, +inf, -inf) as in the exact product -- it does
    not depend on the order of summation -- and every finite row bit-exact.  An entry added to the wrong row shows up
    as a stray NaN or inf."""
    _, gen, kw, sym, taken = _BY_NAME[name]
    cfg = E.make_config(value_map=1, **kw)
    c = ExactCase(E, O, gen, cfg, symmetric=sym)
    probe = E.Plan(c.m, cfg, upload=False)           # where the entries land (slot maps), before any value changes
    picks = _plant(probe, c, np.random.default_rng(7))
    probe.destroy()
    plan = E.Plan(c.m, cfg)
    assert taken(plan, c.n), (name, plan.stats)
    y_ref = nonfinite_reference(c.n, c.m.I, c.m.J, c.m.V, c.xp)
    assert (value_class(y_ref) != 0).sum() >= 2, "the planted values must reach the product"
    for walk in (None, 0, 1):
        y = multiply(E, plan, c.xp, walk=walk)
        assert np.array_equal(value_class(y), value_class(y_ref)), (name, walk, picks)
        assert_exact(y, y_ref, f"{name} walk={walk}")
    if not is_direct(plan, c.n):
        assert_exact(multiply(E, plan, c.xp, phases=(1, 2)), y_ref, f"{name} phases 1+2")


@pytest.mark.parametrize("name", NONFINITE_PATHS)
def test_nonfinite_x(E, O, gpu, name):
    """NaN / +inf / -inf in x: every row that stores such a column comes out non-finite (a NaN is never lost; an inf
    may turn NaN, as 0 * inf in padding does), every other row is the exact product -- or NaN, through padding that
    reads column 0 of a window or of x with the value 0.0 (ehyb.h, under ehyb_spmv).  Those rows are counted."""
    _, gen, kw, sym, taken = _BY_NAME[name]
    cfg = E.make_config(**kw)
    c = ExactCase(E, O, gen, cfg, symmetric=sym)
    plan = E.Plan(c.m, cfg)
    rng = np.random.default_rng(11)
    xp = c.xp.copy()
    cols = np.unique(np.concatenate([[0], rng.choice(np.arange(1, c.n), 6, replace=False)]))
    xp[cols] = np.resize([np.nan, np.inf, -np.inf], len(cols))     # column 0: window column 0 of the first partition
    y_ref = nonfinite_reference(c.n, c.m.I, c.m.J, c.m.V, xp)
    stores = np.zeros(c.n, dtype=bool)
    stores[c.m.I[np.isin(c.m.J, cols)]] = True
    assert stores.sum() >= 6 and np.array_equal(~np.isfinite(y_ref), stores)
    for walk in (None, 0, 1):
        y = multiply(E, plan, xp, walk=walk)
        assert not np.isfinite(y[stores]).any(), (name, walk, "a non-finite x was lost")
        assert np.isnan(y[stores & np.isnan(y_ref)]).all(), (name, walk, "a NaN turned into something else")
        other = ~stores
        ok = (y[other] == y_ref[other]) | np.isnan(y[other])
        assert ok.all(), (name, walk, "a row that stores no non-finite column is neither exact nor NaN")
        print(f"{name} walk={walk}: {int(np.isnan(y[other]).sum())} of {int(other.sum())} rows without a "
              f"non-finite column came out NaN (padding)")
