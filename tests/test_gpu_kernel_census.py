"""The kernel census on the device (kernel_census_cases.py): every instantiation libehyb.so builds is launched against the EXACT
product (integer values and x: bit for bit, y filled with NaN first), and after every case the plan's launch log
(Plan.launched) equals the rows the case declares -- no more, no fewer.  test_kernel_census_host.py proves that those rows are
the library's tables.

Then what no case can say in rows alone: the static round-robin walk (cfg.ell_variant = 3) under the pinned-share arms of
cfg.ell_nt and against the LDS-counter walk bit for bit; the stamp probes; a tuned plan."""
import ctypes as C

import numpy as np
import pytest

from exact_cases import assert_exact
from kernel_census_cases import CASES, FEM, FEM24, NO_ER, CensusCase, build_matrix, check_plan, matrix_key, products, window_rows
from test_gpu_exact import _sync, multiply
from test_gpu_spmm import spmm

pytestmark = pytest.mark.gpu

SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)


def stamped_launch(E, plan, xp, y_ref, what, probe=None):
    """one ehyb_debug_ell_stamps (probe: ehyb_debug_ell_stamps_probe with that triple_gather) into a y filled with NaN and a stamp
    buffer with 64 sentinel words behind the 4 * n_items the call may write -> (y, stamps as (n_items, 4))"""
    lib = plan.lib
    n, n_items = len(xp), plan.stats["n_items"]
    buf = np.full(4 * n_items + 64, SENTINEL, dtype=np.uint64)
    dx, dy = E.DeviceBuffer(n).upload(xp), E.DeviceBuffer(n).upload(np.full(n, np.nan))
    out = buf.ctypes.data_as(C.POINTER(C.c_ulonglong))
    if probe is None:
        rc = lib.ehyb_debug_ell_stamps(plan.h, C.c_void_p(dx.ptr), C.c_void_p(dy.ptr), out)
    else:
        rc = lib.ehyb_debug_ell_stamps_probe(plan.h, C.c_void_p(dx.ptr), C.c_void_p(dy.ptr), out, probe)
    assert rc == 0, (what, lib.ehyb_last_error())
    _sync(E)
    y = dy.download()
    dx.free(), dy.free()
    assert (buf[4 * n_items:] == SENTINEL).all(), f"{what}: a word beyond the stamps of {n_items} items was written"
    st = buf[:4 * n_items].reshape(n_items, 4)
    if probe is None:
        assert_exact(y, y_ref, what)
        items = plan.array("items").reshape(-1, 8)
        has_seg = items[:, 1] > items[:, 0]
        # slot b belongs to WORKGROUP b, which takes its item through a map (XCD map, symmetric pairs heaviest first, a tuned plan):
        # every workgroup stamps entry and exit; the one whose item has a segment stamps the moment its first window was staged
        assert (st[:, 0] != 0).all() and (st[:, 0] <= st[:, 2]).all(), f"{what}: entry <= exit, nonzero, for every workgroup"
        staged = st[:, 1] != 0
        assert staged.sum() == has_seg.sum(), (what, int(staged.sum()), int(has_seg.sum()))
        s = st[staged]
        assert (s[:, 0] <= s[:, 1]).all() and (s[:, 1] <= s[:, 2]).all(), f"{what}: entry <= staged <= exit"
        assert ((st[:, 3] & np.uint64(15)) < 8).all(), f"{what}: XCC id {np.unique(st[:, 3] & np.uint64(15))}"
    return y, st


def run_ops(E, case, plan, X, Y):
    n = plan.n
    direct = case.direct
    for op in case.ops:
        if op == "spmv":
            for walk in (None, 0, 1):
                assert_exact(multiply(E, plan, X[0], walk=walk), Y[0], f"{case.id} walk={walk}")
            if not direct:
                assert_exact(multiply(E, plan, X[0], phases=(1, 2)), Y[0], f"{case.id} phases 1+2")
        elif op == "alternate4":           # (cfg.ell_alternate = 1: first to last, last to first, and again)
            for i in range(4):
                assert_exact(multiply(E, plan, X[0]), Y[0], f"{case.id} multiply {i} of an alternating walk")
        elif op == "spmm":                 # one pass of width k for k <= k_max; k = 5 splits 3 + 2 (k_max = 3: 4 -> 2 + 2 as well)
            for k in (2, 3, 4, 5):
                for walk in (None, 1):
                    Yk = spmm(E, plan, X[:k], ldx=n + 7, ldy=n + 5, walk=walk)
                    assert np.isnan(Yk[:, n:]).all(), f"{case.id} k={k}: a gap of Y was written"
                    for j in range(k):
                        assert_exact(Yk[j, :n], Y[j], f"{case.id} k={k} walk={walk} column {j}")
        elif op == "stamps":
            stamped_launch(E, plan, X[0], Y[0], f"{case.id} stamped")
        else:
            raise AssertionError(op)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_census_case(E, gpu, case):
    cfg = case.cfg(E)
    m = build_matrix(E, case)
    X, Y = products(m, matrix_key(case))
    plan = E.Plan(m, cfg)
    check_plan(case, plan, int(cfg.threads))
    assert plan.stats["nnz_ell"] + plan.stats["nnz_er"] == m.nnz
    plan.launched_clear()
    run_ops(E, case, plan, X, Y)
    log = plan.launched()
    for table, rows in case.rows.items():
        assert log[table] == rows, (case.id, table, "launched and not declared:", sorted(log[table] - rows), "declared and not launched:", sorted(rows - log[table]))
    plan.launched_clear()
    assert plan.launched() == dict(window=set(), panel=set(), er_csr=set())
    plan.destroy()


# ---------------------------------------------------------------------------------------------- static round-robin
STATIC_PLANS = [("plain", FEM, NO_ER, 0), ("sym", FEM24, dict(sym_pairs=1, **NO_ER), 1)]


@pytest.mark.parametrize("nt", [3, 4, 5])
@pytest.mark.parametrize("name,gen,kw,sym", STATIC_PLANS, ids=[p[0] for p in STATIC_PLANS])
def test_static_walk_with_a_pinned_share(E, gpu, name, gen, kw, sym, nt):
    """cfg.ell_variant = 3 under cfg.ell_nt = 3 (the end of an alternating walk kept), 4 and 5 (a spread / a block of every
    segment's slabs kept) with cfg.ell_keep = 400 and cfg.ell_alternate = 1: four multiplies, each exact; one row launched."""
    case = CensusCase(id=f"static-{name}-nt{nt}", gen=gen, kw=dict(threads=512, ell_variant=3, ell_alternate=1, ell_nt=nt, ell_keep=400, **kw),
                      ops=("alternate4", "spmv"), rows=dict(window=window_rows(512, 0, 0, sym), panel=set(), er_csr=set()), sym=sym)
    cfg = case.cfg(E)
    m = build_matrix(E, case)
    X, Y = products(m, matrix_key(case))
    plan = E.Plan(m, cfg)
    check_plan(case, plan, 512)
    if nt != 3:
        assert 0 < plan.resident_bytes < plan.device_value_bytes[0], "a share of the value stream is pinned, not all of it"
    plan.launched_clear()
    run_ops(E, case, plan, X, Y)
    assert plan.launched() == case.rows
    plan.destroy()


@pytest.mark.parametrize("form,kw", [("plain", NO_ER), ("inline", dict(window_mode=2, lds_doubles=1024, fuse_er=1, direct=2))])
@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_static_walk_is_the_lds_counter_walk_bit_for_bit(E, gpu, threads, form, kw):
    """Plain storage, real-valued data (nothing is exact, so the order of a row's sums shows): a row's sums do not depend on
    which wave takes its slab, so cfg.ell_variant = 3 and 1 on the same plan inputs give the same bits, in both walk directions."""
    ys = {}
    for variant in (1, 3):
        cfg = E.make_config(threads=threads, ell_variant=variant, **kw)
        m = E.Matrix.generate(FEM[0], *FEM[1], cfg=cfg)
        m.reorder(cfg)
        x = np.random.default_rng(5).standard_normal(m.n)
        plan = E.Plan(m, cfg)
        assert plan.stats["sym_pairs"] == 0 and not (plan.array("er_seg_row") < 0).any()
        plan.launched_clear()
        ys[variant] = [multiply(E, plan, x, walk=walk) for walk in (0, 1)]
        inl = int(plan.stats["er_inline"] > 0)
        assert inl == (form == "inline")
        assert plan.launched()["window"] == window_rows(threads, int(variant != 3), inl, 0)
        plan.destroy()
    for walk in (0, 1):
        assert np.isfinite(ys[1][walk]).all() and np.abs(ys[1][walk]).max() > 0
        assert np.array_equal(ys[1][walk].view(np.int64), ys[3][walk].view(np.int64)), f"walk {walk}: {int((ys[1][walk] != ys[3][walk]).sum())} rows differ"


# ---------------------------------------------------------------------------------------------- stamp probes, tuned plan
@pytest.mark.parametrize("variant", [1, 3], ids=["dyn", "static"])
@pytest.mark.parametrize("name,gen,kw,sym", STATIC_PLANS, ids=[p[0] for p in STATIC_PLANS])
def test_stamp_probes_launch_and_leave_the_product(E, gpu, name, gen, kw, sym, variant):
    """ehyb_debug_ell_stamps_probe (tools/stamps.py) stages the windows wrongly on purpose (triple_gather 1: from three vectors,
    2: no halo gather): it returns 0 and writes no stamp beyond its items -- nothing is asserted about its y -- and a plain
    multiply afterwards is exact."""
    case = CensusCase(id=f"probe-{name}-{variant}", gen=gen, kw=dict(threads=1024, ell_variant=variant, **kw), ops=(),
                      rows=dict(window=window_rows(1024, int(variant != 3), 0, sym, stamps=True), panel=set(), er_csr=set()), sym=sym)
    cfg = case.cfg(E)
    m = build_matrix(E, case)
    X, Y = products(m, matrix_key(case))
    plan = E.Plan(m, cfg)
    check_plan(case, plan, 1024)
    plan.launched_clear()
    for gather in (1, 2):
        stamped_launch(E, plan, X[0], Y[0], f"{case.id} triple_gather={gather}", probe=gather)
    assert plan.launched()["window"] == {(1024, 1, int(variant != 3), 1, 0, sym, 0)}
    assert_exact(multiply(E, plan, X[0]), Y[0], f"{case.id} after the probes")
    stamped_launch(E, plan, X[0], Y[0], f"{case.id} stamped after the probes")
    assert plan.launched() == case.rows
    plan.destroy()


def test_tuned_plan_logs_its_stamped_row(E, gpu):
    """ehyb_plan_tune measures stamped launches of the plan's own form: the log shows that row and no other; the next multiply
    (through the tuned item map) is exact."""
    case = CensusCase(id="tuned-sym", gen=FEM24, kw=dict(threads=512, sym_pairs=1, **NO_ER), ops=(),
                      rows=dict(window={(512, 1, 1, 1, 0, 1, 0)}, panel=set(), er_csr=set()), sym=1)
    cfg = case.cfg(E)
    m = build_matrix(E, case)
    X, Y = products(m, matrix_key(case))
    plan = E.Plan(m, cfg)
    check_plan(case, plan, 512)
    assert 16 <= plan.stats["n_items"] <= 256                  # (fewer than 16 items, or more than one round: ehyb_plan_tune is a no-op)
    dx, dy = E.DeviceBuffer(m.n).upload(X[0]), E.DeviceBuffer(m.n)
    plan.launched_clear()
    before, after = plan.tune(dx.ptr, dy.ptr, reps=2)
    assert before > 0 and 0 < after <= before
    assert plan.launched() == case.rows
    assert_exact(multiply(E, plan, X[0]), Y[0], "after ehyb_plan_tune")
    stamped_launch(E, plan, X[0], Y[0], "stamped, after ehyb_plan_tune")
    assert plan.launched()["window"] == {(512, 1, 1, 1, 0, 1, 0), (512, 1, 1, 0, 0, 1, 0)}
    n_items = plan.stats["n_items"]
    tuned, kept = plan.item_map()
    print(f"ehyb_plan_tune: {before:.1f} -> {after:.1f} us, {'a map was kept' if kept else 'no gain: no map'}")
    assert np.array_equal(np.sort(tuned), np.arange(n_items)), "the map in force takes every item once"
    # whatever the tuner found on this device: the same checks under a map that is set, on every run
    shuffled = np.random.default_rng(1).permutation(n_items).astype(np.int32)
    plan.set_item_map(shuffled)
    got, installed = plan.item_map()
    assert installed and np.array_equal(got, shuffled)
    assert_exact(multiply(E, plan, X[0]), Y[0], "under a shuffled map")
    stamped_launch(E, plan, X[0], Y[0], "stamped, under a shuffled map")
    assert plan.launched()["window"] == {(512, 1, 1, 1, 0, 1, 0), (512, 1, 1, 0, 0, 1, 0)}
    dx.free(), dy.free(), plan.destroy()
