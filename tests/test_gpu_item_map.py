"""Every window kernel under an item map that the TEST sets (ehyb_debug_set_item_map), not one ehyb_plan_tune may or may not keep.

a  exact under every map: integer values and x (exact_cases.py), y filled with NaN first -- every item is taken exactly once.
b  the kernel READS the map.  A kernel that ignored the map would pass (a): the built-in order takes every item once as well.
   So (b) sets a map that is NOT a permutation (strict = 0): item j is replaced by a second copy of item i.  Two workgroups then
   write identical values to item i's rows, nobody writes item j's: those rows keep the NaN they were filled with, every other row
   is exact.  A kernel that takes its item from anywhere else than the map writes them.  (ehyb_spmv_t zeroes y and adds: item i's
   rows count twice, item j's not at all.)  Plain storage only, on plans where no other launch assigns those rows (the CSR residual
   of the plan of several rounds adds to them: NaN stays NaN).
   What (b) cannot show on the plan of several rounds is WHICH workgroup took which entry of the map: a launch that walks from the
   far end reads map[n - 1 - b], and map[b] instead would take the same items.  It shows that this launch reads the map too.
c  plain storage, real-valued data: the bits of y do not depend on the map (a row's sums are formed inside one slab), nor do the
   iterates of a solver whose dot products come from the dot kernel.  With the dot fused into the multiply the partial sums land in
   other slots of the sum: the bounds of test_gpu_cg.py::test_dot_product_left_by_the_multiply for this system.
d  a graph captured under a map that was replaced and then removed is still exact; maps replaced are freed with the plan.
e  ehyb_plan_tune on top of a set map ends with a permutation, whichever map it keeps.

Plans are the small ones of kernel_census_cases.py (30,000-row FEM), one workgroup per item: 214 items (214 % 8 = 6) with plain
storage, 24 with symmetric pairs, 102 and 121 with an inline residual; and 573 items from 64-double windows, more than the 512
workgroups two rounds hold, where ehyb_spmv_walk 1 takes the items from the far end (reverse_items)."""
import numpy as np
import pytest

from exact_cases import assert_exact, exact_reference, integer_values, integer_x
from kernel_census_cases import FEM, FEM24, NO_ER
from test_gpu_cg import cpu_cg, spd_matrix
from test_gpu_exact import _sync, multiply
from test_gpu_gmres import RTOL, System, _same_bits, cd_matrix, rhs
from test_gpu_kernel_census import stamped_launch
from test_gpu_spmm import spmm
from test_gpu_spmv_t import multiply_t
from val_f32_cases import FEM_INLINE_SYM

pytestmark = pytest.mark.gpu

PLAIN = dict(items_per_cu=1, **NO_ER)
INLINE = dict(window_mode=2, lds_doubles=1024, fuse_er=1, direct=2)
ROUNDS = dict(window_mode=2, lds_doubles=64, items_per_cu=4, fuse_er=2, direct=2)
# cfg fields that change no host array: one matrix serves the plans that differ in these only
DEVICE_ONLY = ("threads", "ell_variant", "ell_alternate", "val_f32")


class Case:
    """matrix (integer values; unsymmetric unless the plan stores symmetric pairs, so that A^T x differs from A x) reordered once,
    four integer columns and their exact products A x and A^T x in the permuted numbering.  Shared: nobody changes it."""

    def __init__(self, E, gen, kw, sym):
        cfg = E.make_config(**kw)
        m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
        m.V[:] = integer_values(m.I, m.J, bool(sym))
        if len(gen) > 2:
            m.c.nParts, m.c.vectorCacheSize = gen[2]
        m.reorder(cfg)
        self.m, self.n = m, m.n
        self.X = np.stack([integer_x(m.n, j + 1) for j in range(4)])
        self.Y = np.stack([exact_reference(m.n, m.I, m.J, m.V, x) for x in self.X])
        self.Yt = exact_reference(m.n, m.J, m.I, m.V, self.X[0])
        assert sym or (self.Yt != self.Y[0]).sum() > m.n // 2


_cases = {}


def case_and_plan(E, gen, kw, sym=0):
    host_kw = {k: v for k, v in kw.items() if k not in DEVICE_ONLY}
    key = (gen, tuple(sorted(host_kw.items())), sym)
    if key not in _cases:
        _cases[key] = Case(E, gen, host_kw, sym)
    c = _cases[key]
    plan = E.Plan(c.m, E.make_config(**kw))
    assert (plan.stats["sym_pairs"] > 0) == bool(sym) and plan.stats["er_partials"] == 0
    assert len(plan.array("pb_units2")) == 0, "no panel form, no partition without a window: the item map reaches every row"
    return c, plan


def strict_maps(E, n, seed=3):
    """the maps of the issue, all permutations: identity, reversal, rotation by one, a seeded shuffle, and what the tuner's
    decision makes of a synthetic launch (XCD b mod 8, XCD k streaming at 1 + k / 10)"""
    rng = np.random.default_rng(seed)
    ident = np.arange(n, dtype=np.int32)
    cost = 4096.0 + 512.0 * rng.permutation(n)
    xcc = ident % 8
    decided = E.tune_decide(cost, xcc, cost / (1.0 + 0.1 * xcc), ident)
    maps = [("identity", ident), ("reversal", ident[::-1].copy()), ("rotation", np.roll(ident, 1)),
            ("shuffle", rng.permutation(n).astype(np.int32)), ("decided", decided)]
    for name, m in maps:
        assert np.array_equal(np.sort(m), ident), name
    assert not np.array_equal(decided, ident)
    return maps


def set_map(plan, m, strict=True):
    plan.set_item_map(m, strict=strict)
    got, installed = plan.item_map()
    assert installed and np.array_equal(got, m), "the map read back is not the map that was set"


# ---------------------------------------------------------------------------------------------- a. exact under every map
# (id, matrix, config, symmetric pairs, n_items, operations)
EXACT_ARMS = [
    ("plain-t256", FEM, dict(threads=256, **PLAIN), 0, 214, ("spmv", "spmm", "stamps", "spmv_t")),
    ("plain-t512", FEM, dict(threads=512, **PLAIN), 0, 214, ("spmv", "spmm", "stamps", "spmv_t")),
    ("plain-t1024", FEM, dict(threads=1024, **PLAIN), 0, 214, ("spmv", "spmm", "stamps", "spmv_t")),
    ("sym", FEM24, dict(sym_pairs=1, **NO_ER), 1, 24, ("spmv", "spmm", "stamps")),
    ("inline", FEM, INLINE, 0, 102, ("spmv", "spmm", "stamps", "spmv_t")),
    ("inline-sym", FEM, dict(direct=2, **FEM_INLINE_SYM), 1, 121, ("spmv", "spmm", "stamps")),
    ("static-walk", FEM, dict(ell_variant=3, **PLAIN), 0, 214, ("spmv", "stamps")),
    ("alternate", FEM, dict(ell_alternate=1, **PLAIN), 0, 214, ("alternate4",)),
    ("val-f32", FEM, dict(val_f32=1, **PLAIN), 0, 214, ("spmv",)),
    ("several-rounds", FEM, ROUNDS, 0, 573, ("walks", "spmm-walks", "spmv_t")),
]


def run_exact(E, c, plan, ops, what):
    n = c.n
    for op in ops:
        if op == "spmv":
            assert_exact(multiply(E, plan, c.X[0]), c.Y[0], f"{what} spmv")
        elif op == "walks":
            for walk in (0, 1):
                assert_exact(multiply(E, plan, c.X[0], walk=walk), c.Y[0], f"{what} walk={walk}")
        elif op == "alternate4":
            for i in range(4):
                assert_exact(multiply(E, plan, c.X[0]), c.Y[0], f"{what} multiply {i} of an alternating walk")
        elif op in ("spmm", "spmm-walks"):
            for k in (2, 3, 4):
                for walk in ((0, 1) if op == "spmm-walks" else (None,)):
                    Yk = spmm(E, plan, c.X[:k], ldx=n + 7, ldy=n + 5, walk=walk)
                    assert np.isnan(Yk[:, n:]).all(), f"{what} k={k}: a gap of Y was written"
                    for j in range(k):
                        assert_exact(Yk[j, :n], c.Y[j], f"{what} k={k} walk={walk} column {j}")
        elif op == "stamps":
            stamped_launch(E, plan, c.X[0], c.Y[0], f"{what} stamped")     # (exact y, no word beyond 4 * n_items)
        elif op == "spmv_t":
            assert_exact(multiply_t(E, plan, c.X[0])[0], c.Yt, f"{what} spmv_t")
        else:
            raise AssertionError(op)


@pytest.mark.parametrize("name,gen,kw,sym,n_items,ops", EXACT_ARMS, ids=[a[0] for a in EXACT_ARMS])
def test_exact_under_every_map(E, gpu, name, gen, kw, sym, n_items, ops):
    c, plan = case_and_plan(E, gen, kw, sym)
    assert plan.stats["n_items"] == n_items
    if name == "several-rounds":
        assert n_items > 2 * 256, "more items than two rounds of workgroups: walk 1 takes the items from the far end"
    else:
        assert 16 <= n_items <= 256
    if "spmm" in ops or "spmm-walks" in ops:
        assert plan.spmm_max_k == 4
    if "spmv_t" in ops:
        assert plan.spmv_t_supported
    for mname, m in strict_maps(E, n_items):
        set_map(plan, m)
        run_exact(E, c, plan, ops, f"{name} under the {mname} map")
    plan.set_item_map(None)
    got, installed = plan.item_map()
    assert not installed and np.array_equal(np.sort(got), np.arange(n_items))
    run_exact(E, c, plan, ops, f"{name} after the map was removed")
    plan.destroy()


# ---------------------------------------------------------------------------------------------- b. the kernel reads the map
def item_rows(plan, item):
    """the rows the slabs of `item` write (plain storage: lane l of a slab writes row slab_row + l of its segment's partition)"""
    items, segs, slab_row = plan.array("items").reshape(-1, 8), plan.array("segs").reshape(-1, 8), plan.array("slab_row")
    rows = []
    for g in range(items[item, 0], items[item, 1]):
        for s in range(segs[g, 1], segs[g, 2]):
            rows.append(np.arange(slab_row[s], min(slab_row[s] + 64, segs[g, 5])))
    return np.concatenate(rows)


def twice_and_never(n, seed=5):
    """(i, j, map): a seeded shuffle in which item j is replaced by a second copy of item i -- j, i at the first, the last and a
    middle item"""
    base = np.random.default_rng(seed).permutation(n).astype(np.int32)
    for i, j in ((n - 1, 0), (n // 2, n - 1), (0, n // 2)):
        m = base.copy()
        m[np.flatnonzero(base == j)[0]] = i
        assert (m == i).sum() == 2 and (m == j).sum() == 0
        yield i, j, m


READS_ARMS = [
    ("t256", FEM, dict(threads=256, **PLAIN), ("spmv", "spmm", "stamps", "spmv_t")),
    ("t512", FEM, dict(threads=512, **PLAIN), ("spmv", "spmm", "stamps", "spmv_t")),
    ("t1024", FEM, dict(threads=1024, **PLAIN), ("spmv", "spmm", "stamps", "spmv_t")),
    ("static-walk", FEM, dict(ell_variant=3, **PLAIN), ("spmv", "stamps")),
    ("val-f32", FEM, dict(val_f32=1, **PLAIN), ("spmv",)),
    ("several-rounds", FEM, ROUNDS, ("walks", "spmm-walks")),
]


@pytest.mark.parametrize("name,gen,kw,ops", READS_ARMS, ids=[a[0] for a in READS_ARMS])
def test_every_kernel_reads_the_map(E, gpu, name, gen, kw, ops):
    c, plan = case_and_plan(E, gen, kw)
    n, n_items = c.n, plan.stats["n_items"]
    every = np.concatenate([item_rows(plan, i) for i in range(n_items)])
    assert np.array_equal(np.sort(every), np.arange(n)), "every row belongs to the slabs of exactly one item"
    for i, j, m in twice_and_never(n_items):
        set_map(plan, m, strict=False)
        lost, doubled = item_rows(plan, j), item_rows(plan, i)
        assert len(lost) > 0 and len(doubled) > 0
        want = c.Y.copy()
        want[:, lost] = np.nan                              # nobody takes item j: its rows keep what y was filled with
        what = f"{name}: item {i} twice, item {j} never"
        for op in ops:
            if op == "spmv":
                assert_exact(multiply(E, plan, c.X[0]), want[0], f"{what}, spmv")
            elif op == "walks":
                for walk in (0, 1):
                    assert_exact(multiply(E, plan, c.X[0], walk=walk), want[0], f"{what}, walk={walk}")
            elif op in ("spmm", "spmm-walks"):
                for k in (2, 3, 4):
                    for walk in ((0, 1) if op == "spmm-walks" else (None,)):
                        Yk = spmm(E, plan, c.X[:k], ldx=n + 7, ldy=n + 5, walk=walk)
                        assert np.isnan(Yk[:, n:]).all()
                        for col in range(k):
                            assert_exact(Yk[col, :n], want[col], f"{what}, k={k} walk={walk} column {col}")
            elif op == "stamps":
                stamped_launch(E, plan, c.X[0], want[0], f"{what}, stamped")
            elif op == "spmv_t":
                # y is zeroed and added to: the rows of item i enter the transposed product twice, those of item j not at all
                weight = np.ones(n)
                weight[doubled], weight[lost] = 2.0, 0.0
                keep = weight[c.m.I] != 0
                want_t = exact_reference(n, c.m.J[keep], c.m.I[keep], (c.m.V * weight[c.m.I])[keep], c.X[0])
                assert (want_t != c.Yt).sum() > 0
                assert_exact(multiply_t(E, plan, c.X[0])[0], want_t, f"{what}, spmv_t")
            else:
                raise AssertionError(op)
    # a permutation again: everything is exact again
    set_map(plan, np.arange(n_items, dtype=np.int32)[::-1].copy())
    assert_exact(multiply(E, plan, c.X[0]), c.Y[0], f"{name}: the reversal after the maps that are none")
    plan.destroy()


# ---------------------------------------------------------------------------------------------- c. bits do not depend on the map
def test_plain_storage_gives_the_same_bits_under_every_map(E, O, gpu):
    """real-valued data (the generator's values, O.x_glibc): nothing is exact, so an order of summation that changed would show"""
    cfg = E.make_config(**PLAIN)
    m = E.Matrix.generate(FEM[0], *FEM[1], cfg=cfg)
    m.reorder(cfg)
    n = m.n
    X = np.stack([E.vector_reorder(O.x_glibc(n), m.reorder_list)] + [np.random.default_rng(j).standard_normal(n) for j in (1, 2, 3)])
    plan = E.Plan(m, cfg)
    assert plan.stats["sym_pairs"] == 0 and plan.stats["nnz_er"] == 0
    n_items = plan.stats["n_items"]

    def all_widths():
        return [multiply(E, plan, X[0], walk=0)] + [spmm(E, plan, X[:k], ldx=n + 7, ldy=n + 5, walk=0)[:, :n] for k in (2, 3, 4)]

    ref = all_widths()
    assert all(np.isfinite(y).all() and np.abs(y).max() > 0 for y in ref)
    assert not np.array_equal(ref[0], np.round(ref[0])), "real-valued data"
    for mname, mp in strict_maps(E, n_items):
        set_map(plan, mp)
        for k, (y, y0) in enumerate(zip(all_widths(), ref), start=1):
            assert np.array_equal(y.view(np.int64), y0.view(np.int64)), f"{mname} map, k={k}: {int((y != y0).sum())} values differ"
    plan.destroy()


def _shuffled(plan, seed=9):
    n_items = plan.stats["n_items"]
    assert n_items >= 16
    m = np.random.default_rng(seed).permutation(n_items).astype(np.int32)
    set_map(plan, m)
    return plan


def test_pcg_with_the_dot_kernel_returns_the_same_bits_under_a_map(E, O, gpu):
    A = spd_matrix(120, 100, 3000, 7)
    n = A.shape[0]
    cfg = E.make_config(lds_doubles=2048, sym_pairs=0, direct=2, cg_fused_dot=2)
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=True)
    m.reorder(cfg)
    b = E.vector_reorder(O.x_glibc(n) + 0.3, m.reorder_list)
    inv_diag = E.vector_reorder(1.0 / A.diagonal(), m.reorder_list)
    run = dict(max_iter=400, rtol=1e-10, check_every=2, inv_diag=inv_diag)
    x0, it0, rel0 = E.Plan(m, cfg).cg(b, **run)
    x1, it1, rel1 = _shuffled(E.Plan(m, cfg)).cg(b, **run)
    assert 0 < it0 < 400 and rel0 <= 1e-10
    assert it1 == it0 and rel1 == rel0 and np.array_equal(x1.view(np.int64), x0.view(np.int64))


def test_gmres_returns_the_same_bits_under_a_map(E, gpu):
    s = System(E, cd_matrix(120, 100, 3000, 6), window_mode=2, lds_doubles=2048, sym_pairs=0)
    b = E.vector_reorder(rhs(s.n), s.perm)
    run = dict(restart=30, max_iter=2000, rtol=RTOL, inv_diag=s.inv_diag)
    ref = s.plan.gmres(b, **run)
    assert 0 < ref[1] < 2000 and ref[2] <= RTOL
    _same_bits(_shuffled(E.Plan(s.m, s.cfg)).gmres(b, **run), ref, "under a shuffled map")


def test_cg_with_the_fused_dot_under_a_map(E, O, gpu):
    """The partial sums of p . (A p) land in other slots of xy_out, so the iterates may differ in roundings: the system, the
    tolerances and the iteration window of test_gpu_cg.py::test_dot_product_left_by_the_multiply."""
    A = spd_matrix(120, 100, 3000, 7)
    n = A.shape[0]
    kw = dict(lds_doubles=2048, sym_pairs=0, direct=2)
    cfg = E.make_config(**kw)
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg, symmetric=True)
    m.reorder(cfg)
    perm = m.reorder_list.copy()
    fused, separate = _shuffled(E.Plan(m, cfg)), E.Plan(m, E.make_config(cg_fused_dot=2, **kw))
    st = fused.stats
    assert st["nnz_er"] == 0 or st["er_inline"] > 0, "this matrix must multiply in one window launch"
    b0 = O.x_glibc(n) + 0.3
    b = E.vector_reorder(b0, perm)
    x1, it1, rel1 = fused.cg(b, max_iter=400, rtol=1e-10, check_every=2)
    x2, it2, rel2 = separate.cg(b, max_iter=400, rtol=1e-10, check_every=2)
    _, it_cpu, _ = cpu_cg(A, b0, 400, 1e-10)
    print(f"fused dot under a map: {it1} iterations, rel {rel1:.3e}; dot kernel, no map: {it2}, rel {rel2:.3e}; cpu {it_cpu}; "
          f"|x1 - x2| / |x2| = {np.linalg.norm(x1 - x2) / np.linalg.norm(x2):.3e}")
    assert rel1 <= 1e-10 and rel2 <= 1e-10 and abs(it1 - it_cpu) <= 2 and abs(it2 - it_cpu) <= 2, (it1, it2, it_cpu)
    assert np.linalg.norm(x1 - x2) <= 1e-9 * np.linalg.norm(x2)
    x = E.vector_recover(x1, perm)
    assert np.linalg.norm(A @ x - b0) <= 2e-10 * np.linalg.norm(b0)
    x1b, _, rel1b = fused.cg(b, max_iter=400, rtol=1e-10, check_every=2)     # fixed summation order: a second solve repeats the first
    assert np.array_equal(x1, x1b) and rel1 == rel1b


# ---------------------------------------------------------------------------------------------- d. lifetime
def test_a_graph_outlives_the_map_it_was_captured_with(E, gpu):
    c, plan = case_and_plan(E, FEM, dict(threads=1024, **PLAIN))
    n_items = plan.stats["n_items"]
    maps = dict(strict_maps(E, n_items))
    dx, dy = E.DeviceBuffer(c.n).upload(c.X[0]), E.DeviceBuffer(c.n)
    set_map(plan, maps["shuffle"])
    graph = plan.graph(dx.ptr, dy.ptr)
    set_map(plan, maps["reversal"])
    plan.set_item_map(None)
    assert not plan.item_map()[1]
    for i in range(2):
        dy.upload(np.full(c.n, np.nan))
        graph.launch()
        _sync(E)
        assert_exact(dy.download(), c.Y[0], f"launch {i} of a graph captured under a map that is no longer the plan's")
    assert_exact(multiply(E, plan, c.X[0]), c.Y[0], "the plan itself, its map removed")
    graph.destroy()
    dx.free(), dy.free()
    plan.destroy()


def test_three_maps_in_a_row_then_the_plan_goes(E, gpu):
    c, plan = case_and_plan(E, FEM, dict(threads=512, **PLAIN))
    for mname, m in strict_maps(E, plan.stats["n_items"])[1:4]:
        set_map(plan, m)
    assert_exact(multiply(E, plan, c.X[0]), c.Y[0], "under the third map")
    plan.destroy()


# ---------------------------------------------------------------------------------------------- e. the tuner on top of a set map
def test_tuner_on_top_of_a_set_map(E, gpu):
    c, plan = case_and_plan(E, FEM, dict(threads=1024, **PLAIN))
    n_items = plan.stats["n_items"]
    reversal = np.arange(n_items, dtype=np.int32)[::-1].copy()
    set_map(plan, reversal)
    dx, dy = E.DeviceBuffer(c.n).upload(c.X[0]), E.DeviceBuffer(c.n)
    before, after = plan.tune(dx.ptr, dy.ptr, reps=2)
    got, installed = plan.item_map()
    print(f"ehyb_plan_tune on the reversal: {before:.1f} -> {after:.1f} us, {'its own map kept' if not np.array_equal(got, reversal) else 'the reversal put back'}")
    assert installed and np.array_equal(np.sort(got), np.arange(n_items)), "a permutation, whichever map the tuner ended with"
    assert before > 0 and 0 < after <= before
    assert_exact(multiply(E, plan, c.X[0]), c.Y[0], "after ehyb_plan_tune on a set map")
    dx.free(), dy.free()
    plan.destroy()
