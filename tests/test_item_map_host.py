"""The item -> workgroup map on the CPU: the decision of ehyb_plan_tune (ehyb_debug_tune_decide) against a restatement in
numpy, the map a plan that was never uploaded reports (ehyb_debug_item_map: the built-in order) against xcd_item restated here,
and what ehyb_debug_set_item_map refuses before it looks for a device.  No GPU compute is called; test_gpu_item_map.py runs the
kernels under maps set this way."""
import ctypes as C

import numpy as np
import pytest

from kernel_census_cases import FEM, FEM24, NO_ER, RMAT13D

ERR_ARG, ERR_STATE = 1, 8


# ---------------------------------------------------------------------------------------------- the decision
def restated_decision(cost, xcc, dur, map_now):
    """ehyb.h, ehyb_debug_tune_decide: median rate per XCD (the upper median of an even count), XCDs fastest first (equal rates by
    id), items by falling cost (stable), each XCD's workgroups in rising order take the next items"""
    rate = cost[map_now] / np.maximum(dur, 1e-3)
    median = {k: np.sort(rate[xcc == k])[(xcc == k).sum() // 2] for k in np.unique(xcc)}
    by_cost = np.argsort(-cost, kind="stable")
    out, at = np.full(len(cost), -1, dtype=np.int32), 0
    for k in sorted(median, key=lambda k: (-median[k], k)):
        slots = np.flatnonzero(xcc == k)
        out[slots] = by_cost[at:at + len(slots)]
        at += len(slots)
    return out


def xcd_ids(n_xcd, high):
    """n_xcd ids; high: ids of 8 and more among them (ehyb_plan_tune masks the id register with 15, so 0..15 can come)"""
    return np.array(([0, 3, 9, 12, 15, 8, 1, 14] if high else list(range(8)))[:n_xcd])


def decision_input(n, n_xcd, high, placement, costs, rates, seed):
    rng = np.random.default_rng(seed)
    ids = xcd_ids(n_xcd, high)
    if placement == "round-robin":
        xcc = ids[np.arange(n) % n_xcd]
    elif placement == "random":
        xcc = ids[rng.integers(0, n_xcd, n)]
    else:                                          # "lonely": the last XCD owns one workgroup, in the middle of the launch
        xcc = ids[np.arange(n) % (n_xcd - 1)]
        xcc[n // 2] = ids[n_xcd - 1]
    if costs == "distinct":
        cost = rng.permutation(n) * 1024.0 + 4096.0
    elif costs == "few":
        cost = rng.integers(1, 4, n) * 1024.0       # three values: the stable sort decides among equals
    else:
        cost = np.full(n, 2048.0)
    map_now = rng.permutation(n).astype(np.int32)
    if rates == "distinct":
        speed = {int(k): 1.0 + 0.07 * ((3 * j) % n_xcd) for j, k in enumerate(ids)}
        dur = cost[map_now] / np.array([speed[int(k)] for k in xcc]) * rng.uniform(0.97, 1.03, n)
    else:
        dur = cost[map_now] * 0.25                  # every rate is 4.0, exactly: the XCD's id decides
    return cost, xcc.astype(np.intc), dur, map_now


DECISIONS = [(n, n_xcd, high, placement, costs, rates)
             for n in (16, 17, 255) for n_xcd in (8, 5) for high in (False, True)
             for placement, costs, rates in (("round-robin", "distinct", "distinct"), ("random", "few", "distinct"),
                                             ("lonely", "distinct", "distinct"), ("round-robin", "equal", "distinct"),
                                             ("random", "distinct", "equal"), ("lonely", "few", "equal"))]


@pytest.mark.parametrize("n,n_xcd,high,placement,costs,rates", DECISIONS,
                         ids=["-".join(str(v) for v in d[:2]) + ("-high-" if d[2] else "-") + "-".join(d[3:]) for d in DECISIONS])
def test_decision_is_the_restatement(E, n, n_xcd, high, placement, costs, rates):
    cost, xcc, dur, map_now = decision_input(n, n_xcd, high, placement, costs, rates, seed=n * 31 + n_xcd)
    if placement != "random":
        assert len(np.unique(xcc)) == n_xcd
    if high:
        assert xcc.max() >= 8
    if placement == "lonely":
        assert (np.bincount(xcc) == 1).sum() == 1
    got = E.tune_decide(cost, xcc, dur, map_now)
    want = restated_decision(cost, xcc, dur, map_now)
    assert got is not None and np.array_equal(np.sort(got), np.arange(n)), "the decision must be a permutation"
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    if rates == "distinct" and costs == "distinct":
        # the heaviest items sit on the slots of the fastest XCD: its median rate is the largest
        rate = cost[map_now] / np.maximum(dur, 1e-3)
        fastest = max(np.unique(xcc), key=lambda k: np.sort(rate[xcc == k])[(xcc == k).sum() // 2])
        slots = np.flatnonzero(xcc == fastest)
        assert set(got[slots]) == set(np.argsort(-cost, kind="stable")[:len(slots)])
        assert cost[got[slots]].min() >= np.delete(cost, got[slots]).max()
    if rates == "equal":
        # the XCD with the lowest id is served first
        slots = np.flatnonzero(xcc == xcc.min())
        assert np.array_equal(got[slots], np.argsort(-cost, kind="stable")[:len(slots)])


@pytest.mark.parametrize("n", [16, 17, 255])
def test_an_unstable_placement_decides_nothing(E, n):
    """a workgroup that ran on two XCDs in two launches (xcc = -2): *stable = 0, map_new untouched"""
    cost, xcc, dur, map_now = decision_input(n, 8, False, "round-robin", "distinct", "distinct", seed=n)
    lib = E.host._lib.load()
    for at in (0, n // 2, n - 1):
        bad = xcc.copy()
        bad[at] = -2
        assert E.tune_decide(cost, bad, dur, map_now) is None
        out, stable = np.full(n, -7, dtype=np.int32), C.c_int(-1)
        rc = lib.ehyb_debug_tune_decide(n, cost.ctypes.data_as(C.POINTER(C.c_double)), bad.ctypes.data_as(C.POINTER(C.c_int)),
                                        dur.ctypes.data_as(C.POINTER(C.c_double)), map_now.ctypes.data_as(C.POINTER(C.c_int32)),
                                        out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(stable))
        assert rc == 0 and stable.value == 0 and (out == -7).all()
    # what would index past the decision's tables is refused: an XCD above 15, an item outside the plan
    for field, value in (("xcc", 16), ("map", n), ("map", -1)):
        x2, m2 = xcc.copy(), map_now.copy()
        if field == "xcc":
            x2[1] = value
        else:
            m2[1] = value
        with pytest.raises(E.EhybError) as ei:
            E.tune_decide(cost, x2, dur, m2)
        assert ei.value.code == ERR_ARG


# ---------------------------------------------------------------------------------------------- the built-in order
def xcd_item(b, n):
    """ell_device.h: workgroups go to the 8 XCDs round robin; XCD k takes the k-th contiguous eighth of the items"""
    k, j, chunk, rem = b & 7, b >> 3, n >> 3, n & 7
    return k * chunk + min(k, rem) + j


def host_plan(E, gen, kw):
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
    if len(gen) > 2:
        m.c.nParts, m.c.vectorCacheSize = gen[2]
    m.reorder(cfg)
    return E.Plan(m, cfg, upload=False)


PLAIN_214 = dict(items_per_cu=1, **NO_ER)                                          # 214 items: 214 % 8 = 6
PLAIN_240 = dict(window_mode=2, lds_doubles=256, items_per_cu=2, direct=2)         # 240 items: 240 % 8 = 0
BUILT_IN = [
    ("plain-ragged-eighths", FEM, PLAIN_214, 214, "xcd"),
    ("plain-whole-eighths", FEM, PLAIN_240, 240, "xcd"),
    ("plain-xcd-map-off", FEM, dict(xcd_map=2, **PLAIN_214), 214, "identity"),
    ("symmetric-pairs", FEM24, dict(sym_pairs=1, **NO_ER), 24, "identity"),
]


@pytest.mark.parametrize("name,gen,kw,n_items,order", BUILT_IN, ids=[b[0] for b in BUILT_IN])
def test_a_plan_never_uploaded_reports_the_built_in_order(E, name, gen, kw, n_items, order):
    plan = host_plan(E, gen, kw)
    assert plan.stats["n_items"] == n_items and (plan.stats["sym_pairs"] > 0) == (name == "symmetric-pairs")
    got, installed = plan.item_map()
    assert not installed and len(got) == n_items
    assert np.array_equal(np.sort(got), np.arange(n_items)), "the built-in order takes every item once"
    want = np.arange(n_items) if order == "identity" else np.array([xcd_item(b, n_items) for b in range(n_items)])
    assert np.array_equal(got, want)
    if order == "xcd":
        assert not np.array_equal(got, np.arange(n_items))
    # a buffer shorter than the map: the count, and no word beyond the buffer's
    lib = plan.lib
    few, n, inst = np.full(12, -7, dtype=np.int32), C.c_int(-1), C.c_int(-1)
    assert lib.ehyb_debug_item_map(plan.h, few.ctypes.data_as(C.POINTER(C.c_int32)), 5, C.byref(n), C.byref(inst)) == 0
    assert n.value == n_items and inst.value == 0 and np.array_equal(few[:5], want[:5]) and (few[5:] == -7).all()
    assert lib.ehyb_debug_item_map(None, None, 0, C.byref(n), C.byref(inst)) == ERR_ARG
    assert lib.ehyb_debug_item_map(plan.h, None, 3, C.byref(n), C.byref(inst)) == ERR_ARG
    plan.destroy()


# ---------------------------------------------------------------------------------------------- what the setter refuses
def _set(plan, entries, strict):
    m = np.ascontiguousarray(entries, dtype=np.int32)
    return plan.lib.ehyb_debug_set_item_map(plan.h, m.ctypes.data_as(C.POINTER(C.c_int32)), len(m), strict)


@pytest.mark.parametrize("strict", [0, 1])
def test_setter_refusals(E, strict):
    """Every argument is checked before the plan's state: on a plan that was never uploaded a bad map is EHYB_ERR_ARG and a good
    one EHYB_ERR_STATE, and the plan keeps the built-in order either way."""
    plan = host_plan(E, FEM, PLAIN_214)
    n = plan.stats["n_items"]
    before, _ = plan.item_map()
    shuffled = np.random.default_rng(2).permutation(n)
    assert plan.lib.ehyb_debug_set_item_map(None, None, 0, strict) == ERR_ARG
    assert _set(plan, shuffled[:-1], strict) == ERR_ARG, "one entry too few"
    assert _set(plan, np.r_[shuffled, 0], strict) == ERR_ARG, "one entry too many"
    for at in (0, n // 2, n - 1):
        for value in (n, -1, 2 ** 31 - 1, -2 ** 31):
            bad = shuffled.copy()
            bad[at] = value
            assert _set(plan, bad, strict) == ERR_ARG, f"entry {at} = {value} is outside the plan's items, strict or not"
            assert str(value) in plan.lib.ehyb_last_error().decode()
    twice = shuffled.copy()
    twice[n - 1] = twice[0]
    assert _set(plan, twice, strict) == (ERR_ARG if strict else ERR_STATE), "strict: a permutation; otherwise in range is enough"
    assert _set(plan, shuffled, strict) == ERR_STATE
    assert plan.lib.ehyb_debug_set_item_map(plan.h, None, 0, strict) == ERR_STATE
    assert plan.lib.ehyb_debug_set_item_map(plan.h, None, 3, strict) == ERR_ARG
    after, installed = plan.item_map()
    assert not installed and np.array_equal(after, before)
    with pytest.raises(E.EhybError) as ei:
        plan.set_item_map(shuffled, strict=bool(strict))
    assert ei.value.code == ERR_STATE
    plan.destroy()


def test_setter_refuses_the_direct_shape(E):
    plan = host_plan(E, RMAT13D, dict())
    st = plan.stats
    assert st["nnz_ell"] == 0 and st["er_segments"] == plan.n
    got, installed = plan.item_map()
    assert not installed and len(got) == st["n_items"]
    assert _set(plan, np.arange(max(st["n_items"], 1)), 1) == ERR_ARG
    assert plan.lib.ehyb_debug_set_item_map(plan.h, None, 0, 1) == ERR_ARG
    plan.destroy()
