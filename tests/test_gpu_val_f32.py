"""cfg.val_f32 on the device: the window kernel, the CSR residual, the direct shape and the refill read value streams held in
fp32 and still do fp64 arithmetic.  The contract (include/ehyb.h, under ehyb_spmv): the multiply is the fp64 multiply of the
matrix float(a_ij), per accumulator in the fp64 kernel's order.  So
  - values that fp32 holds (the +-1..7 of exact_cases.py) give the exact product on every path, bit for bit;
  - values that fp32 does not hold (val_f32_cases.tie_values: every one a rounding tie) give the exact product of the ROUNDED
    matrix, which differs from the exact product of the matrix itself;
  - with plain storage and no split rows the result equals that of an fp64 plan built from the rounded values for ANY values
    and x (np.array_equal), the solvers' iterates included; with symmetric pairs up to the order of the LDS adds.
Without the feature every test here fails at make_config(val_f32=1).

Which exact test launches which ehyb_ell_f32_kernel<THREADS, INLINE_ER, SYM> (the plan's cfg.threads, stats["er_inline"] > 0, and
symmetric pair STORAGE: cfg.sym_pairs = 1 with halo windows, whether or not the matrix had a pair to store; test_val_f32_host.py
pins the seeds' share of the table from host-only plans, and _assert_launch_log holds every plan's launch log -- what really ran,
Plan.launched() -- against it.  Until the log existed this table went by stats["sym_pairs"] > 0 and had seeds 115, 122, 123, 127
and 129, whose matrices pair nowhere, under SYM = no: they launch the SYM kernel.):

  THREADS  INLINE_ER  SYM    test_exact_random_plan_f32 (seeds)      named
  256      no         no     102 107 109 128 135 137                 refwindow-t256-lds1024
  256      no         yes    115 122 123 134
  256      yes        no     108
  256      yes        yes    120                                     test_inline_residual_with_symmetric_pairs_f32[256-*]
  512      no         no     104 114 136                             halo-t512-lds64
  512      no         yes    129 131                                 sym-fem-3dof-t512-lds20480
  512      yes        no     101
  512      yes        yes    --                                      test_inline_residual_with_symmetric_pairs_f32[512-*]
  1024     no         no     100 111 118 121 130                     refwindow-t1024-lds20480, csr-split-*, relative-columns
  1024     no         yes    127 138                                 sym-fem-3dof, sym-*-accidental-pairs
  1024     yes        no     110 117 124                             halo-t1024-lds20480, inline-residual
  1024     yes        yes    --                                      test_inline_residual_with_symmetric_pairs_f32[1024-*]
(named: ids of test_exact_named_path_f32 unless a test is named.  A plan with an inline residual also launches the arm of its row
with INLINE_ER = no, in phase 1 of a multiply in phases.  test_rounded_random_plan_f32 runs the same seeds on tie values, where the
accidental pairs of seeds 134 and 138 are gone: the storage, and so the arm, stays.)"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from exact_cases import assert_exact, exact_reference, integer_values, nonfinite_reference, value_class
from kernel_census_cases import f32_window_row
from range_cases import family
from test_gpu_exact import (FEM, PATHS, REFILL_PLANS, RMAT11, ExactCase, _device_set_values, _integer_spd, _sync, all_ways, is_direct,
                            multiply)
from val_f32_cases import FALLBACK_MAX, FEM_INLINE_SYM, FUZZ_SEEDS, f32, fuzz_case_f32, small_odd_x, tie_values, window_arm

pytestmark = pytest.mark.gpu

# the paths whose residual is not in panel form (cfg.val_f32 refuses that one at upload: test_val_f32_host.py)
F32_PATHS = [p for p in PATHS if p[2].get("er_mode") != 2]
assert len(F32_PATHS) == 14 and not any("panel" in p[0] or "windowless" in p[0] for p in F32_PATHS)


def _assert_launch_log(plan, cfg, n, what):
    """The plan's launch log against window_arm, after multiplies in one launch sequence AND in phases 1 + 2: the window launches
    since the plan was made took the fp32 row window_arm names (kernel_census_cases.f32_window_row) -- the log is what ran,
    window_arm what this file believes ran -- and the CSR residual its fp32 kernel, assigning in the direct shape.  A plan with an
    inline residual multiplies in phases WITHOUT it: phase 1 is the window kernel of the same form with no inline residual, phase 2
    the CSR residual kernel."""
    st, log = plan.stats, plan.launched()
    arm = window_arm(cfg, st)
    inline, sym = st["er_inline"] > 0, int(cfg.sym_pairs) == 1 and int(cfg.window_mode) == 2      # (the storage, not the pairs found)
    rows = {f32_window_row((cfg.threads, inline, sym)), f32_window_row((cfg.threads, False, sym))}
    if arm is not None:
        assert f32_window_row(arm) in log["window"] and log["window"] == rows, (what, arm, log["window"])
    else:                                       # no ELL entry: no launch, or one over windows that hold none
        assert log["window"] <= rows, (what, log["window"])
    # (the direct shape assigns every row, also of a matrix without an entry: one segment per row)
    er = {(1, 1, 1)} if is_direct(plan, n) else ({(1, 0, 1)} if st["nnz_er"] > 0 else set())
    assert log["er_csr"] == er and log["panel"] == set(), (what, log)


@pytest.mark.parametrize("name,gen,kw,sym,taken", F32_PATHS, ids=[p[0] for p in F32_PATHS])
def test_exact_named_path_f32(E, O, gpu, name, gen, kw, sym, taken):
    """Integer values +-1..7 (fp32 holds them) against an x fp32 cannot hold: every way of multiplying is the exact product."""
    cfg = E.make_config(val_f32=1, **kw)
    c = ExactCase(E, O, gen, cfg, symmetric=sym)
    plan = E.Plan(c.m, cfg)
    assert taken(plan, c.n), (name, plan.stats)
    assert plan.device_value_bytes[0] == 4 * len(plan.array("ell_val")) and plan.spmm_max_k == 1
    all_ways(E, plan, c.xp, c.y_ref_p, name + " val_f32")
    _assert_launch_log(plan, cfg, c.n, name)
    plan.destroy()


# ---------------------------------------------------------------------------------------------- the random configurations
_fell_back = set()


def _fuzz_f32(E, O, seed, **more):
    m, cfg, kw, x, y_ref, fell_back = fuzz_case_f32(E, O, seed, **more)
    if fell_back:
        _fell_back.add(seed)
    assert len(_fell_back) <= FALLBACK_MAX, sorted(_fell_back)
    return m, cfg, kw, x, y_ref


def _checked_f32_plan(E, m, cfg, what):
    """The upload of a configuration that passed fuzz_case_f32 must not be refused; the fp32 streams are what the device holds."""
    plan = E.Plan(m, cfg)
    assert plan.spmm_max_k == 1 and plan.device_value_bytes[0] == 4 * len(plan.array("ell_val")), what
    assert plan.stats["er_partials"] == 0 and plan.stats["nnz_ell"] + plan.stats["nnz_er"] == m.nnz, what
    return plan


def _multiplies(E, plan, n, xp, yp, what):
    for k in range(2):                          # (an alternating walk: the second multiply walks back)
        assert_exact(multiply(E, plan, xp), yp, f"{what} multiply {k}")
    if not is_direct(plan, n):
        assert_exact(multiply(E, plan, xp, phases=(1, 2)), yp, f"{what} phases 1+2")


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_exact_random_plan_f32(E, O, gpu, seed):
    """test_exact_random_plan with cfg.val_f32 = 1: every knob drawn at random, integer values (fp32 holds them) and x."""
    m, cfg, kw, x, y_ref = _fuzz_f32(E, O, seed)
    plan = _checked_f32_plan(E, m, cfg, str(kw))
    print(f"seed {seed}: n={m.n} nnz={m.nnz} window arm {window_arm(cfg, plan.stats)}")
    _multiplies(E, plan, m.n, E.vector_reorder(x, m.reorder_list), E.vector_reorder(y_ref, m.reorder_list), str(kw))
    _assert_launch_log(plan, cfg, m.n, f"seed {seed}")
    plan.destroy()


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_rounded_random_plan_f32(E, O, gpu, seed):
    """The same plans on tie values (set after the reorder, in the plan's numbering): the exact product of the ROUNDED matrix,
    which differs from that of the matrix; then a host refill with other tie values: exact again and the bits of a fresh plan."""
    m, cfg, kw, _, _ = _fuzz_f32(E, O, seed, value_map=1)
    n = m.n
    A = m.to_scipy()
    sym = m.nnz > 0 and abs(A - A.T).nnz == 0
    xp = small_odd_x(n, seed)
    V1, V2 = (tie_values(m.I, m.J, sym, salt=salt) if m.nnz else np.zeros(0) for salt in (seed, seed + 1))
    if m.nnz:
        y_full, y1, y2 = (exact_reference(n, m.I, m.J, V, xp) for V in (V1, f32(V1), f32(V2)))      # (asserts sum |a x| < 2^52)
        assert (y_full != y1).any() and (y1 != y2).any(), "rounding the values, and the refill, must change the product"
    else:
        y1 = y2 = np.zeros(n)
    m.V[:] = V1
    plan = _checked_f32_plan(E, m, cfg, str(kw))
    _multiplies(E, plan, n, xp, y1, f"{kw} ties")
    if m.nnz:                                   # (no entry: nothing to refill)
        plan.set_values(V2)
        _multiplies(E, plan, n, xp, y2, f"{kw} ties after the refill")
        m.V[:] = V2
        fresh = _checked_f32_plan(E, m, cfg, str(kw))
        assert fresh.stats == plan.stats
        assert np.array_equal(multiply(E, fresh, xp).view(np.int64), multiply(E, plan, xp).view(np.int64))
        fresh.destroy()
    plan.destroy()


# ---------------------------------------------------------------------------------------------- inline residual x symmetric pairs
def _alternating_walk_and_a_graph(E, plan, n, xp, yp, what):
    """four multiplies of an ell_alternate = 1 plan and a graph of three, as test_alternating_walk_and_graphs"""
    dx, dy = E.DeviceBuffer(n).upload(xp), E.DeviceBuffer(n)
    for k in range(4):
        dy.upload(np.full(n, np.nan))
        plan.spmv(dx.ptr, dy.ptr)
        _sync(E)
        assert_exact(dy.download(), yp, f"{what} multiply {k}")
    g = plan.graph(dx.ptr, dy.ptr, 3)
    for k in range(2):
        dy.upload(np.full(n, np.nan))
        g.launch()
        _sync(E)
        assert_exact(dy.download(), yp, f"{what} graph replay {k}")
    g.destroy()
    dx.free(), dy.free()


@pytest.mark.parametrize("triples", [1, 2], ids=["triples1", "pair-form"])
@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_inline_residual_with_symmetric_pairs_f32(E, O, gpu, threads, triples):
    """ehyb_ell_f32_kernel<THREADS, true, true>, the arm that takes 128 VGPRs: no random configuration reaches it at 512 or 1024
    threads and no named path at any size.  Integer values, tie values (the rounded reference), both walks, two phases, the
    alternating walk and a graph."""
    kw = dict(threads=threads, ell_triples=triples, ell_alternate=1, **FEM_INLINE_SYM)
    cfg = E.make_config(val_f32=1, **kw)
    c = ExactCase(E, O, FEM, cfg, symmetric=True)
    plan = _checked_f32_plan(E, c.m, cfg, str(kw))
    st = plan.stats
    assert window_arm(cfg, st) == (threads, True, True) and st["sym_pairs"] > 0.25 * st["nnz"], st
    coded = (_device_meta(plan)[:, 3] & 0x40) != 0
    print(f"threads={threads} ell_triples={triples}: {int(coded.sum())} of {len(coded)} slabs triple-coded, er_inline={st['er_inline']}")
    if triples == 2:
        assert not coded.any()
    all_ways(E, plan, c.xp, c.y_ref_p, f"{kw} integers")
    _alternating_walk_and_a_graph(E, plan, c.n, c.xp, c.y_ref_p, f"{kw} integers")
    assert plan.launched()["window"] == {(threads, 1, 1, 0, 1, 1, 1), (threads, 1, 1, 0, 0, 1, 1)}      # (the second: phase 1 of phases 1 + 2)
    _assert_launch_log(plan, cfg, c.n, str(kw))
    plan.destroy()
    t = TieCase(E, FEM, cfg, True)
    plan = _checked_f32_plan(E, t.m, cfg, str(kw))
    assert plan.stats == st and (t.y_full_p != t.y_rounded_p).mean() > 0.5
    all_ways(E, plan, t.xp, t.y_rounded_p, f"{kw} ties")
    _alternating_walk_and_a_graph(E, plan, t.n, t.xp, t.y_rounded_p, f"{kw} ties")
    plan.destroy()


class TieCase:
    """generate -> tie values, small odd x -> reorder; the exact products with V and with float(V), both asserted exact"""

    def __init__(self, E, gen, cfg, symmetric, salt=0):
        m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
        self.m, self.n = m, m.n
        self.I0, self.J0, self.rp0 = m.I.copy(), m.J.copy(), m.row_idx.copy()
        m.V[:] = tie_values(m.I, m.J, symmetric, salt=salt)
        self.x = small_odd_x(m.n, 3)
        y_full = exact_reference(m.n, m.I, m.J, m.V, self.x)                  # (asserts sum |a x| < 2^52)
        y_rounded = exact_reference(m.n, m.I, m.J, f32(m.V), self.x)
        m.reorder(cfg)
        self.perm = m.reorder_list.copy()
        self.xp = E.vector_reorder(self.x, self.perm)
        self.y_full_p, self.y_rounded_p = E.vector_reorder(y_full, self.perm), E.vector_reorder(y_rounded, self.perm)


# (id, matrix, config, symmetric values, what the stats must show)
ROUNDING_PLANS = [
    ("window", FEM, dict(lds_doubles=4096, direct=2, fuse_er=2), True, lambda p, n: p.stats["nnz_ell"] > 0 and p.stats["er_inline"] == 0),
    ("window-sym-pairs", FEM, dict(lds_doubles=4096, sym_pairs=1), True, lambda p, n: p.stats["sym_pairs"] > 0.2 * p.stats["nnz"]),
    ("inline-residual", FEM, dict(window_mode=1, lds_doubles=20480, fuse_er=1), True, lambda p, n: p.stats["er_inline"] > 0 and p.stats["nnz_er"] > 0),
    ("csr-split", RMAT11, dict(window_mode=1, lds_doubles=256, er_seg_len=16, er_mode=1, fuse_er=2), False,
     lambda p, n: bool((p.array("er_seg_row") < 0).any()) and p.stats["nnz_ell"] > 0),
    ("direct", ("rmat", (13, 1 << 18, 3)), dict(), False, is_direct),
]


@pytest.mark.parametrize("name,gen,kw,sym,taken", ROUNDING_PLANS, ids=[p[0] for p in ROUNDING_PLANS])
def test_the_rounded_values_are_what_is_multiplied(E, gpu, name, gen, kw, sym, taken):
    cfg = E.make_config(val_f32=1, **kw)
    c = TieCase(E, gen, cfg, sym)
    plan = E.Plan(c.m, cfg)
    assert taken(plan, c.n), (name, plan.stats)
    assert (c.y_full_p != c.y_rounded_p).mean() > 0.5, "rounding the values must change the product"
    all_ways(E, plan, c.xp, c.y_rounded_p, name + " ties")
    # the same plan with fp64 values multiplies the values themselves: the flag did something
    plain = E.Plan(c.m, E.make_config(**kw))
    assert_exact(multiply(E, plain, c.xp), c.y_full_p, name + " ties, fp64 values")
    plan.destroy(), plain.destroy()


# ---------------------------------------------------------------------------------------------- the sums of the fp64 kernel
def _device_meta(plan):
    lib = plan.lib
    n_words = int(lib.ehyb_plan_device_col_words(plan.h))
    words, meta = np.zeros(max(n_words, 1), dtype=np.uint32), np.zeros(len(plan.array("slab_meta")), dtype=np.uint32)
    assert lib.ehyb_plan_device_cols(plan.h, words.ctypes.data_as(C.POINTER(C.c_uint32)), meta.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    return meta.reshape(-1, 4)


@pytest.mark.parametrize("triples", [1, 2], ids=["triple-coded", "pair-form"])
@pytest.mark.parametrize("sym_pairs", [0, 1], ids=["plain", "symmetric-pairs"])
def test_same_sums_as_the_fp64_kernel(E, O, gpu, sym_pairs, triples):
    """Values with every mantissa bit in use (range_cases wide-v) and a real x: nothing is exact, so the order of the sums shows.
    Plain storage: equal, bit for bit, to the default plan of the matrix pre-rounded through float32.  Symmetric pairs: the LDS
    adds land in any order, within the project's 1e-12 * sum |a_ij x_j| per row."""
    kw = dict(lds_doubles=4096, direct=2, sym_pairs=sym_pairs, ell_triples=triples)
    cfg = E.make_config(val_f32=1, **kw)
    c = ExactCase(E, O, FEM, cfg, symmetric=True)
    V_wide, _, _ = family("wide-v", c.n, c.m.I, c.m.J, c.m.V.copy(), c.xp, c.y_ref_p, symmetric=True)
    assert (f32(V_wide) != V_wide).mean() > 0.9
    x = np.random.default_rng(8).standard_normal(c.n)
    c.m.V[:] = V_wide
    plan = E.Plan(c.m, cfg)
    coded = (_device_meta(plan)[:, 3] & 0x40) != 0
    assert coded.any() if triples == 1 else not coded.any()
    assert not (plan.array("er_seg_row") < 0).any() and (plan.stats["sym_pairs"] > 0) == bool(sym_pairs)
    c.m.V[:] = f32(V_wide)
    rounded = E.Plan(c.m, E.make_config(**kw))
    assert rounded.stats == plan.stats
    scale = abs(sp.csr_matrix((f32(V_wide), (c.m.I, c.m.J)), shape=(c.n, c.n))) @ np.abs(x)
    for walk in (0, 1):
        y, y64 = multiply(E, plan, x, walk=walk), multiply(E, rounded, x, walk=walk)
        if sym_pairs:
            assert (np.abs(y - y64) <= 1e-12 * scale).all(), (walk, float(np.max(np.abs(y - y64) / scale)))
        else:
            assert np.array_equal(y, y64), (walk, int((y != y64).sum()))
    plan.destroy(), rounded.destroy()


# ---------------------------------------------------------------------------------------------- range
def test_range_of_fp32_values(E, O, gpu):
    """On an ELL entry and on a residual entry: a row storing 2^128 comes out +-inf; rows storing multiples of 2^-140 (fp32
    subnormals) against an x of 2^100 are exact; a NaN value gives a NaN row; no other row changes class or value."""
    kw = dict(window_mode=1, threads=256, lds_doubles=1024, value_map=1)
    cfg = E.make_config(val_f32=1, **kw)
    c = ExactCase(E, O, FEM, cfg, symmetric=True)
    probe = E.Plan(c.m, cfg, upload=False)
    assert probe.stats["nnz_ell"] > 0 and probe.stats["nnz_er"] > 0 and probe.stats["er_inline"] == 0 and probe.stats["er_partials"] == 0
    I, J, Vi = c.m.I.copy(), c.m.J.copy(), c.m.V.copy()
    ell_src, er_src = probe.array("ell_src"), probe.array("er_src")
    ell_src, er_src = ell_src[ell_src >= 0], er_src[er_src >= 0]
    k_ell, k_er = int(ell_src[len(ell_src) // 3]), int(er_src[len(er_src) // 2])
    rows = (int(I[k_ell]), int(I[k_er]))
    assert rows[0] != rows[1]
    probe.destroy()

    def product(V, x):
        c.m.V[:] = V
        try:
            plan = E.Plan(c.m, cfg)
        finally:
            c.m.V[:] = Vi
        out = [multiply(E, plan, x, walk=w) for w in (0, 1)] + [multiply(E, plan, x, phases=(1, 2))]
        plan.destroy()
        return out

    # 2^128 and NaN: the class of every row, and every finite row exact
    for planted in (np.ldexp(1.0, 128), np.nan):
        V = Vi.copy()
        V[k_ell], V[k_er] = planted, -planted
        y_ref = nonfinite_reference(c.n, I, J, f32(V), c.xp)                # float(2^128) is inf
        assert (value_class(y_ref) != 0).sum() == 2 and not np.isfinite(y_ref[list(rows)]).any()
        if not np.isnan(planted):
            assert set(y_ref[list(rows)]) <= {np.inf, -np.inf}
        for y in product(V, c.xp):
            assert np.array_equal(value_class(y), value_class(y_ref))
            assert_exact(y, y_ref, f"planted {planted}")
    # fp32 subnormals: the two rows scaled by 2^-140, x by 2^100 -- every product of such a row is an integer times 2^-40
    V = Vi.copy()
    in_rows = np.isin(I, rows)
    V[in_rows] = np.ldexp(Vi[in_rows], -140)
    assert (np.abs(V[in_rows]) < np.finfo(np.float32).tiny).all() and np.array_equal(f32(V), V)
    e = np.full(c.n, 100)
    e[list(rows)] = -40
    y_ref = np.ldexp(c.y_ref_p, e)
    for y in product(V, np.ldexp(c.xp, 100)):
        assert_exact(y, y_ref, "subnormal fp32 values")


# ---------------------------------------------------------------------------------------------- refill
F32_REFILL = [p for p in REFILL_PLANS if p[0] != "panel"]
assert [p[0] for p in F32_REFILL] == ["plain", "sym-pairs", "csr-split", "direct"]


@pytest.mark.parametrize("name,gen,kw,sym", F32_REFILL, ids=[p[0] for p in F32_REFILL])
@pytest.mark.parametrize("how", ["host", "device"])
def test_refill_rounds_as_the_upload(E, gpu, name, gen, kw, sym, how):
    """set_values with tie values, from the host or from the device with entry_order: the exact product of the rounded values,
    and bit-equal to a val_f32 plan built from them."""
    cfg = E.make_config(val_f32=1, value_map=1, **kw)
    c = TieCase(E, gen, cfg, sym)
    plan = E.Plan(c.m, cfg)
    assert_exact(multiply(E, plan, c.xp), c.y_rounded_p, f"{name} before the refill")
    V2 = tie_values(c.I0, c.J0, sym, salt=1)
    assert (V2 != tie_values(c.I0, c.J0, sym)).mean() > 0.9
    y2_p = E.vector_reorder(exact_reference(c.n, c.I0, c.J0, f32(V2), c.x), c.perm)
    order = E.entry_order(c.rp0, c.perm)
    if how == "host":
        plan.set_values(V2[order])
    else:
        _device_set_values(plan, V2, order)
    y2 = multiply(E, plan, c.xp)
    assert_exact(y2, y2_p, f"{name}/{how} after the refill")
    if not is_direct(plan, c.n):
        assert_exact(multiply(E, plan, c.xp, phases=(1, 2)), y2_p, f"{name}/{how} after the refill, phases 1+2")
    c.m.V[:] = V2[order]
    fresh = E.Plan(c.m, cfg)
    assert fresh.stats == plan.stats
    assert np.array_equal(multiply(E, fresh, c.xp), y2)
    plan.destroy(), fresh.destroy()


# ---------------------------------------------------------------------------------------------- walks, graphs
@pytest.mark.parametrize("sym_pairs", [0, 1], ids=["plain", "symmetric-pairs"])
def test_alternating_walk_and_graphs(E, gpu, sym_pairs):
    cfg = E.make_config(val_f32=1, ell_alternate=1, lds_doubles=4096, sym_pairs=sym_pairs, direct=2)
    c = TieCase(E, ("fem3d", (60000, 3, 28, 28, 13500, 1, 1)), cfg, True)
    plan = E.Plan(c.m, cfg)
    dx, dy = E.DeviceBuffer(c.n).upload(c.xp), E.DeviceBuffer(c.n)
    for k in range(4):
        dy.upload(np.full(c.n, np.nan))
        plan.spmv(dx.ptr, dy.ptr)
        _sync(E)
        assert_exact(dy.download(), c.y_rounded_p, f"multiply {k}")
    g = plan.graph(dx.ptr, dy.ptr, 3)
    for k in range(2):
        dy.upload(np.full(c.n, np.nan))
        g.launch()
        _sync(E)
        assert_exact(dy.download(), c.y_rounded_p, f"graph replay {k}")
    g.destroy()
    # what cfg.val_f32 has no kernel for is refused, with the knob's name
    with pytest.raises(E.EhybError) as ei:
        plan.tune(dx.ptr, dy.ptr, reps=1)
    assert ei.value.code == 1 and "val_f32" in str(ei.value)
    dx.free(), dy.free(), plan.destroy()


def test_round_robin_variant_is_refused(E, gpu):
    cfg = E.make_config(val_f32=1, ell_variant=3, lds_doubles=4096, direct=2)
    m = E.Matrix.generate(*FEM[:1], *FEM[1], cfg=cfg)
    m.reorder(cfg)
    with pytest.raises(E.EhybError) as ei:
        E.Plan(m, cfg)
    assert ei.value.code == 1 and "val_f32" in str(ei.value)


# ---------------------------------------------------------------------------------------------- solvers
def _system(E, kw, scale, seed):
    """An _integer_spd matrix times `scale` (values fp32 cannot hold) -> (val_f32 plan of it, fp64 plan of the rounded matrix,
    b and inv_diag in the plan's numbering)"""
    A = _integer_spd(120, 100, 3000, seed) * scale
    assert (f32(A.data) != A.data).mean() > 0.9
    cfg1, cfg0 = E.make_config(val_f32=1, **kw), E.make_config(**kw)
    m = E.Matrix.from_csr(A.indptr, A.indices, A.data, cfg1, symmetric=True)
    m.reorder(cfg1)
    perm = m.reorder_list.copy()
    p32 = E.Plan(m, cfg1)
    m.V[:] = f32(m.V)
    p64 = E.Plan(m, cfg0)
    assert p32.stats == p64.stats and p32.stats["sym_pairs"] == 0 and not (p32.array("er_seg_row") < 0).any()
    n = A.shape[0]
    b = np.random.default_rng(seed + 1).standard_normal(n)
    dinv = 1.0 / f32(A.diagonal())
    return p32, p64, E.vector_reorder(b, perm), E.vector_reorder(dinv, perm)


@pytest.mark.parametrize("fused", [0, 2], ids=["fused-dot", "dot-kernel"])
def test_solvers_equal_the_fp64_plan_of_the_rounded_matrix(E, gpu, fused):
    """pcg, bicgstab and cg_multi (k = 3: three width-1 passes on the val_f32 plan) run the same arithmetic on both plans: x,
    the iteration count and the relative residual are equal bit for bit."""
    kw = dict(window_mode=2, lds_doubles=2048, direct=2, cg_fused_dot=fused)
    p32, p64, b, dinv = _system(E, kw, 1.0 + 2.0 ** -30, 1)
    n = len(b)
    B = np.stack([b, np.roll(b, 7), -2.5 * np.roll(b, 100)])
    for what, call in (("pcg", lambda p: p.cg(b, max_iter=200, rtol=1e-9, inv_diag=dinv)),
                       ("bicgstab", lambda p: p.bicgstab(b, max_iter=200, rtol=1e-9, inv_diag=dinv)),
                       ("cg_multi", lambda p: p.cg_multi(B, max_iter=200, rtol=1e-9, inv_diag=dinv))):
        x1, it1, rel1 = call(p32)
        x0, it0, rel0 = call(p64)
        assert np.all(np.asarray(it1) > 3) and np.all(np.asarray(rel1) <= 1e-9), (what, it1, rel1)
        assert np.array_equal(it1, it0) and np.array_equal(rel1, rel0) and np.array_equal(x1, x0), (what, it1, it0, rel1, rel0)
    p32.destroy(), p64.destroy()


# ---------------------------------------------------------------------------------------------- full size
def test_full_size_bench_matrix_f32(E, O, gpu):
    """The bench matrix (fem3d, 943,695 rows) with symmetric pairs, integer values and cfg.val_f32: two multiplies, exact.  In
    fp64 its window launch reads 439 MB; with fp32 values 249 MB, which is BELOW the 256 MiB of the Infinity Cache (asserted):
    such a plan reads every slab with plain loads and no launch of it takes the non-temporal arm.  So that both arms run at full
    size, the same matrix is multiplied again with half of every segment's slabs pinned (ell_keep = 500) and the other half read
    past the caches, and with plain storage, whose 430 MB do exceed the cache (asserted) and pin a share by themselves."""
    cfg = E.make_config(partitioner=E.EHYB_PART_AUTO, sym_pairs=1, val_f32=1)
    c = ExactCase(E, O, ("fem3d", (943695, 3, 68, 68, 13500, 1, 1)), cfg)

    def device_bytes(p):
        st = p.stats
        return st["bytes_format_ell"] - 8 * (st["size_block_ell"] + st["er_inline"]) + p.device_value_bytes[0]

    for what, more, fits in (("fits the cache", dict(sym_pairs=1), True), ("half pinned", dict(sym_pairs=1, ell_keep=500), True),
                             ("plain storage", dict(sym_pairs=2), False)):
        plan = E.Plan(c.m, E.make_config(partitioner=E.EHYB_PART_AUTO, val_f32=1, **more))
        st, ell_bytes = plan.stats, plan.device_value_bytes[0]
        assert (st["sym_pairs"] > 0.35 * st["nnz"]) == (more["sym_pairs"] == 1)
        assert st["bytes_format_ell"] > (256 << 20) and (device_bytes(plan) <= (256 << 20)) == fits, (what, device_bytes(plan))
        if what == "fits the cache":
            assert plan.resident_bytes == ell_bytes
        else:
            assert 0.3 * ell_bytes < plan.resident_bytes < 0.7 * ell_bytes, (what, plan.resident_bytes, ell_bytes)
        dx, dy = E.DeviceBuffer(c.n).upload(c.xp), E.DeviceBuffer(c.n)
        for k in range(2):
            dy.upload(np.full(c.n, np.nan))
            plan.spmv(dx.ptr, dy.ptr)
            _sync(E)
            assert_exact(dy.download(), c.y_ref_p, f"full size, {what}, multiply {k}")
        dx.free(), dy.free(), plan.destroy()
