"""Every kernel path against the exact product over the whole fp64 range and mantissa width (range_cases.py).

The bit-for-bit tests of test_gpu_exact.py, test_gpu_spmm.py and test_gpu_spmm_panel.py run on one kind of input: values of
three bits, x of 26, every exponent near zero.  Here the same integer cases are scaled by powers of two -- per matrix, per row,
per column -- into the subnormals and up to 2^1023, and redrawn with every mantissa bit in use.  Each still has one correct fp64
product whatever the order of summation, so every path must give it with assert_exact.  What shows here and nowhere else:
  - a value or x that loses its low mantissa bits on the way (fill kernel, LDS window, a 128-bit LDS read, a DPP move of halves);
  - a subnormal operand, product, partial sum or result flushed to zero -- the LDS and global fp64 atomic adds included (symmetric
    pairs, the piece sums and pass 2 of the panel form, split rows, ehyb_scatter_add), and a refill that takes two different
    subnormals for equal;
  - arithmetic that mixes rows: a segment sum formed as a difference of prefix sums, an accumulator not cleared between two rows,
    a fold that adds and later subtracts are all exact on homogeneous integers and wrong when neighbouring rows lie hundreds of
    binades apart (the graded families);
  - an infinity met before the end of a finite sum (high).

Observed on gfx950 (MI355X): every case is exact.  ds_add_f64 and global_atomic_add_f64, which the paths above reach through
unsafeAtomicAdd, keep subnormal operands and results, so no (path, family) pair needs a bound in place of equality; the contract
under ehyb_spmv in include/ehyb.h and DESIGN.md section 6 say so."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_spmm as S
import test_gpu_spmm_panel as SP
from exact_cases import assert_exact
from range_cases import COLUMN_EXPONENTS, FAMILIES, GRADED, _hash, columns_scaled, family, odd_integers, row_exponents
from test_gpu_exact import PATHS, REFILL_PLANS, ExactCase, _device_set_values, _sync, all_ways, is_direct, multiply

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------- single multiply
# (path, family) pairs whose `taken` cannot hold, each with its reason.  They still run, and must be exact; what is waived is
# the predicate alone, and it must then really be false, so that the list cannot go stale.  Only sym-* paths stand here, and
# only families that by their definition take the equal mirror values away that the path's predicate counts:
#   graded-rows, graded-low   scale ROWS (a_ij 2^ri, a_ji 2^rj): a matrix symmetric in value keeps a_ij == a_ji only where
#                             r_i == r_j (graded-low draws r from 75 exponents, graded-rows from 1,801), far fewer than the
#                             fifth of the entries the sym-fem-3dof paths ask for; pairs that remain are stored and multiplied
#   wide-v                    draws (i, j) and (j, i) apart on a matrix not symmetric in value: two 40-odd-bit numbers are
#                             never equal by accident, so the accidental-pair paths have no pair left
# A `taken` that fails anywhere else fails the test.
_ROWS = "rows scaled apart: a_ij 2^ri != a_ji 2^rj but where r_i == r_j, too few pairs are left"
_WIDE = "wide values of a matrix not symmetric in value are never equal by accident: no pair is left"
CANNOT_HOLD = {
    ("sym-fem-3dof", "graded-rows"): _ROWS,
    ("sym-fem-3dof", "graded-low"): _ROWS,
    ("sym-fem-3dof-t512-lds20480", "graded-rows"): _ROWS,
    ("sym-fem-3dof-t512-lds20480", "graded-low"): _ROWS,
    ("sym-rmat-accidental-pairs", "graded-rows"): _ROWS,
    ("sym-fem-accidental-pairs", "wide-v"): _WIDE,
    ("sym-rmat-accidental-pairs", "wide-v"): _WIDE,
}
SYM_PATHS = [p[0] for p in PATHS if p[0].startswith("sym-")]
CASES = [(p, fam) for p in PATHS for fam in FAMILIES]


def test_the_exclusion_list_is_within_its_cap():
    names = [p[0] for p in PATHS]
    assert len(SYM_PATHS) >= 4
    for (name, fam), reason in CANNOT_HOLD.items():
        assert name in SYM_PATHS and fam in ("wide-v", "graded-rows", "graded-low") and reason, (name, fam)
    asserted = {name: {fam for fam in FAMILIES if (name, fam) not in CANNOT_HOLD} for name in names}
    for name in names:
        assert {"low", "high", "wide-x"} <= asserted[name] and asserted[name] & set(GRADED), name
    for name in SYM_PATHS:
        assert {"graded-sym", "low-v", "low", "low-x", "high", "wide-x"} <= asserted[name], name


_case = {}


def path_case(E, O, name, gen, kw, sym, extra=None):
    """The ExactCase of a path: generated and reordered once per path (the parametrisation runs path by path)."""
    key = (name, tuple(sorted((extra or {}).items())))
    if key not in _case:
        _case.clear()
        cfg = E.make_config(**kw, **(extra or {}))
        c = ExactCase(E, O, gen, cfg, symmetric=sym)
        c.Vi = c.m.V.copy()                     # the integer case in the plan's numbering: (m.I, m.J, Vi, xp, y_ref_p)
        _case[key] = (c, cfg)
    return _case[key]


def family_of(c, fam, sym, x_salt=0):
    return family(fam, c.n, c.m.I, c.m.J, c.Vi, c.xp, c.y_ref_p, symmetric=sym, x_salt=x_salt)


@pytest.mark.parametrize("path,fam", CASES, ids=[f"{p[0]}-{fam}" for p, fam in CASES])
def test_range_named_path(E, O, gpu, path, fam):
    name, gen, kw, sym, taken = path
    c, cfg = path_case(E, O, name, gen, kw, sym)
    V2, x2, y2 = family_of(c, fam, sym)
    c.m.V[:] = V2
    try:
        plan = E.Plan(c.m, cfg)
    finally:
        c.m.V[:] = c.Vi
    if (name, fam) in CANNOT_HOLD:
        assert not taken(plan, c.n), (name, fam, "listed in CANNOT_HOLD, but the path is taken", plan.stats)
    else:
        assert taken(plan, c.n), (name, fam, plan.stats)
    assert plan.stats["nnz_ell"] + plan.stats["nnz_er"] == c.m.nnz
    all_ways(E, plan, x2, y2, f"{name} {fam}")
    plan.destroy()


# ---------------------------------------------------------------------------------------------- ehyb_spmm
SPMM_PATHS = [("spmm", p[0], p[1], p[2], p[3], lambda plan, n, t=p[4]: t(plan, n)) for p in S.PATHS] + \
             [("panel", p[0], p[1], p[2], False, lambda plan, n, t=p[5]: t(plan)) for p in SP.PATHS]
# graded-sym and wide-v run on every one of them: both keep a matrix that is symmetric in value symmetric, and no path here pairs
# by accident, so `taken` holds throughout and is asserted.


def _int_case(E, O, which, gen, cfg, sym, k):
    return S.IntCase(E, O, gen, cfg, symmetric=sym, k=k) if which == "spmm" else SP.IntCase(E, gen, cfg, k=k)


@pytest.mark.parametrize("which,name,gen,kw,sym,taken", SPMM_PATHS, ids=[f"{p[0]}-{p[1]}" for p in SPMM_PATHS])
def test_range_spmm(E, O, gpu, which, name, gen, kw, sym, taken):
    """Per column: the matrix as it is, column j of X scaled by 2^e_j -- one call carries a subnormal column (2^-1074) beside a
    near-overflow one (2^940), so a partial sum that reaches another column shows; k = 4 and k = 5 (two passes), both walks.
    Then graded-sym and wide-v values of the same pattern, k = 4 columns of their own x."""
    cfg = E.make_config(**kw)
    c = _int_case(E, O, which, gen, cfg, sym, 5)
    plan = E.Plan(c.m, cfg)
    assert taken(plan, c.n), (name, plan.stats)
    Xs, Ys = columns_scaled(c.X, c.Y)
    assert {-1074, 0, 940} <= set(COLUMN_EXPONENTS[:4])
    for k in (4, 5):
        for walk in (0, 1):
            Y = S.spmm(E, plan, Xs[:k], walk=walk)
            for j in range(k):
                assert_exact(Y[j], Ys[j], f"{name} per-column k={k} walk={walk} column {j} (2^{COLUMN_EXPONENTS[j]})")
    plan.destroy()
    Vi = c.m.V.copy()
    for fam in ("graded-sym", "wide-v"):
        cols = [family(fam, c.n, c.m.I, c.m.J, Vi, c.X[j], c.Y[j], symmetric=sym, x_salt=j) for j in range(4)]
        assert all(np.array_equal(col[0], cols[0][0]) for col in cols)
        c.m.V[:] = cols[0][0]
        plan = E.Plan(c.m, cfg)
        c.m.V[:] = Vi
        assert taken(plan, c.n), (name, fam, plan.stats)
        X2, Y2 = np.stack([col[1] for col in cols]), np.stack([col[2] for col in cols])
        for walk in (0, 1):
            Y = S.spmm(E, plan, X2, walk=walk)
            for j in range(4):
                assert_exact(Y[j], Y2[j], f"{name} {fam} k=4 walk={walk} column {j}")
        plan.destroy()


# ---------------------------------------------------------------------------------------------- refill
@pytest.mark.parametrize("name,gen,kw,sym", REFILL_PLANS, ids=[p[0] for p in REFILL_PLANS])
@pytest.mark.parametrize("how", ["host", "device"])
def test_range_refill(E, O, gpu, name, gen, kw, sym, how):
    """A plan built from integer values, refilled with wide-v and then with low-v values of the same pattern -- from the host in
    reordered order, or from the device in the caller's order with entry_order: every mantissa bit and every subnormal must
    arrive.  Each result is the exact product and bit-equal to a plan built from those values."""
    c, cfg = path_case(E, O, "refill-" + name, gen, kw, sym, extra=dict(value_map=1))
    plan = E.Plan(c.m, cfg)
    assert_exact(multiply(E, plan, c.xp), c.y_ref_p, f"{name} before the refill")
    order = E.entry_order(c.rp0, c.perm)
    for fam in ("wide-v", "low-v"):
        V2, x2, y2 = family_of(c, fam, sym)
        if how == "host":
            plan.set_values(V2)
        else:
            V0 = np.empty_like(V2)
            V0[order] = V2                              # the caller's order: V0[order[k]] is entry k of the reordered matrix
            _device_set_values(plan, V0, order)
        y = multiply(E, plan, x2)
        assert_exact(y, y2, f"{name}/{how} after the {fam} refill")
        if not is_direct(plan, c.n):
            assert_exact(multiply(E, plan, x2, phases=(1, 2)), y2, f"{name}/{how} after the {fam} refill, phases 1+2")
        c.m.V[:] = V2
        try:
            fresh = E.Plan(c.m, cfg)
        finally:
            c.m.V[:] = c.Vi
        assert np.array_equal(multiply(E, fresh, x2), y)
        fresh.destroy()
    plan.destroy()


def test_refill_with_a_pair_that_differs_in_the_subnormals_is_refused(E, O, gpu):
    """a_ij = 3 * 2^-1074 and a_ji = 5 * 2^-1074 are two different numbers: a refill that flushed them to zero before comparing
    would take them for a pair and multiply wrongly.  It must be refused with code 1 and leave the plan as it was."""
    name, gen, kw, sym = REFILL_PLANS[1]
    assert name == "sym-pairs"
    c, cfg = path_case(E, O, "refill-" + name, gen, kw, sym, extra=dict(value_map=1))
    plan = E.Plan(c.m, cfg)
    V2, x2, y2 = family_of(c, "low-v", sym)
    plan.set_values(V2)                                 # an accepted refill: every pair equal, all of it subnormal
    assert_exact(multiply(E, plan, x2), y2, "low-v refill")
    src, src2 = plan.array("ell_src"), plan.array("ell_src2")
    paired = np.flatnonzero((src2 >= 0) & (src2 != src))
    assert len(paired) > 0
    a, b = int(src[paired[len(paired) // 2]]), int(src2[paired[len(paired) // 2]])
    assert (c.m.I[a], c.m.J[a]) == (c.m.J[b], c.m.I[b]) and V2[a] == V2[b]
    V3 = V2.copy()
    V3[a], V3[b] = np.ldexp(3.0, -1074), np.ldexp(5.0, -1074)
    assert V3[a] != V3[b] and V3[a] > 0
    with pytest.raises(E.EhybError) as ei:
        plan.set_values(V3)
    assert ei.value.code == 1
    assert_exact(multiply(E, plan, x2), y2, "after the refused refill")
    plan.destroy()


# ---------------------------------------------------------------------------------------------- ehyb_scatter_add / ehyb_gather
N_DST = 100_000
N_SRC = 1_000_003            # not a multiple of 1024 (a workgroup's share), nor of 4 (a thread's)


class DeviceInts:
    def __init__(self, lib, a):
        self.lib, self.p = lib, C.c_void_p()
        a = np.ascontiguousarray(a, dtype=np.int32)
        assert lib.ehyb_dev_alloc(a.nbytes, C.byref(self.p)) == 0
        assert lib.ehyb_h2d(self.p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0

    def free(self):
        self.lib.ehyb_dev_free(self.p)


def _indices(rng):
    """Half of the entries fall on 64 hot destinations (thousands of adds to one address), the rest anywhere; some
    destinations get nothing."""
    hot = rng.choice(N_DST, 64, replace=False)
    idx = np.where(rng.random(N_SRC) < 0.5, hot[rng.integers(0, 64, N_SRC)], rng.integers(0, N_DST, N_SRC)).astype(np.int32)
    idx[-3:] = [N_DST - 1, 0, N_DST - 1]                 # the last, short thread reaches both ends
    assert idx.min() >= 0 and idx.max() < N_DST and N_SRC % 1024 and N_SRC % 4
    assert np.bincount(idx, minlength=N_DST).max() > 5000 and (np.bincount(idx, minlength=N_DST) == 0).any()
    return idx


# exponent per destination: everything subnormal / near the top (2^40 * 2^982 < 2^1023) / graded over the whole range
SCATTER = {"low": lambda: np.full(N_DST, -1074), "high": lambda: np.full(N_DST, 982), "graded": lambda: row_exponents(N_DST, -1074, 982)}


@pytest.mark.parametrize("fam", list(SCATTER))
def test_scatter_add_is_exact(E, gpu, fam):
    """y[idx[i]] += src[i] with integer multiples of one unit 2^e per destination: every partial sum is exact, so the result is
    the int64 accumulation scaled, in whatever order the global fp64 atomics land."""
    lib = E.host._lib.load()
    rng = np.random.default_rng(5)
    idx = _indices(rng)
    src_i = rng.integers(-(1 << 19), 1 << 19, N_SRC) * 2 + 1              # odd, |.| < 2^20: a million of them stay below 2^40
    y0_i = rng.integers(-(1 << 30), 1 << 30, N_DST)
    acc = y0_i.copy()
    np.add.at(acc, idx, src_i)
    mag = np.abs(y0_i)
    np.add.at(mag, idx, np.abs(src_i))
    e = SCATTER[fam]().astype(np.int64)
    assert mag.max() < 2 ** 40 and e.min() >= -1074 and e.max() + 40 <= 1023
    src, y0, y_ref = np.ldexp(src_i.astype(np.float64), e[idx]), np.ldexp(y0_i.astype(np.float64), e), np.ldexp(acc.astype(np.float64), e)
    assert np.isfinite(y_ref).all() and np.array_equal(np.ldexp(np.ldexp(src, -(e[idx] // 2)), -(e[idx] - e[idx] // 2)), src_i)
    dy, ds, di = E.DeviceBuffer(N_DST).upload(y0), E.DeviceBuffer(N_SRC).upload(src), DeviceInts(lib, idx)
    try:
        assert lib.ehyb_scatter_add(C.c_void_p(dy.ptr), di.p, C.c_void_p(ds.ptr), N_SRC, None) == 0
        _sync(E)
        assert_exact(dy.download(), y_ref, f"scatter-add {fam}")
    finally:
        dy.free(), ds.free(), di.free()


def test_gather_is_bit_equal(E, gpu):
    """dst[i] = src[idx[i]]: 52-bit values over the whole exponent range, subnormals, both zeros, infinities and NaN payloads
    among them, must arrive bit for bit."""
    lib = E.host._lib.load()
    rng = np.random.default_rng(6)
    idx = _indices(rng)
    h = _hash(np.arange(N_DST), np.zeros(N_DST, dtype=np.int64), 0x6A7)
    src = np.ldexp(odd_integers(h, 52).astype(np.float64), row_exponents(N_DST, -1074, 970))
    src[:6] = [0.0, -0.0, np.inf, -np.inf, np.ldexp(1.0, -1074), -np.ldexp(3.0, -1074)]
    bits = src.view(np.uint64).copy()
    bits[6], bits[7] = 0x7FF8000000000123, 0xFFF0000000000001               # a quiet NaN with a payload, a signalling NaN
    src = bits.view(np.float64)
    idx[:8] = np.arange(8)
    dsrc, ddst, di = E.DeviceBuffer(N_DST).upload(src), E.DeviceBuffer(N_SRC + 8).upload(np.full(N_SRC + 8, -7.0)), DeviceInts(lib, idx)
    try:
        assert lib.ehyb_gather(C.c_void_p(dsrc.ptr), di.p, C.c_void_p(ddst.ptr), N_SRC, None) == 0
        _sync(E)
        out = ddst.download()
        assert np.array_equal(out[:N_SRC].view(np.uint64), bits[idx]), "a gathered value changed a bit"
        assert np.array_equal(out[N_SRC:], np.full(8, -7.0)), "written past the end of the list"
    finally:
        dsrc.free(), ddst.free(), di.free()
