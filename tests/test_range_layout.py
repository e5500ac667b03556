"""The fuzz cases of test_exact_layout.py over the whole fp64 range and mantissa width (range_cases.py): the integer case of every
seed scaled by powers of two -- per matrix, per row, symmetrically -- into the subnormals and up to 2^1023, and redrawn with
as many mantissa bits as the longest row leaves room for.  Every product still has one correct fp64 value whatever the order
of summation, so the layout walked the way the kernels index it (oracle.walk_plan) must give it bit for bit, every row written
once.  This pins the host builders, the plan cache and the reference on these inputs before any GPU time is spent
(test_gpu_range.py runs the same families on the device), and the family builder's own preconditions."""
import struct

import numpy as np
import pytest

from exact_cases import assert_exact, integer_values, integer_x
from fuzz_cases import build
from range_cases import COLUMN_EXPONENTS, FAMILIES, columns_scaled, family, odd_integers, row_exponents, wide_bits

SEEDS = range(48)
_cases = {}
_stats = {}


def fuzz_case(E, O, seed):
    """The exact fuzz case of `seed` in the plan's numbering -> (matrix, cfg, kw, integer V, x, y, symmetric in value);
    built once per seed (the matrix is shared: every user sets m.V itself)."""
    if seed not in _cases:
        _cases.clear()
        m, cfg, kw, x, y_ref, scale = build(E, O, seed, exact=True)
        A = m.to_scipy()
        _cases[seed] = (m, cfg, kw, m.V.copy(), E.vector_reorder(x, m.reorder_list), E.vector_reorder(y_ref, m.reorder_list),
                        m.nnz > 0 and abs(A - A.T).nnz == 0)
    return _cases[seed]


def family_plan(E, O, seed, fam):
    m, cfg, kw, Vi, xp, yp, sym = fuzz_case(E, O, seed)
    V2, x2, y2 = family(fam, m.n, m.I, m.J, Vi, xp, yp, symmetric=sym)
    m.V[:] = V2
    plan = E.Plan(m, cfg, upload=False)
    m.V[:] = Vi
    _stats[seed, fam] = plan.stats
    return plan, m, kw, V2, x2, y2


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("seed", SEEDS)
def test_range_layout_walk(E, O, seed, fam):
    plan, m, kw, V2, x2, y2 = family_plan(E, O, seed, fam)
    if m.nnz:
        assert np.array_equal(O.spmv_coo(m.n, m.I, m.J, V2, x2), y2), "the fp64 oracle is not exact on a scaled integer input"
    yp, written = O.walk_plan(plan, x2)
    assert (written == 1).all(), (fam, kw)
    assert_exact(yp, y2, f"{fam} {kw}")
    st = plan.stats
    assert st["nnz_ell"] + st["nnz_er"] == m.nnz, kw


def test_every_family_meets_pairs_partial_sums_and_an_inline_residual(E, O):
    """The seeds above must take every family through symmetric pair storage, a panel-form residual and an inline residual, or
    the walks would not exercise them on these values (graded-rows and wide-v on a matrix not symmetric in value keep only
    accidentally equal mirror pairs)."""
    met = {fam: np.zeros(3, dtype=np.int64) for fam in FAMILIES}
    for seed in SEEDS:
        for fam in FAMILIES:
            st = _stats[seed, fam] if (seed, fam) in _stats else family_plan(E, O, seed, fam)[0].stats    # (kept by the walks above)
            met[fam] += [st["sym_pairs"] > 0, st["er_partials"] > 0, st["er_inline"] > 0]
    for fam, counts in met.items():
        assert (counts >= 1).all(), (fam, dict(zip(("sym_pairs", "er_partials", "er_inline"), counts.tolist())))


@pytest.mark.parametrize("fam", ["wide-v", "low-v"])
@pytest.mark.parametrize("seed", range(200, 212))
def test_range_plan_cache_round_trip(E, O, seed, fam, tmp_path):
    """ehyb_plan_save / ehyb_plan_load keep every mantissa bit and every subnormal of the value streams."""
    plan, m, kw, V2, x2, y2 = family_plan(E, O, seed, fam)
    path = tmp_path / "p.cache"
    plan.save(path, reorder_list=m.reorder_list, key=777)
    back, perm = E.Plan.load(path, key=777, upload=False)
    assert np.array_equal(perm, m.reorder_list), kw
    for name in ("ell_val", "er_val", "pb_val"):
        a, b = plan.array(name), back.array(name)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, kw)
    if m.nnz:
        stored = np.concatenate([np.abs(back.array(name)) for name in ("ell_val", "er_val", "pb_val")])
        assert np.isin(np.abs(V2), stored).all(), "a value of the family is in no value stream"
    yp, written = O.walk_plan(back, x2)
    assert (written == 1).all(), kw
    assert_exact(yp, y2, f"{fam} {kw}")


# ---------------------------------------------------------------------------------------------- the family builder
def _ring(n, row_len, x_mag):
    """n rows of row_len entries (+-1..7), integer x of magnitude x_mag, and the int64 product."""
    I = np.repeat(np.arange(n), row_len)
    J = (I + np.tile(np.arange(row_len), n)) % n
    V = integer_values(I, J, False)
    x = np.full(n, float(x_mag))
    y = np.zeros(n)
    np.add.at(y, I, V * x[J])
    return n, I, J, V, x, y


def test_families_are_what_the_table_says():
    n, I, J, V, x, y = _ring(40, 5, 2 ** 25 + 1)
    sub = 2.0 ** -1022
    V2, x2, y2 = family("low", n, I, J, V, x, y)
    assert (np.abs(V2) >= sub).all() and (np.abs(x2) >= sub).all() and (np.abs(V2[:, None] * x2[None, :4]) < sub).all()
    assert np.array_equal(y2, np.ldexp(y, -1074)) and (np.abs(y2) < sub).all() and (y2 != 0).any()
    V2, x2, y2 = family("low-x", n, I, J, V, x, y)
    assert np.array_equal(V2, V) and (np.abs(x2) < sub).all() and (x2 != 0).all()
    V2, x2, y2 = family("low-v", n, I, J, V, x, y)
    assert np.array_equal(x2, x) and (np.abs(V2) < sub).all() and (V2 != 0).all()
    V2, x2, y2 = family("high", n, I, J, V, x, y)
    assert np.isfinite(y2).all() and np.array_equal(y2, np.ldexp(y, 971)) and np.abs(y2).max() > 2.0 ** 990
    r = row_exponents(n, -480, 480)
    assert r.min() >= -480 and r.max() <= 480 and len(np.unique(r)) > n // 2
    V2, x2, y2 = family("graded-sym", n, I, J, V, x, y)
    assert np.array_equal(V2, np.ldexp(V, r[I] + r[J])) and np.array_equal(x2, np.ldexp(x, -r)) and np.array_equal(y2, np.ldexp(y, r))
    V2, x2, y2 = family("graded-low", n, I, J, V, x, y)
    assert (np.abs(y2[y2 != 0]) < sub).any() and (np.abs(y2) >= sub).any(), "subnormal and normal rows side by side"
    b = wide_bits(I, n)
    assert b == 51 - 3
    V2, x2, y2 = family("wide-v", n, I, J, V, x, y)
    assert set(np.abs(x2)) == {1.0} and (np.abs(V2) >= 2.0 ** (b - 1)).all() and (np.abs(V2) < 2.0 ** b).all() and (V2 % 2 == 1).all()
    assert np.bitwise_or.reduce(np.abs(V2).astype(np.int64)) == (1 << b) - 1, "every one of the b mantissa bits is used"
    assert not np.array_equal(V2.astype(np.float32).astype(np.float64), V2)
    V2, x2, y2 = family("wide-x", n, I, J, V, x, y)
    assert np.array_equal(V2, V) and (np.abs(x2) >= 2.0 ** (b - 4)).all() and (np.abs(x2) < 2.0 ** (b - 3)).all() and (x2 % 2 == 1).all()
    ref = np.zeros(n, dtype=np.int64)
    np.add.at(ref, I, V2.astype(np.int64) * x2.astype(np.int64)[J])
    assert np.array_equal(y2, ref.astype(np.float64))


def test_wide_v_stays_symmetric_where_the_case_is():
    n = 30
    I, J = np.nonzero(np.ones((n, n)))
    V, x = integer_values(I, J, True), integer_x(n, 1)
    y = np.zeros(n)
    np.add.at(y, I, V * x[J])
    for fam in ("wide-v", "graded-sym", "low-v"):
        V2 = family(fam, n, I, J, V, x, y, symmetric=True)[0]
        M = np.zeros((n, n))
        M[I, J] = V2
        assert np.array_equal(M, M.T), fam
    M[I, J] = family("wide-v", n, I, J, V, x, y, symmetric=False)[0]
    assert not np.array_equal(M, M.T)


def test_a_row_too_long_for_the_mantissa_budget_is_refused():
    """2^24 + 1 entries in one row leave 51 - 25 = 26 bits per value and 23 per x of wide-x, which fp32 holds: such a case
    would show nothing.  The builder refuses it; it does not shorten the row or the values."""
    I = np.zeros((1 << 24) + 1, dtype=np.int64)
    with pytest.raises(ValueError, match="longest row"):
        wide_bits(I, 1)
    assert wide_bits(I[:1 << 23], 1) == 28
    J = np.arange(len(I)) % 7
    V = np.ones(len(I))
    x = np.ones(7)
    y = np.array([float(len(I))])
    for fam in ("wide-v", "wide-x"):
        with pytest.raises(ValueError, match="longest row"):
            family(fam, 1, I, J, V, x, y)


def test_preconditions_are_asserted():
    n, I, J, V, x, y = _ring(16, 4, 2 ** 25 + 1)
    with pytest.raises(ValueError, match="unknown family"):
        family("medium", n, I, J, V, x, y)
    with pytest.raises(ValueError, match="not the int64 product"):
        family("low", n, I, J, V, x, y + 1.0)
    with pytest.raises(AssertionError):
        family("low", n, I, J, V + 0.5, x, y)                # not an integer case
    # sum |a x| >= 2^52: no exact product, whatever the scale
    nb, Ib, Jb, Vb, xb, yb = _ring(16, 4, 2 ** 50)
    for fam in ("low", "high", "graded-rows"):
        with pytest.raises(ValueError, match="too large"):
            family(fam, nb, Ib, Jb, Vb, xb, yb)
    # per column: 2^52 * 2^972 reaches 2^1023; 2^-1075 is no fp64 number
    X, Y = np.stack([x, x]), np.stack([y, y])
    with pytest.raises(ValueError, match="leaves the fp64 range"):
        columns_scaled(X, Y, (0, 972))
    with pytest.raises(ValueError, match="leaves the fp64 range"):
        columns_scaled(X, Y, (-1075, 0))
    Xs, Ys = columns_scaled(X, Y, (-1074, 971))
    assert np.array_equal(Ys[0], np.ldexp(y, -1074)) and np.array_equal(Xs[1], np.ldexp(x, 971)) and np.isfinite(Ys).all()
    assert {-1074, 0, 940} <= set(COLUMN_EXPONENTS[:4]) and any(-1074 < e < 940 and e != 0 for e in COLUMN_EXPONENTS[:4])
    assert (odd_integers(np.arange(5, dtype=np.uint64), 52) % 2 != 0).all()


# ---------------------------------------------------------------------------------------------- what the build compiled in
def _code_objects(path):
    """The device code objects of a shared library: every entry of its clang offload bundles -> (target, ELF image)."""
    d = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    at = d.find(magic)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", d, at + len(magic))
        p = at + len(magic) + 8
        for _ in range(count):
            off, size, tl = struct.unpack_from("<QQQ", d, p)
            target = d[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if target.startswith("hip") and size:
                yield target, d[at + off:at + off + size]
        at = d.find(magic, at + 1)


def _kernel_descriptors(elf):
    """Every <kernel>.kd symbol of an amdhsa code object -> (kernel, FLOAT_DENORM_MODE_32, FLOAT_DENORM_MODE_16_64): bits 16-17 and
    18-19 of compute_pgm_rsrc1, byte 48 of the 64-byte kernel descriptor; 3 keeps denormal sources and results, 0 flushes both."""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2
    (shoff,) = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    for s in secs:
        if s[1] != 2:                                     # SHT_SYMTAB
            continue
        names = secs[s[6]][4]
        for k in range(s[5] // 24):
            name_off, _, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, s[4] + k * 24)
            name = elf[names + name_off:elf.index(b"\0", names + name_off)].decode()
            if name.endswith(".kd") and size == 64:
                at = secs[shndx][4] + value - secs[shndx][3]
                (rsrc1,) = struct.unpack_from("<I", elf, at + 48)
                yield name[:-3], (rsrc1 >> 16) & 3, (rsrc1 >> 18) & 3


def test_no_kernel_is_compiled_to_flush_denormals(E):
    """The range contract of ehyb_spmv (include/ehyb.h) is a property of the build too: every kernel of libehyb.so must run with
    both denormal modes of its kernel descriptor at 3 (keep).  -fgpu-flush-denormals-to-zero in HIPFLAGS sets the fp32 mode to 0 and
    leaves fp64 arithmetic alone on gfx950, so no fp64 product shows it; this test does, before it reaches the fp64 mode."""
    lib = E.host._lib.LIB_PATH
    kernels = [kd for target, elf in _code_objects(lib) if target.endswith("gfx950") for kd in _kernel_descriptors(elf)]
    assert len(kernels) >= 100 and any("ehyb_ell_kernel" in k[0] for k in kernels) and any("ehyb_fill_kernel" in k[0] for k in kernels)
    flushing = [k for k in kernels if k[1:] != (3, 3)]
    assert not flushing, f"{len(flushing)} of {len(kernels)} kernels flush denormals, e.g. {flushing[0]}"
