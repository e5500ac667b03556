"""The fixed set of slabs the window kernel reads with plain loads (cfg.ell_nt = 4 spread, 5 block; cfg.ell_keep), so that the
Infinity Cache keeps it from one multiply to the next: the rule itself through its C export, the byte count of plans built on the
host, and the automatic share against the size of the cache.  No device needed."""
import numpy as np
import pytest

WALK_END, SPREAD, BLOCK = 0, 1, 2
KEEPS = (0, 1, 300, 512, 1023, 1024)
CACHE = 256 << 20


def _marks(lib, n, keep1024, shape):
    return np.array([lib.ehyb_ell_slab_resident(i, n, keep1024, shape) for i in range(n)], dtype=bool)


@pytest.mark.parametrize("keep1024", KEEPS)
def test_spread_marks_the_floor_of_the_share(E, keep1024):
    """Bresenham over the slab index: exactly floor(n * keep1024 / 1024) slabs of n -- never more than the budget --, evenly:
    every prefix of i slabs holds floor(i * keep1024 / 1024) of them."""
    lib = E.host._lib.load()
    for n in range(1, 201):
        m = _marks(lib, n, keep1024, SPREAD)
        assert m.sum() == n * keep1024 // 1024, (n, keep1024)
        assert np.array_equal(np.cumsum(m), np.arange(1, n + 1) * keep1024 // 1024)
        if keep1024 == 0:
            assert not m.any()
        if keep1024 == 1024:
            assert m.all()


@pytest.mark.parametrize("keep1024", KEEPS)
def test_block_marks_the_first_slabs(E, keep1024):
    lib = E.host._lib.load()
    for n in range(1, 201):
        m = _marks(lib, n, keep1024, BLOCK)
        k = n * keep1024 // 1024
        assert m[:k].all() and not m[k:].any(), (n, keep1024)


@pytest.mark.parametrize("shape", [SPREAD, BLOCK])
@pytest.mark.parametrize("keep1024", KEEPS)
def test_the_set_does_not_depend_on_the_walk(E, shape, keep1024):
    """The kernel asks about slab `reverse ? n - 1 - p : p` at walk position p: both directions mark the same slabs."""
    lib = E.host._lib.load()
    for n in range(1, 201):
        sets = []
        for reverse in (0, 1):
            slabs = [n - 1 - p if reverse else p for p in range(n)]
            sets.append({s for s in slabs if lib.ehyb_ell_slab_resident(s, n, keep1024, shape)})
        assert sets[0] == sets[1], (n, keep1024)


def test_walk_end_is_the_old_position_rule(E):
    """cfg.ell_nt = 3 keeps its rule: walk positions below ceil(n * (1024 - keep1024) / 1024) carry the hint, the rest do not."""
    lib = E.host._lib.load()
    for n in range(1, 201):
        for keep1024 in KEEPS:
            nt_end = -(-n * (1024 - keep1024) // 1024)
            assert np.array_equal(_marks(lib, n, keep1024, WALK_END), np.arange(n) >= nt_end)


def test_automatic_share_fits_the_cache(E):
    """(256 MiB - the bytes a launch reads and writes with plain accesses) x a safety factor <= 1, over the value stream's bytes,
    capped at all of it; a stream that fits whole is kept whole."""
    lib = E.host._lib.load()
    assert lib.ehyb_ell_auto_keep1024(100 << 20, 50 << 20) == 1024
    assert lib.ehyb_ell_auto_keep1024(CACHE - 1000, 1000) == 1024
    for value in (200 << 20, 380_000_000, 729_000_000, 2_560_000_000, 40 << 30):
        for plain in (0, 1 << 20, 59_000_000, 200 << 20, CACHE, 300 << 20):
            k = lib.ehyb_ell_auto_keep1024(value, plain)
            assert 0 <= k <= 1024
            if value + plain > CACHE:
                assert value * k // 1024 + plain <= max(CACHE, plain), (value, plain, k)
    # the headline's sizes (audikw_1-like, symmetric pairs: 380 MB of values beside 59 MB): a real share, not a token one
    assert lib.ehyb_ell_auto_keep1024(380_000_000, 59_000_000) >= 400


def _host_plan(E, sym, **kw):
    import bench as B

    gen, gargs, _ = B.WORKLOADS["audikw_1-like"]
    gargs = (90000, gargs[1], 30, 30) + tuple(gargs[4:])         # the bench's generator, scaled down
    cfg = E.make_config(partitioner=B.partitioner_for(E, gen), lds_doubles=4096, **(dict(sym_pairs=1) if sym else {}), **kw)
    m = E.Matrix.generate(gen, *gargs, cfg=cfg)
    m.reorder(cfg)
    return E.Plan(m, cfg, upload=False), cfg


def _walk(lib, plan, keep1024, shape):
    """-> (resident bytes, slabs marked per segment, slabs per segment) by the rule over slab_meta, in numpy"""
    meta = plan.array("slab_meta").reshape(-1, 4)
    segs = plan.array("segs").reshape(-1, 8)
    pairs = (meta[:, 3] >> 16).astype(np.int64)
    total, marked, sizes = 0, [], []
    for sg in segs:
        sb, se = int(sg[1]), int(sg[2])
        m = _marks(lib, se - sb, keep1024, shape)
        total += int(pairs[sb:se][m].sum()) * 64 * 16
        marked.append(int(m.sum()))
        sizes.append(se - sb)
    return total, np.array(marked), np.array(sizes)


@pytest.mark.parametrize("sym", [True, False], ids=["symmetric-pairs", "plain"])
@pytest.mark.parametrize("ell_nt,shape", [(4, SPREAD), (5, BLOCK)])
@pytest.mark.parametrize("ell_keep", [1, 400, 1000])
def test_resident_bytes_of_host_plans(E, sym, ell_nt, shape, ell_keep):
    lib = E.host._lib.load()
    plan, cfg = _host_plan(E, sym, ell_nt=ell_nt, ell_keep=ell_keep)
    try:
        assert (cfg.ell_nt, cfg.ell_keep) == (ell_nt, ell_keep)
        keep1024 = ell_keep * 1024 // 1000
        total, marked, sizes = _walk(lib, plan, keep1024, shape)
        assert np.array_equal(marked, sizes * keep1024 // 1024)
        assert plan.resident_bytes == total
        st = plan.stats
        if ell_keep == 1000:
            assert total == 8 * st["size_block_ell"]
    finally:
        plan.destroy()


@pytest.mark.parametrize("sym", [True, False], ids=["symmetric-pairs", "plain"])
def test_automatic_share_of_a_host_plan(E, sym):
    """ell_nt = 4 forced, ell_keep automatic: the pinned bytes together with what the launch reads and writes with plain accesses
    (everything of bytes_format_ell that is not the value stream) stay within 256 MiB."""
    lib = E.host._lib.load()
    plan, cfg = _host_plan(E, sym, ell_nt=4)
    try:
        assert (cfg.ell_nt, cfg.ell_keep) == (4, 0)
        st = plan.stats
        value = 8 * st["size_block_ell"]
        plain = st["bytes_format_ell"] - value
        assert plain > 0
        keep1024 = lib.ehyb_ell_auto_keep1024(value, plain)
        total, marked, sizes = _walk(lib, plan, keep1024, SPREAD)
        assert np.array_equal(marked, sizes * keep1024 // 1024)
        assert plan.resident_bytes == total
        assert total + plain <= CACHE
    finally:
        plan.destroy()
