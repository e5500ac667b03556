"""cfg.val_f32 on the host: the fp32 value streams ehyb_plan_upload would send (ehyb_plan_device_values_f32), their size
(ehyb_plan_device_value_bytes), and everything that must NOT change -- the host arrays, the stats, the plan files.  CPU only:
every call here works on a plan that was never uploaded."""
import numpy as np
import pytest

from test_gpu_exact import PATHS, RMAT14
from val_f32_cases import FALLBACK_MAX, FEM_INLINE_SYM, FUZZ_SEEDS, SPECIALS, fuzz_case_f32, same_bits_f32, special_values, window_arm

_BY_NAME = {p[0]: p for p in PATHS}
# FEM with plain storage (a residual of its own; one that rides inline behind the slabs' pairs), FEM with symmetric pairs, R-MAT
# with split rows in CSR segments
PLANS = ["refwindow-t256-lds1024", "halo-t1024-lds20480", "sym-fem-3dof", "csr-split-16"]


def _plan_pair(E, name, **more):
    """(matrix, val_f32 plan, fp64 plan) of a named path, the matrix filled with the special values"""
    _, gen, kw, sym, _ = _BY_NAME[name]
    cfg1, cfg0 = E.make_config(val_f32=1, **kw, **more), E.make_config(**kw, **more)
    assert cfg1.val_f32 == 1 and cfg0.val_f32 == 0
    m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg1)
    m.V[:] = special_values(m.I, m.J, sym)
    m.reorder(cfg1)
    return m, E.Plan(m, cfg1, upload=False), E.Plan(m, cfg0, upload=False)


def test_make_config_keeps_the_knob_and_the_size(E):
    import ctypes as C

    assert C.sizeof(E.host.Config) == 260
    assert E.make_config().val_f32 == 0 and E.make_config(val_f32=1).val_f32 == 1 and E.make_config(val_f32=7).val_f32 == 0
    assert not any(E.make_config(val_f32=1).reserved)


@pytest.mark.parametrize("name", PLANS)
def test_rounding_bytes_and_host_form(E, name):
    m, p32, p64 = _plan_pair(E, name)
    st = p32.stats
    ell, er = p32.array("ell_val"), p32.array("er_val")
    # (inline residual pairs sit behind their slab's ELL pairs in the same stream: stats count them apart)
    assert len(ell) == st["size_block_ell"] + st["er_inline"] and st["size_block_ell"] > 0
    assert (st["er_inline"] > 0) == (name == "halo-t1024-lds20480")
    if name == "csr-split-16":
        assert len(er) > 1000
    # ---- rounding: what numpy's astype(float32) gives, bit for bit
    for stream, host in (("ell_val", ell), ("er_val", er)):
        got = p32.device_values_f32(stream)
        assert len(got) == len(host) and same_bits_f32(got, host), (name, stream)
        present = [bool(np.isnan(host).any()) if np.isnan(s) else bool((host == s).any()) for s in SPECIALS]
        ties = (np.abs(host) >= 2.0 ** 24) & (np.abs(host) < 2.0 ** 25) & (np.mod(np.abs(host), 2) == 1)
        if len(host) > 1000:
            assert all(present) and ties.sum() > len(host) // 4, (name, stream, present)
            with np.errstate(over="ignore", invalid="ignore"):
                assert (np.abs(got[ties].astype(np.float64) - host[ties]) == 1).all()           # every tie moved, by one
            assert (got[host == SPECIALS[0]] == np.float32(SPECIALS[0])).all() and SPECIALS[0] < np.finfo(np.float32).tiny
            assert (got[host == SPECIALS[1]] == 0).all()
            assert (got[host == SPECIALS[2]] == np.inf).all() and (got[host == SPECIALS[3]] == -np.inf).all()
    with pytest.raises(E.EhybError):
        p64.device_values_f32("ell_val")               # an fp64 plan has no fp32 stream
    # ---- bytes
    assert p32.device_value_bytes == (4 * (st["size_block_ell"] + st["er_inline"]), 4 * len(er))
    assert p64.device_value_bytes == (8 * (st["size_block_ell"] + st["er_inline"]), 8 * len(er))
    # ---- the host form and the stats do not know the knob
    assert p32.stats == p64.stats
    for arr in E.host.ARRAYS:
        a, b = p32.array(arr), p64.array(arr)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, arr)
    # ---- width
    assert p32.spmm_max_k == 1 and p64.spmm_max_k >= 1


def test_resident_bytes_of_a_plan_that_fits_the_cache_halve(E):
    m, p32, p64 = _plan_pair(E, "sym-fem-3dof")
    assert p64.stats["bytes_format_ell"] < (256 << 20)
    assert p64.resident_bytes == 8 * p64.stats["size_block_ell"]        # fits: every slab is read with plain loads
    assert 2 * p32.resident_bytes == p64.resident_bytes


def test_size_rules_use_the_device_bytes(E):
    """A stream of 300 MB in fp64 does not fit the Infinity Cache beside the plain bytes, the same stream in fp32 does: the
    fp64 plan pins a share of its slabs, the val_f32 plan all of them (ehyb_plan_resident_bytes, 8 B per pair and lane)."""
    kw = dict(sym_pairs=1)
    cfg1, cfg0 = E.make_config(val_f32=1, **kw), E.make_config(**kw)
    m = E.Matrix.generate("fem3d", 599997, 3, 60, 60, 13500, 1, 1, cfg=cfg0)
    m.reorder(cfg0)
    p32, p64 = E.Plan(m, cfg1, upload=False), E.Plan(m, cfg0, upload=False)
    st = p64.stats
    value = 8 * st["size_block_ell"]
    assert st["bytes_format_ell"] > (256 << 20) > st["bytes_format_ell"] - value // 2, st
    assert p64.resident_bytes < value
    assert p32.resident_bytes == value // 2


def test_plan_cache_round_trip_keeps_the_knob(E, tmp_path):
    m, p32, p64 = _plan_pair(E, "csr-split-16")
    path = tmp_path / "f32.plan"
    p32.save(path, m.reorder_list)
    back, perm = E.Plan.load(path, upload=False)
    assert back.device_value_bytes == p32.device_value_bytes and back.spmm_max_k == 1
    for stream in ("ell_val", "er_val"):
        assert np.array_equal(back.device_values_f32(stream).view(np.uint32), p32.device_values_f32(stream).view(np.uint32))
    # an fp64 plan comes back an fp64 plan, and the two files differ in the knob's word alone
    path0 = tmp_path / "f64.plan"
    p64.save(path0, m.reorder_list)
    back0, _ = E.Plan.load(path0, upload=False)
    assert back0.device_value_bytes == p64.device_value_bytes
    a, b = np.fromfile(path, dtype=np.uint8), np.fromfile(path0, dtype=np.uint8)
    assert len(a) == len(b) and (a != b).sum() == 1


def test_panel_form_is_refused_at_upload_without_a_device(E):
    kw = dict(er_mode=2, fuse_er=2, lds_doubles=512, er_panel_cols=512, er_block_rows=300)
    cfg = E.make_config(val_f32=1, **kw)
    m = E.Matrix.generate(RMAT14[0], *RMAT14[1], cfg=cfg)
    m.reorder(cfg)
    plan = E.Plan(m, cfg, upload=False)
    assert plan.stats["er_partials"] > 0
    with pytest.raises(E.EhybError) as ei:
        plan.upload()
    assert ei.value.code == 1 and "val_f32" in str(ei.value) and "panel" in str(ei.value)


# ------------------------------------------------------------------ what the fuzz seeds of test_gpu_val_f32.py reach
def test_what_the_random_configurations_reach_with_val_f32(E, O):
    """From host-only plans of the forty seeds: ten of the twelve ehyb_ell_f32_kernel<THREADS, INLINE_ER, SYM> -- all but an inline
    residual together with symmetric pairs at 512 and 1024 threads (test_inline_residual_with_symmetric_pairs_f32 has those) --,
    split residual rows, the direct shape, matrices of up to five rows and without an entry; and how many seeds had to leave
    the panel form their draw asked for."""
    arms, fell_back, split, tiny, empty, direct = set(), [], 0, 0, 0, 0
    for seed in FUZZ_SEEDS:
        m, cfg, kw, x, y_ref, fb = fuzz_case_f32(E, O, seed)
        plan = E.Plan(m, cfg, upload=False)
        st = plan.stats
        assert cfg.val_f32 == 1 and st["er_partials"] == 0 and st["nnz_ell"] + st["nnz_er"] == m.nnz, (seed, kw)
        if fb:
            fell_back.append(seed)
        arms.add(window_arm(cfg, st))
        split += bool((plan.array("er_seg_row") < 0).any())
        tiny += m.n <= 5
        empty += m.nnz == 0
        direct += m.nnz > 0 and st["nnz_ell"] == 0
        plan.destroy()
    print(f"arms {sorted(a for a in arms if a)}, fell back {fell_back}, split rows in {split}, n <= 5 in {tiny}, empty {empty}, direct {direct}")
    assert len(fell_back) <= FALLBACK_MAX, fell_back
    want = {(256, i, s) for i in (False, True) for s in (False, True)} | {(t, i, s) for t in (512, 1024) for i, s in ((False, False), (False, True), (True, False))}
    assert len(want) == 10 and want <= arms, sorted(want - arms)
    assert split >= 1 and tiny >= 4 and empty == 6 and direct >= 1


@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_the_named_plan_has_an_inline_residual_and_symmetric_pairs(E, threads):
    """FEM_INLINE_SYM: what the named arms of test_gpu_val_f32.py launch, from the stats of a host-only plan"""
    from test_gpu_exact import FEM

    for triples in (1, 2):
        cfg = E.make_config(val_f32=1, threads=threads, ell_triples=triples, **FEM_INLINE_SYM)
        m = E.Matrix.generate(FEM[0], *FEM[1], cfg=cfg)
        m.reorder(cfg)
        plan = E.Plan(m, cfg, upload=False)
        st = plan.stats
        assert window_arm(cfg, st) == (threads, True, True) and st["sym_pairs"] > 0.25 * st["nnz"] and st["er_partials"] == 0, st
        plan.destroy()
