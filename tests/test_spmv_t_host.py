"""The transposed multiply on the CPU: which plans ehyb_spmv_t serves and refuses (ehyb_spmv_t_supported, host-only plans), the
errors that need no device, its kernel table, that the three pinned tables are what they were -- and a CPU walk of the host
arrays (spmv_t_walk.py) that indexes them as the transposed kernels do and must give the exact A^T x on every supported named
path, over the pair form of the column words and over the triple-coded words as ehyb_plan_upload would send them."""
import ctypes as C

import numpy as np
import pytest

from exact_cases import assert_exact, exact_reference, integer_values, integer_x
from spmv_t_cases import ALL_ROWS, EXTRA_PATHS, NAMED, REFUSED, nodes_and_pairs
from spmv_t_walk import walk_plan_t
from test_col_triples import device_cols

ERR_ARG, ERR_STATE = 1, 8

# the supported named paths of test_gpu_exact.PATHS (that module is marked gpu as a whole: restated here, compared there)
FEM = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))
STENCIL = ("stencil2d", (150, 150, 5, 3000, 1))
RMAT11 = ("rmat", (11, 1 << 17, 3))
HOST_PATHS = {
    "refwindow-t256-lds1024": (FEM, dict(window_mode=1, threads=256, lds_doubles=1024)),
    "halo-t512-lds64": (STENCIL, dict(window_mode=2, threads=512, lds_doubles=64)),
    "halo-t1024-lds20480": (FEM, dict(window_mode=2, threads=1024, lds_doubles=20480, direct=2)),
    "refwindow-t1024-lds20480": (FEM, dict(window_mode=1, threads=1024, lds_doubles=20480)),
    "inline-residual": (FEM, dict(window_mode=1, lds_doubles=20480, fuse_er=1)),
    "csr-split-16": (RMAT11, dict(window_mode=1, lds_doubles=256, er_seg_len=16, er_mode=1, fuse_er=2)),
    "csr-split-64": (RMAT11, dict(window_mode=1, lds_doubles=256, er_seg_len=64, er_mode=1, fuse_er=2)),
    "direct-rmat": (("rmat", (13, 1 << 18, 3)), dict()),
    "direct-fem": (("fem3d", (10974, 3, 62, 59, 250000, 1, 17)), dict()),
    "relative-columns": (("banded", (1024 * 64, 32, 1024)), dict(direct=2)),
}


def host_case(E, gen, kw, rows=None, col_segs=None):
    """-> (matrix with unsymmetric integer values, reordered; host-only plan; integer x; exact A x; exact A^T x), permuted numbering"""
    cfg = E.make_config(**kw)
    m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg)
    m.V[:] = integer_values(m.I, m.J, False)
    m.reorder(cfg)
    if rows == "half":
        pb = m.part_boundary
        rows = (0, int(pb[len(pb) // 2]))
    if col_segs == "half":
        col_segs = np.array([0, m.n // 2 & ~1, m.n], dtype=np.int32)
    plan = E.Plan(m, cfg, rows=rows, upload=False, col_segs=col_segs)
    x = integer_x(m.n, 1)
    return m, plan, x, exact_reference(m.n, m.I, m.J, m.V, x), exact_reference(m.n, m.J, m.I, m.V, x)


def test_the_named_paths_are_the_issue_s_and_cover_the_table(E):
    assert set(HOST_PATHS) == set(NAMED)
    assert set(E.kernel_table_t()) == ALL_ROWS == set().union(*NAMED.values(), *(c[4] for c in EXTRA_PATHS))


@pytest.mark.parametrize("name", sorted(HOST_PATHS))
def test_supported_forms_and_the_cpu_walk(E, name):
    """OK on the host-only plan; the walk of its arrays is the exact transposed product, which differs from the forward one"""
    gen, kw = HOST_PATHS[name]
    m, plan, x, y_fwd, y_t = host_case(E, gen, kw)
    assert plan.spmv_t_supported and plan.spmv_t_refusal == (0, "")
    assert (y_fwd != y_t).sum() > m.n // 2
    assert_exact(walk_plan_t(plan, x), y_t, f"{name}: host words")
    assert_exact(walk_plan_t(plan, x, device=True), y_t, f"{name}: device words")
    assert plan.launched_t() == set()
    plan.destroy()


def test_cpu_walk_over_triple_words_with_one_two_and_six_pairs(E):
    """nodes_and_pairs: coded slabs with pairs % 3 of 0, 1 and 2, odd partition starts"""
    cfg = E.make_config(lds_doubles=1024, direct=2)
    indptr, indices = nodes_and_pairs()
    I = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    m = E.Matrix.from_csr(indptr, indices, integer_values(I, indices, False), cfg)
    m.reorder(cfg)
    plan = E.Plan(m, cfg, upload=False)
    _, dmeta = device_cols(plan)
    coded = (dmeta[:, 3] & 0x40) != 0
    assert set(((dmeta[coded, 3] >> 16) % 3).tolist()) == {0, 1, 2}
    assert (plan.array("part_boundary")[:-1] & 1).any()
    x = integer_x(m.n, 3)
    assert_exact(walk_plan_t(plan, x, device=True), exact_reference(m.n, m.J, m.I, m.V, x), "nodes and pairs")
    plan.destroy()


@pytest.mark.parametrize("name,gen,kw,words", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_forms_are_named(E, name, gen, kw, words):
    m, plan, x, _, _ = host_case(E, gen, kw)
    assert not plan.spmv_t_supported
    rc, msg = plan.spmv_t_refusal
    assert rc == ERR_ARG and words in msg, (name, msg)
    # the multiply itself says the same, before it asks for an upload (pointers that are never followed)
    assert plan.lib.ehyb_spmv_t(plan.h, C.c_void_p(64), C.c_void_p(128), None) == ERR_ARG
    assert words in plan.lib.ehyb_last_error().decode()
    with pytest.raises(E.EhybError) as ei:
        plan.spmv_t(64, 128)
    assert ei.value.code == ERR_ARG and words in str(ei.value)
    plan.destroy()


def test_a_row_range_and_column_segments_are_refused(E):
    _, plan, _, _, _ = host_case(E, FEM, dict(lds_doubles=4096, direct=2), rows="half")
    assert plan.spmv_t_refusal[0] == ERR_ARG and "not over all rows" in plan.spmv_t_refusal[1]
    plan.destroy()
    _, plan, _, _, _ = host_case(E, ("rmat", (14, 1 << 17, 1)), dict(er_mode=1, fuse_er=2, lds_doubles=512, direct=2), col_segs="half")
    assert plan.col_segs == 2
    assert plan.spmv_t_refusal[0] == ERR_ARG and "column segments" in plan.spmv_t_refusal[1], plan.spmv_t_refusal
    plan.destroy()


def test_errors_that_need_no_device(E):
    _, plan, _, _, _ = host_case(E, FEM, dict(lds_doubles=4096, direct=2))
    lib = plan.lib
    assert plan.spmv_t_supported
    assert lib.ehyb_spmv_t(plan.h, C.c_void_p(64), C.c_void_p(128), None) == ERR_STATE       # never uploaded
    assert "not uploaded" in lib.ehyb_last_error().decode()
    assert lib.ehyb_spmv_t(plan.h, C.c_void_p(64), C.c_void_p(64), None) == ERR_ARG           # x == y
    assert lib.ehyb_spmv_t(plan.h, None, C.c_void_p(64), None) == ERR_ARG
    assert lib.ehyb_spmv_t(None, C.c_void_p(64), C.c_void_p(128), None) == ERR_ARG
    assert lib.ehyb_spmv_t_supported(None) == ERR_ARG
    # ehyb_gmres_t: its own argument checks, then the upload
    args = (30, 2, 100, 1e-10, None, None, None)
    assert lib.ehyb_gmres_t(plan.h, None, C.c_void_p(64), C.c_void_p(128), *args) == ERR_STATE
    assert lib.ehyb_gmres_t(plan.h, None, None, C.c_void_p(128), *args) == ERR_ARG
    assert lib.ehyb_gmres_t(plan.h, None, C.c_void_p(64), C.c_void_p(128), 65, 2, 100, 1e-10, None, None, None) == ERR_ARG
    plan.destroy()
    _, sym, _, _, _ = host_case(E, FEM, dict(lds_doubles=4096, sym_pairs=1))
    assert lib.ehyb_gmres_t(sym.h, None, C.c_void_p(64), C.c_void_p(128), *args) == ERR_ARG  # the form, before the upload
    assert "symmetric pair storage" in lib.ehyb_last_error().decode()
    assert lib.ehyb_gmres(sym.h, None, C.c_void_p(64), C.c_void_p(128), *args) == ERR_STATE  # the forward solver takes the form
    sym.destroy()


def test_kernel_table_t_and_the_pinned_tables(E):
    rows = E.kernel_table_t()
    assert len(rows) == 7 == len(set(rows)) and all(len(r) == len(E.KERNEL_TABLE_T) == 3 for r in rows)
    assert E.KERNEL_TABLE_T == ("kind", "threads", "inl")
    assert {r for r in rows if r[0] == 0} == {(0, t, i) for t in (256, 512, 1024) for i in (0, 1)}
    assert [r for r in rows if r[0] == 1] == [(1, 256, 0)]
    lib = E.host._lib.load()
    n = C.c_int(-1)
    few = (C.c_int32 * 6)(*([-7] * 6))
    assert lib.ehyb_debug_kernel_table_t(few, 1, C.byref(n)) == 0 and n.value == 7
    assert tuple(few[:3]) == rows[0] and list(few[3:]) == [-7] * 3
    assert lib.ehyb_debug_kernel_table_t(None, 0, None) == ERR_ARG
    # the three tables of ehyb_debug_kernel_table are what they were: names, fields, row counts, and no fourth table
    assert E.KERNEL_TABLES == {"window": ("threads", "k", "dyn", "stamp", "inl", "sym", "f32"),
                               "panel": ("pass", "threads", "k", "dpp", "probe", "nt"), "er_csr": ("k", "assign", "f32")}
    assert {name: len(E.kernel_table(name)) for name in E.KERNEL_TABLES} == {"window": 96, "panel": 22, "er_csr": 10}
    assert lib.ehyb_debug_kernel_table(3, None, 0, C.byref(n)) == ERR_ARG


def test_the_fuzz_seed_list_is_the_supported_seeds(E, O):
    """at most half of the 40 seeds may be filtered out; the list in spmv_t_cases.py is exactly the seeds a host-only plan supports"""
    from spmv_t_cases import FUZZ_RANGE, FUZZ_REFUSED, FUZZ_SEEDS, fuzz_case

    assert len(FUZZ_RANGE) == 40 and len(FUZZ_SEEDS) >= 20 and sorted(FUZZ_SEEDS + FUZZ_REFUSED) == list(FUZZ_RANGE)
    for seed in FUZZ_RANGE:
        for more in ({}, dict(ell_alternate=1)):
            m, cfg, xp, y_t = fuzz_case(E, O, seed, **more)
            plan = E.Plan(m, cfg, upload=False)
            assert plan.spmv_t_supported == (seed in FUZZ_SEEDS), (seed, more, plan.spmv_t_refusal)
            if plan.spmv_t_supported and not more:
                assert_exact(walk_plan_t(plan, xp, device=True), y_t, f"seed {seed}")
            plan.destroy()
