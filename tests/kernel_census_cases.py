"""The kernel census: cases that together launch EVERY instantiation libehyb.so builds -- the rows of its three kernel tables
(E.kernel_table: "window" 96 rows, "panel" 22, "er_csr" 10) -- against exact products.  Cases only, no tests:
test_kernel_census_host.py proves on the CPU that the rows the cases declare are the tables' rows and that every case's host-only
plan is the plan it claims; test_gpu_kernel_census.py runs each case and compares the plan's launch log (Plan.launched) with the
rows it declares, no more and no fewer.

A case declares its rows from its OWN parameters (workgroup size, walk, inline residual, symmetric pairs, widths), never from the
library's tables: a row someone adds to a table without a case here makes the union differ.

Matrices are those of test_gpu_exact.py (30,000-row FEM, R-MAT 2^11 / 2^13 / 2^14); integer values and x (exact_cases.py), so a
product is one number whatever the order of summation.  One plan with a window of at most 5118 doubles serves K = 1..4.

What a window case must be able to go wrong on (SHOWS), per walk and workgroup size:
  more      some segment has more slabs than the workgroup has waves: the walk iterates (LDS counter) / wraps (round-robin)
  fewer     some segment has fewer: waves find nothing to take
  halo      some window gathers halo columns
  multiseg  some item has more than one segment: a window is re-staged inside a workgroup
The scheduled sizes of these matrices give at most 12 slabs per segment (at least 512 rows per partition of a small matrix with
symmetric pairs, two slabs per item with plain storage), fewer than the 16 waves of 1024 threads; FEM24 is the FEM matrix in 24
partitions sized by the caller (matrixCOO.nParts / vectorCacheSize, the drop-in's hints): one workgroup per partition of 15 to 20
slabs."""
from dataclasses import dataclass, field

import numpy as np

from exact_cases import exact_reference, integer_values, integer_x
from test_gpu_exact import FEM, PANEL_ARMS, RMAT11, RMAT14
from val_f32_cases import FEM_INLINE_SYM

RMAT13D = ("rmat", (13, 1 << 18, 3))  # "direct-rmat" of test_gpu_exact.py
FEM24 = FEM + ((24, 1280),)          # generator, arguments, (nParts, vectorCacheSize) set before the reorder

THREADS = (256, 512, 1024)
LDS_K4 = 5118                        # (20480 * 8 - 16) / (8 * 5118) = 4 columns per pass
SHOWS = ("more", "fewer", "halo", "multiseg")
# cfg fields that change no host array: a matrix is generated and reordered once for the cases that differ in these only
DEVICE_ONLY = ("ell_variant", "ell_nt", "ell_keep", "ell_triples", "ell_alternate", "val_f32")


def window_rows(threads, dyn, inl, sym, ks=(1,), stamps=False, f32=0):
    """rows of the window table: threads, k, dyn, stamp, inl, sym, f32 (k > 1: the LDS counter only)"""
    rows = {(threads, k, dyn if k == 1 else 1, 0, inl, sym, f32) for k in ks}
    if stamps:
        rows.add((threads, 1, dyn, 1, inl, sym, 0))
    return rows


@dataclass
class CensusCase:
    id: str
    gen: tuple
    kw: dict
    ops: tuple                       # of "spmv" (automatic walk, walk 0, walk 1, phases 1 + 2), "spmm" (k = 2..5), "stamps", "alternate4"
    rows: dict                       # table name -> the set of rows the ops must launch
    sym_values: bool = True
    # what the host-only plan must show: inline residual, symmetric pairs, a CSR residual launch, panel form, direct shape, k_max
    inl: int = 0
    sym: int = 0
    csr: bool = False
    panel: bool = False
    direct: bool = False
    kmax: int = 4
    coded: object = None             # True: ehyb_plan_device_cols reports triple-coded slabs, False: none, None: not asked
    split_rows: bool = False
    shows: tuple = ()                # of SHOWS: what this case must show (window cases)
    walk_key: tuple = field(default=None)   # (dyn, threads) of a window case

    def cfg(self, E):
        return E.make_config(**self.kw)


_matrices = {}


def build_matrix(E, case):
    """generate -> integer values -> (caller's partition sizes) -> reorder; one matrix for all cases with the same host inputs.
    The matrix is shared: nobody changes it."""
    host_kw = tuple(sorted((k, v) for k, v in case.kw.items() if k not in DEVICE_ONLY))
    key = (case.gen, case.sym_values, host_kw)
    if key not in _matrices:
        cfg = E.make_config(**dict(host_kw))
        m = E.Matrix.generate(case.gen[0], *case.gen[1], cfg=cfg)
        m.V[:] = integer_values(m.I, m.J, case.sym_values)
        if len(case.gen) > 2:
            m.c.nParts, m.c.vectorCacheSize = case.gen[2]
        m.reorder(cfg)
        _matrices.clear()            # (one at a time: the cases come grouped by matrix)
        _matrices[key] = m
    return _matrices[key]


_products = {}


def products(m, key, k=5):
    """k integer columns (seeds 1..k) in the permuted numbering and their exact products, computed once per matrix"""
    if key not in _products:
        _products.clear()
        X = np.stack([integer_x(m.n, j + 1) for j in range(k)])
        _products[key] = (X, np.stack([exact_reference(m.n, m.I, m.J, m.V, x) for x in X]))
    return _products[key]


def matrix_key(case):
    return (case.gen, case.sym_values, tuple(sorted((k, v) for k, v in case.kw.items() if k not in DEVICE_ONLY)))


# ---------------------------------------------------------------------------------------------- what a plan shows
def device_coded_slabs(plan):
    """number of triple-coded slabs in the column words as ehyb_plan_upload sends them (ehyb_plan_device_cols)"""
    import ctypes as C

    lib = plan.lib
    words = np.zeros(max(int(lib.ehyb_plan_device_col_words(plan.h)), 1), dtype=np.uint32)
    meta = np.zeros(len(plan.array("slab_meta")), dtype=np.uint32)
    assert lib.ehyb_plan_device_cols(plan.h, words.ctypes.data_as(C.POINTER(C.c_uint32)), meta.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    return int(((meta.reshape(-1, 4)[:, 3] & 0x40) != 0).sum())


def plan_shows(plan, threads):
    """which of SHOWS the window launch of this plan shows at this workgroup size"""
    segs, items = plan.array("segs").reshape(-1, 8), plan.array("items").reshape(-1, 8)
    if len(segs) == 0:
        return set()
    slabs, waves = segs[:, 2] - segs[:, 1], threads // 64
    out = set()
    if slabs.max() > waves:
        out.add("more")
    if slabs.min() < waves:
        out.add("fewer")
    if segs[:, 3].max() > 0:
        out.add("halo")
    if (items[:, 1] - items[:, 0]).max() > 1:
        out.add("multiseg")
    return out


def check_plan(case, plan, threads):
    """the host-only (or uploaded) plan is the one the case claims: path taken, what it shows, ehyb_spmm_max_k"""
    st = plan.stats
    what = (case.id, st)
    direct = st["nnz_ell"] == 0 and st["nnz_er"] == st["nnz"] and st["er_segments"] == plan.n
    assert direct == case.direct, what
    assert (st["er_inline"] > 0) == bool(case.inl), what
    assert (st["sym_pairs"] > 0) == bool(case.sym), what
    assert (st["er_partials"] > 0) == case.panel, what
    assert (st["nnz_er"] > 0 and st["er_inline"] == 0 and st["er_partials"] == 0) == case.csr, what
    assert plan.spmm_max_k == case.kmax, (case.id, plan.spmm_max_k)
    if case.panel:
        assert st["nnz_ell"] == 0, what                # every entry in panel form (the windows are kept and launched: they hold no entry)
    if case.rows.get("window"):
        assert (st["nnz_ell"] > 0 or case.panel) and st["n_items"] > 0 and len(plan.array("segs")) > 0, what
        assert set(case.shows) <= plan_shows(plan, threads), (case.id, case.shows, plan_shows(plan, threads))
    if "stamps" in case.ops:                                                     # the window launch writes the final y
        assert st["nnz_er"] == 0 or st["er_inline"] > 0, what
    if case.coded is not None:
        assert (device_coded_slabs(plan) > 0) == case.coded, (case.id, device_coded_slabs(plan))
    if case.split_rows:
        assert bool((plan.array("er_seg_row") < 0).any()), what


# ---------------------------------------------------------------------------------------------- the window table, fp64
# the four forms (inline residual, symmetric pairs) on plans whose window launch writes the final y (so that the stamped launch
# of ehyb_debug_ell_stamps can be checked against the product), and a fifth plan with a CSR residual and items of several segments
NO_ER = dict(window_mode=2, lds_doubles=LDS_K4, fuse_er=2, direct=2)            # every halo column fits: no residual
FORMS = [
    # (name, matrix, config, inl, sym, CSR residual launch, shows, stamps)
    ("plain", FEM, NO_ER, 0, 0, False, ("fewer", "halo"), True),
    ("sym", FEM24, dict(sym_pairs=1, **NO_ER), 0, 1, False, ("more", "halo"), True),
    ("inline", FEM, dict(window_mode=2, lds_doubles=1024, fuse_er=1, direct=2), 1, 0, False, ("fewer", "halo"), True),
    ("inline-sym", FEM, dict(direct=2, **FEM_INLINE_SYM), 1, 1, False, ("fewer", "halo"), True),
    ("csr-multiseg", FEM, dict(window_mode=2, lds_doubles=256, items_per_cu=1, fuse_er=2, direct=2), 0, 0, True, ("fewer", "halo", "multiseg"), False),
]
# the two value-load bodies (ell_nt = 1: every slab hinted, 2: none) x the two forms of the column words (ell_triples = 1 on a
# plan that has coded slabs, 2: the host's pair words): every arm runs under each
VARIANTS = [("nt1-coded", dict(ell_nt=1, ell_triples=1)), ("nt2-pairs", dict(ell_nt=2, ell_triples=2))]


def _coded(inl, sym, kmax, triples):
    if triples == 2:
        return False
    return not (inl and sym and kmax >= 4)       # (plan_keeps_pair_words: K = 4 with pairs and an inline residual has no decoder)


def _phase_1(threads, dyn, inl, sym):
    """A plan with an inline residual multiplies in phases 1 + 2 (the "spmv" op) WITHOUT it: phase 1 is the window kernel of the
    same form with no inline residual, phase 2 the CSR residual kernel."""
    return window_rows(threads, dyn, 0, sym) if inl else set()


def _phase_2(inl):
    return {(1, 0, 0)} if inl else set()


def window_cases():
    out = []
    for name, gen, kw, inl, sym, csr, shows, stamps in FORMS:
        for threads in THREADS:
            for vname, vkw in VARIANTS:
                er = {(k, 0, 0) for k in (1, 2, 3, 4)} if csr else set()
                # LDS-counter walk: K = 1..4 on one plan (k = 5 splits 3 + 2)
                out.append(CensusCase(
                    id=f"{name}-t{threads}-dyn-{vname}", gen=gen, kw=dict(threads=threads, ell_variant=1, **kw, **vkw),
                    ops=("spmv", "spmm") + (("stamps",) if stamps else ()),
                    rows=dict(window=window_rows(threads, 1, inl, sym, (1, 2, 3, 4), stamps) | _phase_1(threads, 1, inl, sym), panel=set(),
                              er_csr=er | _phase_2(inl)),
                    inl=inl, sym=sym, csr=csr, coded=_coded(inl, sym, 4, vkw["ell_triples"]), shows=shows, walk_key=(1, threads)))
                # static round-robin: one vector only (a wider pass of such a plan takes the LDS counter)
                out.append(CensusCase(
                    id=f"{name}-t{threads}-static-{vname}", gen=gen, kw=dict(threads=threads, ell_variant=3, ell_alternate=1, **kw, **vkw),
                    ops=("spmv", "alternate4") + (("stamps",) if stamps else ()),
                    rows=dict(window=window_rows(threads, 0, inl, sym, (1,), stamps) | _phase_1(threads, 0, inl, sym), panel=set(),
                              er_csr=({(1, 0, 0)} if csr else set()) | _phase_2(inl)),
                    inl=inl, sym=sym, csr=csr, coded=_coded(inl, sym, 4, vkw["ell_triples"]), shows=shows, walk_key=(0, threads)))
    # symmetric pairs AND an inline residual with triple-coded slabs: a plan three columns wide (K = 4 of that form is the one
    # kernel without a decoder).  Contiguous partitions of the scrambled FEM matrix: few pairs, a large residual.
    k3 = dict(window_mode=2, lds_doubles=6826, partitioner=1, fuse_er=1, sym_pairs=1, direct=2, ell_triples=1)
    for threads in THREADS:
        for nt in (1, 2):
            out.append(CensusCase(
                id=f"inline-sym-k3-t{threads}-dyn-nt{nt}-coded", gen=FEM, kw=dict(threads=threads, ell_nt=nt, **k3), ops=("spmv", "spmm", "stamps"),
                rows=dict(window=window_rows(threads, 1, 1, 1, (1, 2, 3), True) | _phase_1(threads, 1, 1, 1), panel=set(), er_csr=_phase_2(1)),
                inl=1, sym=1, kmax=3, coded=True, shows=("halo",), walk_key=(1, threads)))
            out.append(CensusCase(
                id=f"inline-sym-k3-t{threads}-static-nt{nt}-coded", gen=FEM, kw=dict(threads=threads, ell_nt=nt, ell_variant=3, ell_alternate=1, **k3),
                ops=("spmv", "alternate4", "stamps"),
                rows=dict(window=window_rows(threads, 0, 1, 1, (1,), True) | _phase_1(threads, 0, 1, 1), panel=set(), er_csr=_phase_2(1)),
                inl=1, sym=1, kmax=3, coded=True, shows=("halo",), walk_key=(0, threads)))
    return out


# ---------------------------------------------------------------------------------------------- the panel table
def panel_cases():
    """pass 1: both workgroup sizes x {register-scan sums, LDS sums} at K = 1 and K = 2..4; pass 2: streamed and cached at K = 1..4.
    The four probe rows: ELSEWHERE."""
    out = []
    for threads, er_sums, er_nt in ((512, 1, 1), (512, 2, 2), (1024, 1, 2), (1024, 2, 1)):
        dpp = 1 if er_sums != 2 else 0
        rows = {(1, threads, 1, dpp, 0, 0)} | {(1, threads, k, 1, 0, 0) for k in (2, 3, 4)} | {(2, 512, k, 1, 0, 1 if er_nt == 1 else 0) for k in (1, 2, 3, 4)}
        out.append(CensusCase(
            id=f"panel-t{threads}-{'scan' if dpp else 'lds'}-sums-pass2-{'streamed' if er_nt == 1 else 'cached'}", gen=RMAT14,
            kw=dict(er_sums=er_sums, er_panel_threads=threads, er_nt=er_nt, **PANEL_ARMS), ops=("spmv", "spmm"), sym_values=False,
            rows=dict(window=window_rows(1024, 1, 0, 0, (1, 2, 3, 4)), panel=rows, er_csr=set()), panel=True))   # (er_mode = 2 keeps the empty windows)
    return out


# ---------------------------------------------------------------------------------------------- the CSR residual table
def er_cases():
    """add (behind a window launch) with split rows and ASSIGN (the direct shape) at K = 1..4 -- the add rows without split rows
    run in the csr-multiseg window cases too --, and the two fp32 kernels"""
    split = dict(window_mode=1, lds_doubles=256, er_seg_len=16, er_mode=1, fuse_er=2)
    return [
        CensusCase(id="er-add-split-rows", gen=RMAT11, kw=split, ops=("spmv", "spmm"), sym_values=False, csr=True, split_rows=True,
                   rows=dict(window=window_rows(1024, 1, 0, 0, (1, 2, 3, 4)), panel=set(), er_csr={(k, 0, 0) for k in (1, 2, 3, 4)})),
        CensusCase(id="er-assign-direct", gen=RMAT13D, kw=dict(), ops=("spmv", "spmm"), sym_values=False, direct=True, csr=True,
                   rows=dict(window=set(), panel=set(), er_csr={(k, 1, 0) for k in (1, 2, 3, 4)})),
        CensusCase(id="er-add-split-rows-f32", gen=RMAT11, kw=dict(val_f32=1, **split), ops=("spmv",), sym_values=False, csr=True, split_rows=True, kmax=1,
                   rows=dict(window=window_rows(1024, 1, 0, 0, f32=1), panel=set(), er_csr={(1, 0, 1)})),
        CensusCase(id="er-assign-direct-f32", gen=RMAT13D, kw=dict(val_f32=1), ops=("spmv",), sym_values=False, direct=True, csr=True, kmax=1,
                   rows=dict(window=set(), panel=set(), er_csr={(1, 1, 1)})),
    ]


CASES = window_cases() + panel_cases() + er_cases()
assert len({c.id for c in CASES}) == len(CASES)

# ---------------------------------------------------------------------------------------------- rows other tests launch
# (table, row, the test that launches it and asserts it in the plan's launch log)
ELSEWHERE = [("panel", (1, threads, 1, dpp, 1, 0), f"test_gpu_exact.py::test_panel_times_probes_launch_and_leave_the_product[{2 - dpp}-{threads}]")
             for threads in (512, 1024) for dpp in (1, 0)]
# the fp32 window kernels: the table in the docstring of test_gpu_val_f32.py (1024, no, no runs in er-add-split-rows-f32 here too)
_F32_NAMED = {(256, 0, 0): "test_exact_named_path_f32[refwindow-t256-lds1024]", (256, 0, 1): "test_exact_random_plan_f32[134]",
              (256, 1, 0): "test_exact_random_plan_f32[108]", (512, 0, 0): "test_exact_named_path_f32[halo-t512-lds64]",
              (512, 0, 1): "test_exact_named_path_f32[sym-fem-3dof-t512-lds20480]", (512, 1, 0): "test_exact_random_plan_f32[101]",
              (1024, 0, 0): "test_exact_named_path_f32[refwindow-t1024-lds20480]", (1024, 0, 1): "test_exact_named_path_f32[sym-fem-3dof]",
              (1024, 1, 0): "test_exact_named_path_f32[inline-residual]"}
for _t in THREADS:
    _F32_NAMED[(_t, 1, 1)] = f"test_inline_residual_with_symmetric_pairs_f32[{_t}-triples1]"
ELSEWHERE += [("window", (t, 1, 1, 0, inl, sym, 1), "test_gpu_val_f32.py::" + test) for (t, inl, sym), test in sorted(_F32_NAMED.items())]

# rows no case launches: (table, row, one-line reason).  Empty.
EXEMPT = []


def f32_window_row(arm):
    """val_f32_cases.window_arm -> the row of the window table that launch must log"""
    threads, inl, sym = arm
    return (int(threads), 1, 1, 0, int(bool(inl)), int(bool(sym)), 1)
