"""Cases shared by the tests of the transposed multiply (test_spmv_t_host.py, test_gpu_spmv_t.py): the named paths of
test_gpu_exact.py that ehyb_spmv_t serves with the rows of E.kernel_table_t() each must launch, the forms it refuses, and a small
matrix whose triple-coded slabs have 1, 2 and 6 pairs.  No tests here."""
import numpy as np

from test_col_triples import node_matrix

# rows of E.kernel_table_t(): (kind 0 window / 1 residual, threads, inline residual)
W1024, W1024I = (0, 1024, 0), (0, 1024, 1)
W512, W512I = (0, 512, 0), (0, 512, 1)
W256, W256I = (0, 256, 0), (0, 256, 1)
RES = (1, 256, 0)
ALL_ROWS = {W1024, W1024I, W512, W512I, W256, W256I, RES}

# name of test_gpu_exact.PATHS -> the rows its transposed multiply launches.  Which case launches which row:
#   (0, 256, 0)   refwindow-t256-lds1024           (0, 256, 1)   inline-t256 (EXTRA_PATHS)
#   (0, 512, 0)   halo-t512-lds64                  (0, 512, 1)   inline-t512 (EXTRA_PATHS)
#   (0, 1024, 0)  refwindow-t1024-lds20480, csr-split-16, csr-split-64, relative-columns
#   (0, 1024, 1)  halo-t1024-lds20480 (its 144 residual entries ride inline), inline-residual
#   (1, 256, 0)   every window case with a CSR residual, and direct-rmat, direct-fem alone
NAMED = {
    "refwindow-t256-lds1024": {W256, RES},
    "halo-t512-lds64": {W512, RES},
    "halo-t1024-lds20480": {W1024I},
    "refwindow-t1024-lds20480": {W1024, RES},
    "inline-residual": {W1024I},
    "csr-split-16": {W1024, RES},
    "csr-split-64": {W1024, RES},
    "direct-rmat": {RES},
    "direct-fem": {RES},
    "relative-columns": {W1024},
}

FEM = ("fem3d", (30000, 3, 22, 22, 13500, 1, 1))
# the two instantiations no named path of test_gpu_exact.py reaches: an inline residual at 256 and 512 threads
# (id, matrix, config, what the stats must show, rows)
EXTRA_PATHS = [
    ("inline-t256", FEM, dict(window_mode=1, lds_doubles=20480, fuse_er=1, threads=256),
     lambda p, n: p.stats["er_inline"] > 0 and p.stats["nnz_er"] > 0, {W256I}),
    ("inline-t512", FEM, dict(window_mode=2, lds_doubles=2048, fuse_er=1, threads=512, direct=2),
     lambda p, n: p.stats["er_inline"] > 0 and p.stats["nnz_er"] > 0, {W512I}),
]

# (id, matrix, config, the words ehyb_last_error must hold): the forms ehyb_spmv_t refuses (a row range and column segments:
# test_spmv_t_host.py)
REFUSED = [
    ("sym-pairs", FEM, dict(lds_doubles=4096, sym_pairs=1), "symmetric pair storage"),
    ("panel", ("rmat", (14, 1 << 17, 1)), dict(er_mode=2, fuse_er=2, lds_doubles=512, er_panel_cols=512, er_block_rows=300), "panel form"),
    ("val-f32", FEM, dict(lds_doubles=4096, val_f32=1, direct=2), "val_f32"),
]


def nodes_and_pairs(n_nodes=2048, n_pairs=1000):
    """CSR pattern (indptr, indices): the node matrix of test_col_triples.py -- 3 unknowns per node, rows of 3, 9 and 12 entries:
    slabs of 2, 5 and 6 pairs -- and behind it n_pairs nodes of TWO unknowns coupled to themselves only: rows of the two entries
    (a, a + 1), slabs of ONE pair, which the triple form codes as a word for one pair.  With both, triple-coded slabs with
    pairs % 3 of 0, 1 and 2 occur (node triples alone give rows of 3 k entries: 2 pairs = 3 k or 3 k + 1, never 3 k + 2)."""
    indptr, indices, _ = node_matrix(n_nodes)
    n3 = len(indptr) - 1
    tail = n3 + 2 * (np.arange(2 * n_pairs) // 2)
    indptr = np.concatenate([indptr, indptr[-1] + 2 * np.arange(1, 2 * n_pairs + 1)])
    indices = np.concatenate([indices, np.stack([tail, tail + 1], axis=1).ravel()])
    return indptr, indices


# The seeds of test_gpu_exact.test_exact_random_plan (range(100, 140)) whose plan ehyb_spmv_t serves: 28 of 40, found with host-only
# plans (test_spmv_t_host.py holds the list to that rule); of the other 12, ten drew symmetric pair storage and two a panel residual.
FUZZ_RANGE = range(100, 140)
FUZZ_REFUSED = [104, 113, 115, 118, 120, 122, 123, 127, 129, 131, 134, 138]
FUZZ_SEEDS = [s for s in FUZZ_RANGE if s not in FUZZ_REFUSED]


def fuzz_case(E, O, seed, **overrides):
    """fuzz_cases.build(exact=True) with the values replaced by UNSYMMETRIC integers (with symmetric values the forward kernel
    would pass) -> (matrix, config, x permuted, exact A^T x permuted)"""
    from exact_cases import exact_reference, integer_values
    from fuzz_cases import build

    m, cfg, kw, x, _, _ = build(E, O, seed, exact=True, **overrides)
    if m.nnz:
        m.V[:] = integer_values(m.I, m.J, False, salt=seed)
    xp = E.vector_reorder(x, m.reorder_list)
    return m, cfg, xp, exact_reference(m.n, m.J, m.I, m.V, xp)
