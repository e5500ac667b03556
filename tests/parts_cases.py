"""Rank-local matrices for the multiply in PARTS (ehyb_spmv_part, ehyb_step_*, ehyb_halo_step; include/ehyb.h "The multiply in
PARTS"), built the way dist.RankLocalMatrix builds them but small and by hand: an own block of n0 rows from a generator,
reordered; Matrix.append_ghosts for the receive columns and the entries that couple own rows to them; for the split case
ehyb_matrix_append_rows for foreign rows with entries in own columns only.  Every value is then overwritten with a small
integer and x holds integers (exact_cases.py), so the product over the whole rank-local matrix, in plan numbering, is ONE
number per row whatever the order of summation, and every comparison is bit for bit.

The ghost columns come in CHUNK_COLS chunks, every start even (n0 is even and so is every chunk length but the last one's,
which nothing follows): many panels of 256 columns with a ragged last one, a chunk barely over one panel, an empty chunk and
a chunk smaller than a panel.  Cases only; test_parts_host.py proves what they claim, test_gpu_parts_exact.py runs them."""
import ctypes as C

import numpy as np

from exact_cases import exact_reference, integer_values, integer_x

PART_FIRST, PART_LAST, PART_LAST_FOREIGN = 1, 2, 4     # EHYB_PART_* of ehyb.h
ERR_ARG, ERR_STATE = 1, 8                              # EHYB_ERR_ARG, EHYB_ERR_STATE

CHUNK_COLS = (700, 258, 0, 2)
PANEL_COLS = 256
N_FOREIGN = 300
_PANEL = dict(er_mode=2, fuse_er=2, direct=2, er_panel_cols=PANEL_COLS, er_block_rows=100)
_RMAT = ("rmat", (11, 1 << 14, 1))
_STENCIL = ("stencil2d", (40, 40, 5, 200, 3))

# name -> (generator of the own block, what sizes the partitions (reorder AND plan), the plan's further fields, foreign rows)
# (value_map on the window cases: the plan then names the entry behind every window slot, and with it what the window launch
# alone must leave in y -- the layout is the same array for array)
CASES = {
    "panel-all": (_RMAT, dict(lds_doubles=1024), dict(prune_pct=1, **_PANEL), 0),
    "panel-split": (_RMAT, dict(lds_doubles=1024), dict(prune_pct=1, **_PANEL), N_FOREIGN),
    "panel-windows-kept": (_RMAT, dict(lds_doubles=512), dict(ell_prune=2, value_map=1, **_PANEL), 0),
    "csr-windows": (_STENCIL, dict(lds_doubles=1024), dict(er_mode=1, fuse_er=2, direct=2, value_map=1), 0),
    "csr-windows-f32": (_STENCIL, dict(lds_doubles=1024), dict(er_mode=1, fuse_er=2, direct=2, value_map=1, val_f32=1), 0),
}
PANEL_CASES = ("panel-all", "panel-split", "panel-windows-kept")
WINDOW_CASES = ("panel-windows-kept", "csr-windows", "csr-windows-f32")
CSR_CASES = ("csr-windows", "csr-windows-f32")


def _ghost_entries(n0, n_ghost, seed):
    """Coupling entries (own row, ghost column), no pair twice: every ghost column is referenced by one to four own rows, and a
    few hub rows reference a run of ghost columns each (long pieces in the panels)."""
    rng = np.random.default_rng(seed)
    per = rng.integers(1, 5, n_ghost)
    gj = np.repeat(np.arange(n_ghost), per)
    gi = rng.integers(0, n0, len(gj))
    hubs = rng.choice(n0, 4, replace=False)
    hi = np.repeat(hubs, 150)
    hj = np.concatenate([(h * 37 + np.arange(150) * 5) % n_ghost for h in range(4)])
    pairs = np.unique(np.stack([np.concatenate([gi, hi]), np.concatenate([gj, hj])], axis=1), axis=0)
    return pairs[:, 0].astype(np.int32), pairs[:, 1].astype(np.int32)


def _foreign_entries(n0, n_foreign, seed):
    """Entries of the foreign rows (row ascending, own columns only, no pair twice): one to five per row, row 7 empty."""
    rng = np.random.default_rng(seed)
    per = rng.integers(1, 6, n_foreign)
    per[7] = 0
    ri = np.repeat(np.arange(n_foreign), per)
    cj = rng.integers(0, n0, len(ri))
    pairs = np.unique(np.stack([ri, cj], axis=1), axis=0)
    return pairs[:, 0].astype(np.int32), pairs[:, 1].astype(np.int32)


class PartsCase:
    """One rank-local matrix in plan numbering: columns [0, n0) own, then the ghost columns chunk by chunk (segs); rows [0, n0)
    own, then n_foreign foreign rows.  I, J, V, x and y_ref (the exact product, n_rows long) stay as made: share, do not write."""

    def __init__(self, E, name, x_seed=1):
        gen, size_kw, plan_kw, n_foreign = CASES[name]
        self.E, self.name, self.n_foreign = E, name, n_foreign
        cfg0 = E.make_config(**size_kw)
        m = E.Matrix.generate(gen[0], *gen[1], cfg=cfg0)
        m.reorder(cfg0)
        n0 = self.n0 = m.n
        assert n0 % 2 == 0, "the first ghost column must be even"
        starts = n0 + np.concatenate([[0], np.cumsum(CHUNK_COLS)])
        assert np.all(starts[:-1] % 2 == 0), "every chunk starts on an even column"
        self.segs = np.concatenate([[0], starts]).astype(np.int32)      # segment 0 = the own columns, then one per chunk
        n_ghost = int(starts[-1]) - n0
        gi, gj = _ghost_entries(n0, n_ghost, 11)
        m.append_ghosts(n_ghost, gi, gj, np.ones(len(gi)))
        if n_foreign:
            ri, cj = _foreign_entries(n0, n_foreign, 12)
            lib = E.host._lib.load()
            v = np.ones(len(ri))
            E.host._check(lib.ehyb_matrix_append_rows(C.byref(m.c), n0, n_foreign, len(ri), ri.ctypes.data_as(C.POINTER(C.c_int)),
                                                      cj.ctypes.data_as(C.POINTER(C.c_int)), v.ctypes.data_as(C.POINTER(C.c_double)), 256),
                          "ehyb_matrix_append_rows")
            plan_kw = dict(plan_kw, row_split=n0)
        self.m, self.n, self.n_rows = m, m.n, n0 + n_foreign
        m.V[:] = integer_values(m.I, m.J, False)                        # ghost and foreign entries included
        self.I, self.J, self.V = m.I.copy(), m.J.copy(), m.V.copy()
        # (n_top = 2, as dist.RankLocalMatrix sets it for a rank that exchanges: a window then holds the plan's own columns only)
        self.cfg = E.make_config(n_top=2, **size_kw, **plan_kw)
        self.panel, self.split, self.windows = name in PANEL_CASES, n_foreign > 0, name in WINDOW_CASES
        self.n_segs = len(self.segs) - 1
        self.x = integer_x(self.n, x_seed)
        self.y_ref = self.reference(self.x)

    def reference(self, x):
        return exact_reference(self.n, self.I, self.J, self.V, x)[:self.n_rows]

    def plan(self, upload=True):
        return self.E.Plan(self.m, self.cfg, rows=(0, self.n_rows), upload=upload, col_segs=self.segs)

    def chunks(self):
        """(segment, first column, end column) of every ghost chunk, the empty one included"""
        return [(s, int(self.segs[s]), int(self.segs[s + 1])) for s in range(1, self.n_segs)]

    def window_product(self, plan, x):
        """-> (y, rows): what the window launch (EHYB_PART_FIRST) alone leaves in y -- the exact sum of the entries the plan keeps in
        its windows (ell_src: cfg.value_map) -- and the rows it writes: all but those a pass-2 unit ASSIGNS (rows < 0 in pb_units2:
        partitions without a window)."""
        src = plan.array("ell_src")
        src = src[src >= 0]
        assert len(src) == plan.stats["nnz_ell"] and len(np.unique(src)) == len(src)
        y = exact_reference(self.n, self.I[src], self.J[src], self.V[src], x)[:self.n_rows]
        rows = np.ones(self.n_rows, dtype=bool)
        for _, _, r0, nr in plan.array("pb_units2").reshape(-1, 4):
            if nr < 0:
                rows[r0:r0 - nr] = False
        return y, rows


_cache = {}


def case(E, name):
    """The case `name`, built once per session."""
    if name not in _cache:
        _cache[name] = PartsCase(E, name)
    return _cache[name]
