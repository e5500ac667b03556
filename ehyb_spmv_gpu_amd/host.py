"""Python mirror of the reference's host interface for the EHYB path.

Names follow the reference (solver_test.c / spmv.h / reordering.h): a `Matrix` is a
`matrixCOO`, `matrix_reorder` is `matrixReorder[_unsym]`, `vector_reorder` /
`vector_recover` are `vectorReorder` / `vectorRecover`, `spmv_gpu_ehyb` is `spmvGPuEHYB`.
Everything is a thin call into libehyb.so; numpy is used only to hand buffers over.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Config, MatrixCOO, Stats

EHYB_WINDOW_REFERENCE = 1
EHYB_WINDOW_HALO = 2
EHYB_PART_AUTO, EHYB_PART_CONTIGUOUS, EHYB_PART_MULTILEVEL, EHYB_PART_MTMETIS, EHYB_PART_DEGREE = 0, 1, 2, 3, 4

ARRAYS = {
    "part_boundary": (0, np.int32), "win_len": (1, np.int32), "halo_ptr": (2, np.int32),
    "halo_cols": (3, np.int32), "slab_pair_ptr": (4, np.uint32), "slab_row": (5, np.int32),
    "slab_part": (6, np.int32), "ell_val": (7, np.float64), "ell_col": (8, np.uint32),
    "items": (9, np.int32), "er_seg_ptr": (10, np.int64), "er_seg_row": (11, np.int32),
    "er_col": (12, np.int32), "er_val": (13, np.float64), "er_bins": (14, np.int32),
    "slab_col_ptr": (15, np.uint32), "lane_group": (16, np.uint8), "slab_meta": (17, np.uint32),
    "segs": (18, np.int32), "perm": (19, np.int32), "slab_lrow": (20, np.uint16),
    "pb_val": (21, np.float64), "pb_col": (22, np.uint16), "pb_dst": (23, np.uint32), "pb_units1": (24, np.int32),
    "pb_row": (25, np.uint16), "pb_units2": (26, np.int32),
    "pb_colf": (31, np.uint16), "pb_chunk": (32, np.uint32), "pb_jump": (33, np.uint32),
    "ell_src": (27, np.int32), "er_src": (28, np.int32), "pb_src": (29, np.int32), "ell_src2": (30, np.int32),
    "col_seg_first": (34, np.int32), "pb_seg_item": (35, np.int32), "pb_items1": (36, np.int32),
}


class EhybError(RuntimeError):
    def __init__(self, code, where):
        msg = _lib.load().ehyb_last_error().decode(errors="replace")
        super().__init__(f"{where} failed with status {code}: {msg}")
        self.code = code


def _check(code, where):
    if code != 0:
        raise EhybError(code, where)


def make_config(**kw):
    """ehyb_config with defaults, overridden by keyword (field names of ehyb.h)."""
    cfg = Config()  # all zero = all defaults
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise TypeError(f"unknown ehyb_config field {k!r}")
        setattr(cfg, k, int(v))
    # fill in what the library will use (window and partition sizes depend on the mode fields)
    _lib.load().ehyb_config_resolve(C.byref(cfg), C.byref(cfg))
    return cfg


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


# the kernel tables of the library (EHYB_KERNELS_* of ehyb.h, in that order) and the fields of a row of each
KERNEL_TABLES = {
    "window": ("threads", "k", "dyn", "stamp", "inl", "sym", "f32"),
    "panel": ("pass", "threads", "k", "dpp", "probe", "nt"),
    "er_csr": ("k", "assign", "f32"),
}


def kernel_table(name):
    """ehyb_debug_kernel_table -> the rows of table "window", "panel" or "er_csr" as tuples of ints (KERNEL_TABLES[name] names
    the fields), in table order.  Needs no device."""
    lib = _lib.load()
    which, width = list(KERNEL_TABLES).index(name), len(KERNEL_TABLES[name])
    n = C.c_int(0)
    _check(lib.ehyb_debug_kernel_table(which, None, 0, C.byref(n)), "ehyb_debug_kernel_table")
    rows = np.zeros((n.value, width), dtype=np.int32)
    _check(lib.ehyb_debug_kernel_table(which, _ptr(rows, C.c_int32), n.value, C.byref(n)), "ehyb_debug_kernel_table")
    return [tuple(int(v) for v in r) for r in rows]


# the fields of a row of the transposed multiply's own table (ehyb_debug_kernel_table_t): kind 0 = window, 1 = residual
KERNEL_TABLE_T = ("kind", "threads", "inl")


def kernel_table_t():
    """ehyb_debug_kernel_table_t -> the rows of the transposed multiply's kernel table as tuples of ints (KERNEL_TABLE_T names
    the fields), in table order.  Needs no device."""
    lib = _lib.load()
    n = C.c_int(0)
    _check(lib.ehyb_debug_kernel_table_t(None, 0, C.byref(n)), "ehyb_debug_kernel_table_t")
    rows = np.zeros((n.value, len(KERNEL_TABLE_T)), dtype=np.int32)
    _check(lib.ehyb_debug_kernel_table_t(_ptr(rows, C.c_int32), n.value, C.byref(n)), "ehyb_debug_kernel_table_t")
    return [tuple(int(v) for v in r) for r in rows]


def _view(ptr, count, dtype):
    if count == 0:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(C.addressof(ptr.contents))
    return np.frombuffer(buf, dtype=dtype, count=count)


def x_glibc(n):
    """x[i]: srand(i); (rand()%200-100)/1000 -- solver_test.c:89-92, 228-231."""
    x = np.empty(n, dtype=np.float64)
    _lib.load().ehyb_x_glibc(n, _ptr(x, C.c_double))
    return x


def sizing(dimension, cfg=None):
    """(nParts, vectorCacheSize, kernelPerPart) -- solver_test.c:53-77 re-derived."""
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    _check(_lib.load().ehyb_sizing(dimension, C.byref(cfg) if cfg else None, C.byref(a), C.byref(b), C.byref(c)),
           "ehyb_sizing")
    return a.value, b.value, c.value


class Matrix:
    """Owner of a matrixCOO whose arrays live in the C heap (the reorder step frees and
    replaces I/J/V exactly like reordering.c:363-369)."""

    def __init__(self):
        self.lib = _lib.load()
        self.c = MatrixCOO()
        self.symmetric = False
        self._alive = False

    # ---- constructors
    @classmethod
    def from_csr(cls, indptr, indices, data, cfg=None, symmetric=False):
        m = cls()
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float64)
        n = len(indptr) - 1
        _check(m.lib.ehyb_matrix_from_csr(n, _ptr(indptr, C.c_int64), _ptr(indices, C.c_int), _ptr(data, C.c_double),
                                          C.byref(cfg) if cfg else None, C.byref(m.c)), "ehyb_matrix_from_csr")
        m._alive = True
        m.symmetric = symmetric
        return m

    @classmethod
    def read_mtx(cls, path, cfg=None):
        m = cls()
        sym = C.c_int(0)
        _check(m.lib.ehyb_mm_read(str(path).encode(), C.byref(cfg) if cfg else None, C.byref(m.c), C.byref(sym)),
               "ehyb_mm_read")
        m._alive = True
        m.symmetric = bool(sym.value)
        return m

    @classmethod
    def generate(cls, kind, *args, cfg=None):
        m = cls()
        cp = C.byref(cfg) if cfg else None
        if kind == "banded":
            n, band, block = args
            rc = m.lib.ehyb_gen_banded(n, band, block, cp, C.byref(m.c))
        elif kind == "fem3d":
            n, dof, nx, ny, ppm, scramble, seed = args
            rc = m.lib.ehyb_gen_fem3d(n, dof, nx, ny, ppm, scramble, seed, cp, C.byref(m.c))
            m.symmetric = True
        elif kind == "fem3d_graded":
            n, dof, nx, ny, near_ppm, far_ppm, scramble, seed = args
            rc = m.lib.ehyb_gen_fem3d_graded(n, dof, nx, ny, near_ppm, far_ppm, scramble, seed, cp, C.byref(m.c))
            m.symmetric = True
        elif kind == "fem3d_block":
            n, dof, nx, ny, ppm, scramble, seed, block, n_blocks = args
            rc = m.lib.ehyb_gen_fem3d_block(n, dof, nx, ny, ppm, scramble, seed, block, n_blocks, cp, C.byref(m.c))
            m.symmetric = n_blocks == 1
        elif kind == "rmat":
            scale, edges, seed = args
            rc = m.lib.ehyb_gen_rmat(scale, edges, seed, cp, C.byref(m.c))
        elif kind == "rmat_block":
            scale, edges, seed, block, n_blocks = args[:5]
            cost_model = int(args[5]) if len(args) > 5 else 0      # 1: cuts balanced for the "cover" exchange (ehyb_gen_rmat_block_cost)
            cuts = (C.c_int * (n_blocks + 1))()
            rc = m.lib.ehyb_gen_rmat_block_cost(scale, edges, seed, block, n_blocks, cost_model, cuts, cp, C.byref(m.c))
            m.block_cuts = [int(c) for c in cuts]
        elif kind == "rmat_rows":
            scale, edges, seed, row0, row1 = args
            rc = m.lib.ehyb_gen_rmat_rows(scale, edges, seed, row0, row1, cp, C.byref(m.c))
        elif kind == "stencil2d":
            nx, ny, points, extra, seed = args
            rc = m.lib.ehyb_gen_stencil2d(nx, ny, points, extra, seed, cp, C.byref(m.c))
            m.symmetric = True
        elif kind == "kkt3d":
            (nx,) = args
            rc = m.lib.ehyb_gen_kkt3d(nx, cp, C.byref(m.c))
            m.symmetric = True
        elif kind == "mesh3d":
            n, dof, knn, grade, seed = args
            rc = m.lib.ehyb_gen_mesh3d(n, dof, knn, grade, seed, cp, C.byref(m.c))
            m.symmetric = True
        else:
            raise ValueError(f"unknown generator {kind!r}")
        _check(rc, f"ehyb_gen_{kind}")
        m._alive = True
        return m

    # ---- views (valid until reorder()/free())
    @property
    def n(self):
        return self.c.dimension

    @property
    def nnz(self):
        return self.c.totalNum

    def _arr(self, name, count, dtype):
        return _view(getattr(self.c, name), count, dtype)

    @property
    def I(self):
        return self._arr("I", self.nnz, np.int32)

    @property
    def J(self):
        return self._arr("J", self.nnz, np.int32)

    @property
    def V(self):
        return self._arr("V", self.nnz, np.float64)

    @property
    def row_idx(self):
        return self._arr("rowIdx", self.n + 1, np.int32)

    @property
    def num_in_row(self):
        return self._arr("numInRow", self.n, np.int32)

    @property
    def num_in_row2(self):
        return self._arr("numInRow2", self.n, np.int32)

    @property
    def part_boundary(self):
        return self._arr("partBoundary", self.c.nParts + 1, np.int32)

    @property
    def reorder_list(self):
        return self._arr("reorderList", self.n, np.int32)

    def to_scipy(self):
        import scipy.sparse as sp

        return sp.csr_matrix((self.V.copy(), self.J.copy(), self.row_idx.astype(np.int64)), shape=(self.n, self.n))

    # ---- the pre-step (solver_test.c:369-376)
    def reorder(self, cfg=None, symmetric=None):
        """matrixReorder / matrixReorder_unsym (reordering.c:231-378 / 41-228), in place.
        With cfg.n_top > 1 the first partition of every top-level block is kept in self.block_first."""
        sym = self.symmetric if symmetric is None else symmetric
        c = Config.from_buffer_copy(cfg) if cfg is not None else Config()
        c.part_boundary_cap = self.n + 1  # what ehyb_mm_read / ehyb_gen_* / ehyb_matrix_from_csr allocate
        n_top = max(1, int(c.n_top))
        blocks = (C.c_int * (n_top + 1))()
        _check(self.lib.ehyb_matrix_reorder_blocks(C.byref(self.c), 1 if sym else 0, C.byref(c), blocks),
               "ehyb_matrix_reorder")
        self.block_first = [int(b) for b in blocks]
        return self

    def reorder_like(self, other):
        """ehyb_matrix_reorder_like, in place: this matrix, in the ORIGINAL numbering of `other` (a Matrix that has been through
        reorder()), takes other's permutation -- new = other.reorder_list[old], as vector_reorder -- and its partitions, so that a
        Plan of it lives in other's numbering (a mass matrix beside its stiffness matrix).  Build that Plan with sym_pairs=2."""
        _check(self.lib.ehyb_matrix_reorder_like(C.byref(self.c), C.byref(other.c)), "ehyb_matrix_reorder_like")
        return self

    def transposed_like(self, cfg=None):
        """A^T on this matrix's permutation and partitions, for the plan_t of Plan.lsqr.  This matrix has been through reorder():
        its entries are taken back to the original numbering, transposed, and handed to reorder_like(self), so nothing of the
        unpermuted matrix needs to be kept.  Build the plan with symmetric pairs off: Plan(At, make_config(sym_pairs=2, ...))."""
        lst = self.reorder_list.astype(np.int64)
        old_of = np.empty(self.n, dtype=np.int64)
        old_of[lst] = np.arange(self.n)
        rows, cols, vals = old_of[self.J], old_of[self.I], self.V
        order = np.lexsort((cols, rows))
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=self.n))])
        t = Matrix.from_csr(indptr, cols[order], vals[order], cfg, symmetric=False)
        return t.reorder_like(self)

    def reorder_dropin(self):
        """matrixReorder(m) / matrixReorder_unsym(m) exactly as the reference's driver calls them
        (solver_test.c:369-374; the C++-linkage symbols of include/reordering.h): no configuration,
        nParts / vectorCacheSize as the caller left them are only hints."""
        name = "_Z13matrixReorderP10_matrixCOO" if self.symmetric else "_Z19matrixReorder_unsymP10_matrixCOO"
        old = C.cast(self.c.partBoundary, C.c_void_p).value
        if not hasattr(self, "_lib_part_boundary"):
            self._lib_part_boundary = old          # first call: what the reader / generator allocated
        getattr(self.lib, name)(C.byref(self.c))
        # like the reference (reordering.c:44,234) the call mallocs a new partBoundary over the field; the array this
        # library's reader/generator had put there is ours to release
        if old and old == getattr(self, "_lib_part_boundary", None) and old != C.cast(self.c.partBoundary, C.c_void_p).value:
            C.CDLL(None).free(C.c_void_p(old))
        return self

    def key(self):
        """ehyb_matrix_key: digest of the matrix as stored (take it BEFORE reorder() to key a plan cache)."""
        return int(self.lib.ehyb_matrix_key(C.byref(self.c)))

    def append_ghosts(self, n_ghost, gi, gj, gv):
        """Rank-local multi-GPU build: add n_ghost receive-buffer columns and the entries coupling
        to them (ehyb_matrix_append_ghosts)."""
        gi = np.ascontiguousarray(gi, dtype=np.int32)
        gj = np.ascontiguousarray(gj, dtype=np.int32)
        gv = np.ascontiguousarray(gv, dtype=np.float64)
        _check(self.lib.ehyb_matrix_append_ghosts(C.byref(self.c), int(n_ghost), len(gi), _ptr(gi, C.c_int), _ptr(gj, C.c_int),
                                                  _ptr(gv, C.c_double)), "ehyb_matrix_append_ghosts")
        self.symmetric = False
        return self

    def write_mtx(self, path, symmetric_lower_only=False):
        _check(self.lib.ehyb_mm_write(str(path).encode(), C.byref(self.c), int(symmetric_lower_only)), "ehyb_mm_write")

    def free(self):
        if self._alive:
            self.lib.ehyb_matrix_free(C.byref(self.c))
            self._alive = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def vector_reorder(v, reorder_list):
    """vectorReorder (reordering.c:380-384): out[list[i]] = v[i]."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    lst = np.ascontiguousarray(reorder_list, dtype=np.int32)
    out = np.empty_like(v)
    _lib.load().ehyb_vector_reorder(len(v), _ptr(v, C.c_double), _ptr(out, C.c_double), _ptr(lst, C.c_int))
    return out


def entry_order(row_idx_before, reorder_list):
    """ehyb_entry_order: out[k_new] = k_old, the place of every entry of the reordered matrix in the caller's
    arrays before ehyb_matrix_reorder (the V scatter of reordering.c:348-362 as an index list)."""
    rp = np.ascontiguousarray(row_idx_before, dtype=np.int32)
    lst = np.ascontiguousarray(reorder_list, dtype=np.int32)
    n = len(lst)
    assert rp.shape == (n + 1,)
    out = np.empty(int(rp[-1]) - int(rp[0]), dtype=np.int32)
    _check(_lib.load().ehyb_entry_order(n, _ptr(rp, C.c_int), _ptr(lst, C.c_int), _ptr(out, C.c_int32)), "ehyb_entry_order")
    return out


def vector_recover(v_rodr, reorder_list):
    """vectorRecover (reordering.c:386-391): out[i] = v_rodr[list[i]]."""
    v = np.ascontiguousarray(v_rodr, dtype=np.float64)
    lst = np.ascontiguousarray(reorder_list, dtype=np.int32)
    out = np.empty_like(v)
    _lib.load().ehyb_vector_recover(len(v), _ptr(v, C.c_double), _ptr(out, C.c_double), _ptr(lst, C.c_int))
    return out


def partition_graph(indptr, indices, nparts, max_part_rows=0, vwgt=None, cfg=None):
    """ehyb_partition_graph: stands in for MTMETIS_PartGraphKway (reordering.c:280-293)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    n = len(indptr) - 1
    part = np.empty(n, dtype=np.int32)
    cut = C.c_int64(0)
    vw = None if vwgt is None else _ptr(np.ascontiguousarray(vwgt, dtype=np.int32), C.c_int)
    _check(_lib.load().ehyb_partition_graph(n, _ptr(indptr, C.c_int64), _ptr(indices, C.c_int), vw, nparts,
                                            max_part_rows, C.byref(cfg) if cfg else None, _ptr(part, C.c_int),
                                            C.byref(cut)), "ehyb_partition_graph")
    return part, cut.value


class Plan:
    """ehyb_plan: the device-resident EHYB layout of one (permuted) matrix."""

    def __init__(self, matrix, cfg=None, rows=None, upload=True, col_segs=None):
        """col_segs (multi-GPU): first column of every column segment + the dimension (ehyb_plan_create_host_segs);
        the multiply can then run segment by segment (spmv_part)."""
        self.lib = _lib.load()
        self.h = C.c_void_p()
        self.n = matrix.n
        r0, r1 = (0, matrix.n) if rows is None else rows
        self.rows = (r0, r1)
        segs = None if col_segs is None else np.ascontiguousarray(col_segs, dtype=np.int32)
        args = (C.byref(matrix.c), r0, r1, C.byref(cfg) if cfg else None, 0 if segs is None else len(segs) - 1,
                None if segs is None else _ptr(segs, C.c_int), C.byref(self.h))
        if upload:
            # build + upload in one call: what the device can build (cfg.symbolic: the panel form of a residual) is built there
            _check(self.lib.ehyb_plan_create_segs(*args), "ehyb_plan_create_segs")
        else:
            _check(self.lib.ehyb_plan_create_host_segs(*args), "ehyb_plan_create_host_segs")

    def upload(self):
        _check(self.lib.ehyb_plan_upload(self.h), "ehyb_plan_upload")
        return self

    def save(self, path, reorder_list=None, key=0):
        """ehyb_plan_save: the host layout (+ the permutation, + a matrix key) to a cache file."""
        lst = None if reorder_list is None else np.ascontiguousarray(reorder_list, dtype=np.int32)
        assert lst is None or lst.shape == (self.n,)
        _check(self.lib.ehyb_plan_save(self.h, _ptr(lst, C.c_int) if lst is not None else None, key, str(path).encode()),
               "ehyb_plan_save")

    @classmethod
    def load(cls, path, key=0, want_perm=True, upload=True):
        """ehyb_plan_load -> (plan, reorder_list or None); key != 0 must match the file's."""
        self = cls.__new__(cls)
        self.lib = _lib.load()
        self.h = C.c_void_p()
        _check(self.lib.ehyb_plan_load(str(path).encode(), key, C.byref(self.h), None), "ehyb_plan_load")
        st = self.stats
        self.n = st["n_cols"]
        seg = self.array("part_boundary")
        self.rows = (int(seg[0]), int(seg[-1]))
        perm = self.array("perm") if want_perm else None
        if perm is not None and len(perm) == 0:
            perm = None
        if upload:
            self.upload()
        return self, perm

    def check(self):
        """ehyb_plan_check: raises EhybError (code 6, the first array, index and rule named) if a kernel or a host routine
        would index outside one of the plan's arrays; what ehyb_plan_load applies to a file.  Needs no device."""
        _check(self.lib.ehyb_plan_check(self.h), "ehyb_plan_check")
        return self

    @property
    def stats(self):
        st = Stats()
        _check(self.lib.ehyb_plan_stats(self.h, C.byref(st)), "ehyb_plan_stats")
        return st.as_dict()

    @property
    def resident_bytes(self):
        """ehyb_plan_resident_bytes: bytes of the window kernel's value stream read with plain loads (kept in the Infinity Cache)"""
        b = int(self.lib.ehyb_plan_resident_bytes(self.h))
        if b < 0:
            raise EhybError(b, "ehyb_plan_resident_bytes")
        return b

    @property
    def device_value_bytes(self):
        """ehyb_plan_device_value_bytes -> (bytes of the window kernel's value stream, of the CSR residual's values) as the
        device holds them: 8 per value, 4 with cfg.val_f32 = 1"""
        e, r = C.c_int64(0), C.c_int64(0)
        _check(self.lib.ehyb_plan_device_value_bytes(self.h, C.byref(e), C.byref(r)), "ehyb_plan_device_value_bytes")
        return e.value, r.value

    def device_values_f32(self, name):
        """ehyb_plan_device_values_f32: the fp32 stream ehyb_plan_upload sends for "ell_val" or "er_val" (cfg.val_f32 = 1)"""
        which, _ = ARRAYS[name]
        out = np.empty(len(self.array(name)), dtype=np.float32)
        _check(self.lib.ehyb_plan_device_values_f32(self.h, which, _ptr(out, C.c_float), len(out)), "ehyb_plan_device_values_f32")
        return out

    def array(self, name):
        which, dtype = ARRAYS[name]
        p = C.c_void_p()
        cnt = C.c_int64()
        _check(self.lib.ehyb_plan_host_array(self.h, which, C.byref(p), C.byref(cnt)), "ehyb_plan_host_array")
        if cnt.value == 0 or not p.value:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (cnt.value * np.dtype(dtype).itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=cnt.value).copy()

    def spmv(self, x_dev, y_dev, stream=0, phase=0, walk=None):
        """Asynchronous y = A x on device pointers (ints).  walk: None = the plan's own alternation (ehyb_spmv), 0 / 1 = this
        launch walks its streams first to last / last to first (ehyb_spmv_walk)."""
        if walk is not None:
            _check(self.lib.ehyb_spmv_walk(self.h, C.c_void_p(x_dev), C.c_void_p(y_dev), C.c_void_p(stream), int(walk)), "ehyb_spmv_walk")
            return
        _check(self.lib.ehyb_spmv_phase(self.h, C.c_void_p(x_dev), C.c_void_p(y_dev), C.c_void_p(stream), phase),
               "ehyb_spmv")

    def spmv_t(self, x_dev, y_dev, stream=0):
        """Asynchronous y = A^T x on device pointers (ints), on this plan of A (ehyb_spmv_t): y is zeroed in-stream, then every
        contribution is an atomic add.  Raises EhybError (code 1, the form named) on a plan spmv_t_supported refuses."""
        _check(self.lib.ehyb_spmv_t(self.h, C.c_void_p(x_dev), C.c_void_p(y_dev), C.c_void_p(stream)), "ehyb_spmv_t")

    @property
    def spmv_t_supported(self):
        """ehyb_spmv_t_supported: plain storage over all rows with fp64 values and no panel-form residual.  Host only; the reason
        of a False is in ehyb_last_error (spmv_t_refusal)."""
        return self.lib.ehyb_spmv_t_supported(self.h) == 0

    @property
    def spmv_t_refusal(self):
        """(status, message) of ehyb_spmv_t_supported: (0, "") or (1, the form that is not served)"""
        rc = self.lib.ehyb_spmv_t_supported(self.h)
        return rc, (self.lib.ehyb_last_error().decode(errors="replace") if rc else "")

    def launched_t(self):
        """ehyb_debug_launched_t -> the set of rows of kernel_table_t() this plan's transposed launches took since the plan was
        made or launched_clear()"""
        rows = kernel_table_t()
        log = np.zeros(len(rows), dtype=np.uint8)
        _check(self.lib.ehyb_debug_launched_t(self.h, _ptr(log, C.c_uint8), len(log)), "ehyb_debug_launched_t")
        return {rows[i] for i in np.flatnonzero(log)}

    def spmm(self, x_dev, y_dev, k, ldx=None, ldy=None, stream=0, walk=None):
        """Asynchronous Y[:, j] = A X[:, j], j < k, on device pointers (ints; column j at X + j*ldx, Y + j*ldy; None = n) --
        ehyb_spmm: ceil(k / spmm_max_k) passes over the matrix, a panel-form residual's two passes as wide as the window launch.
        walk: None = the plan's own alternation, 0 / 1 explicit."""
        _check(self.lib.ehyb_spmm(self.h, C.c_void_p(x_dev), self.n if ldx is None else int(ldx), C.c_void_p(y_dev),
                                  self.n if ldy is None else int(ldy), int(k), C.c_void_p(stream), -1 if walk is None else int(walk)),
               "ehyb_spmm")

    @property
    def spmm_max_k(self):
        """ehyb_spmm_max_k: the widest k one pass over the matrix serves (1..4; build with lds_doubles = 20480 // k for k; a plan
        whose residual is in panel form -- stats["er_partials"] > 0 -- with er_panel_cols = 16384 // k, and lds_doubles as well
        where it keeps windows)."""
        k = C.c_int(0)
        _check(self.lib.ehyb_spmm_max_k(self.h, C.byref(k)), "ehyb_spmm_max_k")
        return k.value

    def graph(self, x_dev, y_dev, multiplies=1):
        """ehyb_spmv_graph_create: `multiplies` multiplies captured into a hipGraph that keeps the alternating walk -> SpmvGraph"""
        return SpmvGraph(self, x_dev, y_dev, multiplies)

    def tune(self, x_dev, y_dev, reps=5):
        """ehyb_plan_tune: the heaviest work items on the XCDs measured fastest -> (launch span before, after) in us."""
        a, b = C.c_double(0), C.c_double(0)
        _check(self.lib.ehyb_plan_tune(self.h, C.c_void_p(x_dev), C.c_void_p(y_dev), reps, C.byref(a), C.byref(b)), "ehyb_plan_tune")
        return a.value, b.value

    def item_map(self):
        """ehyb_debug_item_map -> (the item every workgroup of the window launch takes, True if the plan holds a map of its own:
        a tuned or a set one; False: the built-in order).  Host only."""
        n, inst = C.c_int(0), C.c_int(0)
        _check(self.lib.ehyb_debug_item_map(self.h, None, 0, C.byref(n), C.byref(inst)), "ehyb_debug_item_map")
        out = np.zeros(n.value, dtype=np.int32)
        if n.value:
            _check(self.lib.ehyb_debug_item_map(self.h, _ptr(out, C.c_int32), len(out), C.byref(n), C.byref(inst)), "ehyb_debug_item_map")
        return out, bool(inst.value)

    def set_item_map(self, map, strict=True):
        """ehyb_debug_set_item_map: workgroup b takes item map[b] from now on (None: the built-in order again).  strict=False
        allows repeated and missing items: products are then wrong by design."""
        if map is None:
            _check(self.lib.ehyb_debug_set_item_map(self.h, None, 0, int(strict)), "ehyb_debug_set_item_map")
            return
        m = np.ascontiguousarray(map, dtype=np.int32)
        _check(self.lib.ehyb_debug_set_item_map(self.h, _ptr(m, C.c_int32), len(m), int(strict)), "ehyb_debug_set_item_map")

    def launched(self):
        """ehyb_debug_launched -> {"window" / "panel" / "er_csr": set of the rows of kernel_table() this plan's launches took since
        the plan was made or launched_clear()}, each row a tuple of the table's fields"""
        out = {}
        for which, name in enumerate(KERNEL_TABLES):
            rows = kernel_table(name)
            log = np.zeros(len(rows), dtype=np.uint8)
            _check(self.lib.ehyb_debug_launched(self.h, which, _ptr(log, C.c_uint8), len(log)), "ehyb_debug_launched")
            out[name] = {rows[i] for i in np.flatnonzero(log)}
        return out

    def launched_clear(self):
        _check(self.lib.ehyb_debug_launched_clear(self.h), "ehyb_debug_launched_clear")

    def spmv_part(self, x_dev, y_dev, stream, seg_begin, seg_end, flags):
        """ehyb_spmv_part: flags 1 = the ELL launch first, 2 = the closing pass, 4 = the closing pass over the rows from cfg.row_split
        on (EHYB_PART_FIRST / _LAST / _LAST_FOREIGN).  A refused call has enqueued nothing."""
        _check(self.lib.ehyb_spmv_part(self.h, C.c_void_p(x_dev), C.c_void_p(y_dev), C.c_void_p(stream), seg_begin, seg_end, flags),
               "ehyb_spmv_part")

    @property
    def col_segs(self):
        n = C.c_int(0)
        _check(self.lib.ehyb_plan_col_segs(self.h, C.byref(n)), "ehyb_plan_col_segs")
        return n.value

    def spmv_host(self, x, iters=1):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (self.n,)
        y = np.zeros(self.n, dtype=np.float64)
        _check(self.lib.ehyb_spmv_host(self.h, _ptr(x, C.c_double), _ptr(y, C.c_double), iters), "ehyb_spmv_host")
        return y

    def set_values(self, values, entry_order=None, stream=0):
        """ehyb_plan_set_values: the numeric phase of the build again, on the device, for new values on the
        plan's pattern (needs cfg.value_map = 1).  values / entry_order: numpy arrays (host) or, both of them,
        device pointers given as (ptr, count) tuples."""
        if isinstance(values, tuple):
            ptr, count = values
            order = None if entry_order is None else C.c_void_p(entry_order[0])
            _check(self.lib.ehyb_plan_set_values(self.h, C.c_void_p(ptr), count, order, 1, C.c_void_p(stream)), "ehyb_plan_set_values")
            return
        v = np.ascontiguousarray(values, dtype=np.float64)
        o = None if entry_order is None else np.ascontiguousarray(entry_order, dtype=np.int32)
        assert o is None or o.shape == v.shape
        _check(self.lib.ehyb_plan_set_values(self.h, v.ctypes.data_as(C.c_void_p), len(v), o.ctypes.data_as(C.c_void_p) if o is not None else None,
                                             0, C.c_void_p(stream)), "ehyb_plan_set_values")

    def bench(self, x_dev, y_dev, stream=0, warmup=10, iters=100, per_kernel=True):
        t, e, r = C.c_double(), C.c_double(), C.c_double()
        _check(self.lib.ehyb_spmv_bench(self.h, C.c_void_p(x_dev), C.c_void_p(y_dev), C.c_void_p(stream), warmup, iters,
                                        C.byref(t), C.byref(e) if per_kernel else None,
                                        C.byref(r) if per_kernel else None), "ehyb_spmv_bench")
        return {"ms_total": t.value, "ms_ell_avg": e.value, "ms_er_avg": r.value}

    def _solve(self, name, B, X0, inv_diag, scalars, stream=0, allow_breakdown=False, multi=False, inner=None, counters=None, diag=True):
        """One call of the solver `name`: B, X0 (zeros if None) and the optional inv_diag staged on the device; the arguments in
        the one-vector shape or (multi) the (ldb, ldx, k) one, `scalars` between the vectors and the stream; `inner`: the second
        plan of ehyb_pcg_refine, which also reports two integer counters instead of one, or of ehyb_pcg_cheb (counters=1).  A
        failure raises EhybError, unless
        allow_breakdown and the error text says breakdown.  diag=False: the solver takes no inv_diag argument (ehyb_pcg_fsai).  -> (X, counters ...): scalars from a one-vector call, (k,) arrays
        and X (k, n) from a multi one."""
        n, k = self.n, 1
        B = np.ascontiguousarray(np.atleast_2d(B) if multi else B, dtype=np.float64)
        if multi:
            k, nb = B.shape
            assert nb == n, (nb, n)
            X0 = None if X0 is None else np.ascontiguousarray(X0, dtype=np.float64).reshape(k, n)
        db = DeviceBuffer(k * n).upload(B.ravel())
        dx = DeviceBuffer(k * n).upload(np.zeros(k * n) if X0 is None else np.ravel(X0))
        dd = None if inv_diag is None else DeviceBuffer(n).upload(inv_diag)
        counts, rel = np.zeros((counters or (1 if inner is None else 2), k), dtype=np.int32), np.zeros(k, dtype=np.float64)
        vectors = (C.c_void_p(db.ptr), n, C.c_void_p(dx.ptr), n, k) if multi else (C.c_void_p(db.ptr), C.c_void_p(dx.ptr))
        rc = getattr(self.lib, name)(self.h, *(() if inner is None else (inner.h,)), *((C.c_void_p(dd.ptr) if dd else None,) if diag else ()), *vectors,
                                     *scalars, C.c_void_p(stream), *(_ptr(c, C.c_int) for c in counts), _ptr(rel, C.c_double))
        if rc != 0 and not (allow_breakdown and b"breakdown" in self.lib.ehyb_last_error()):
            raise EhybError(rc, name)
        if multi:
            return dx.download().reshape(k, n), counts[0], rel
        return (dx.download(), *(int(c[0]) for c in counts), float(rel[0]))

    def cg(self, b, x0=None, max_iter=1000, rtol=1e-10, check_every=10, inv_diag=None):
        """ehyb_cg / ehyb_pcg: (Jacobi-preconditioned if inv_diag is given) conjugate gradients on the
        device; b, x, inv_diag in the permuted numbering.  -> (x, iterations, relative residual)"""
        return self._solve("ehyb_pcg", b, x0, inv_diag, (max_iter, rtol, check_every))

    def cg_multi(self, B, X0=None, max_iter=1000, rtol=1e-10, check_every=10, inv_diag=None, allow_breakdown=False, stream=0):
        """ehyb_cg_multi / ehyb_pcg_multi: k independent (Jacobi-preconditioned if inv_diag is given) CG solves that share every
        multiply; B, X0 (k, n) in the permuted numbering, column j solved as cg(B[j]) would.  -> (X (k, n), iterations (k,),
        relative residuals (k,)).  A breakdown raises EhybError, unless allow_breakdown: then the broken columns report NaN.
        The multiplies are as wide as spmm_max_k allows -- on a panel-form plan too, when it was built with er_panel_cols = 16384 // k."""
        return self._solve("ehyb_pcg_multi", B, X0, inv_diag, (max_iter, rtol, check_every), stream, allow_breakdown, multi=True)

    def pcg_refine(self, inner_plan, b, x0=None, max_outer=10, inner_max_iter=1000, rtol=1e-12, inner_rtol=1e-6, inv_diag=None, stream=0):
        """ehyb_pcg_refine: iterative refinement -- residuals and updates in fp64 on this plan, the corrections from ehyb_pcg on
        inner_plan (normally the cfg.val_f32 plan of the same reordered matrix).  -> (x, outer steps, inner iterations in all,
        relative residual ||b - A x|| / ||b|| on this plan); a run that stagnates returns normally: compare the residual with rtol."""
        return self._solve("ehyb_pcg_refine", b, x0, inv_diag, (max_outer, inner_max_iter, rtol, inner_rtol), stream, inner=inner_plan)

    def lambda_max(self, inv_diag=None, iters=20, stream=0):
        """ehyb_lambda_max: the Rayleigh quotient after `iters` steps of the power method on D^-1 A (inv_diag in the permuted
        numbering; None: on A) -- an estimate of the largest eigenvalue from below."""
        dd = None if inv_diag is None else DeviceBuffer(self.n).upload(inv_diag)
        lam = C.c_double(0)
        _check(self.lib.ehyb_lambda_max(self.h, C.c_void_p(dd.ptr) if dd else None, int(iters), C.c_void_p(stream), C.byref(lam)),
               "ehyb_lambda_max")
        return lam.value

    def cg_cheb(self, b, degree, poly_plan=None, lmin=0.0, lmax=0.0, x0=None, max_iter=1000, rtol=1e-10, check_every=10, inv_diag=None,
                allow_breakdown=False, stream=0):
        """ehyb_pcg_cheb: CG on this plan, preconditioned with a Chebyshev polynomial of `degree` in D^-1 A evaluated on
        poly_plan (None: this plan; intended: the cfg.val_f32 plan of the same reordered matrix).  lmax <= 0: estimated
        (1.1 * lambda_max on poly_plan), lmin <= 0: lmax / 30; lmax must be an upper bound of the spectrum of D^-1 A.
        -> (x, iterations, relative residual).  A breakdown raises EhybError, unless allow_breakdown: then the residual is NaN."""
        return self._solve("ehyb_pcg_cheb", b, x0, inv_diag, (int(degree), lmin, lmax, max_iter, rtol, check_every), stream, allow_breakdown,
                           inner=poly_plan or self, counters=1)

    def cg_cheb_multi(self, B, degree, poly_plan=None, lmin=0.0, lmax=0.0, X0=None, max_iter=1000, rtol=1e-10, check_every=10,
                      inv_diag=None, allow_breakdown=False, stream=0):
        """ehyb_pcg_cheb_multi: k independent cg_cheb solves that share every multiply; B, X0 (k, n), column j solved as
        cg_cheb(B[j]) would -- with plain storage bit for bit.  -> (X (k, n), iterations (k,), relative residuals (k,)).  The
        multiplies are as wide as spmm_max_k of each plan allows: a cfg.val_f32 poly_plan runs passes of width 1."""
        return self._solve("ehyb_pcg_cheb_multi", B, X0, inv_diag, (int(degree), lmin, lmax, max_iter, rtol, check_every), stream,
                           allow_breakdown, multi=True, inner=poly_plan or self, counters=1)

    def cg_coarse(self, b, coarse, x0=None, max_iter=1000, rtol=1e-10, check_every=10, inv_diag=None, allow_breakdown=False, stream=0):
        """ehyb_pcg_coarse: CG on this plan with the two-level preconditioner z = inv_diag .* r + P E^-1 P^T r of `coarse` (a Coarse
        of the reordered matrix this plan was built from).  -> (x, iterations, relative residual).  A breakdown raises
        EhybError, unless allow_breakdown: then the residual is NaN."""
        return self._solve("ehyb_pcg_coarse", b, x0, inv_diag, (max_iter, rtol, check_every), stream, allow_breakdown, inner=coarse, counters=1)

    def cg_coarse_multi(self, B, coarse, X0=None, max_iter=1000, rtol=1e-10, check_every=10, inv_diag=None, allow_breakdown=False, stream=0):
        """ehyb_pcg_coarse_multi: k independent cg_coarse solves that share every multiply; B, X0 (k, n), column j solved as
        cg_coarse(B[j]) would -- with plain storage bit for bit.  -> (X (k, n), iterations (k,), relative residuals (k,))."""
        return self._solve("ehyb_pcg_coarse_multi", B, X0, inv_diag, (max_iter, rtol, check_every), stream, allow_breakdown, multi=True,
                           inner=coarse, counters=1)

    def cg_fsai(self, b, fsai, x0=None, max_iter=1000, rtol=1e-10, check_every=10, allow_breakdown=False, stream=0):
        """ehyb_pcg_fsai: CG on this plan with the preconditioner z = G^T (G r) of `fsai` (an Fsai of the reordered matrix this plan
        was built from; there is no inv_diag: G carries the scaling).  -> (x, iterations, relative residual).  A breakdown raises
        EhybError, unless allow_breakdown: then the residual is NaN."""
        return self._solve("ehyb_pcg_fsai", b, x0, None, (max_iter, rtol, check_every), stream, allow_breakdown, inner=fsai, counters=1, diag=False)

    def cg_fsai_multi(self, B, fsai, X0=None, max_iter=1000, rtol=1e-10, check_every=10, allow_breakdown=False, stream=0):
        """ehyb_pcg_fsai_multi: k independent cg_fsai solves that share every multiply; B, X0 (k, n), column j solved as
        cg_fsai(B[j]) would -- with plain storage and transpose="plan" bit for bit.  -> (X (k, n), iterations (k,), relative
        residuals (k,))."""
        return self._solve("ehyb_pcg_fsai_multi", B, X0, None, (max_iter, rtol, check_every), stream, allow_breakdown, multi=True, inner=fsai,
                           counters=1, diag=False)

    def cg_bic(self, b, bic, x0=None, max_iter=1000, rtol=1e-10, check_every=10, allow_breakdown=False, stream=0):
        """ehyb_pcg_bic: CG on this plan with the block incomplete Cholesky preconditioner z = P^T (L L^T)^-1 P r of `bic` (a Bic of
        the reordered matrix this plan was built from; there is no inv_diag: L carries the scaling).  -> (x, iterations, relative
        residual).  A breakdown raises EhybError, unless allow_breakdown: then the residual is NaN."""
        return self._solve("ehyb_pcg_bic", b, x0, None, (max_iter, rtol, check_every), stream, allow_breakdown, inner=bic, counters=1, diag=False)

    def cg_bic_multi(self, B, bic, X0=None, max_iter=1000, rtol=1e-10, check_every=10, allow_breakdown=False, stream=0):
        """ehyb_pcg_bic_multi: k independent cg_bic solves that share every multiply; B, X0 (k, n), column j solved as cg_bic(B[j])
        would -- with plain storage bit for bit.  -> (X (k, n), iterations (k,), relative residuals (k,))."""
        return self._solve("ehyb_pcg_bic_multi", B, X0, None, (max_iter, rtol, check_every), stream, allow_breakdown, multi=True, inner=bic,
                           counters=1, diag=False)

    def bicgstab(self, b, x0=None, max_iter=1000, rtol=1e-10, check_every=10, inv_diag=None, allow_breakdown=False, stream=0):
        """ehyb_bicgstab: BiCGSTAB for an unsymmetric system on the device, right Jacobi-preconditioned if inv_diag is given;
        b, x0, inv_diag in the permuted numbering.  -> (x, iterations, relative residual).  A breakdown raises EhybError,
        unless allow_breakdown: then x is the last good iterate and the counts are those of the device."""
        return self._solve("ehyb_bicgstab", b, x0, inv_diag, (max_iter, rtol, check_every), stream, allow_breakdown)

    def bicgstab_multi(self, B, X0=None, max_iter=1000, rtol=1e-10, check_every=10, inv_diag=None, allow_breakdown=False, stream=0):
        """ehyb_bicgstab_multi: k independent BiCGSTAB solves (right Jacobi-preconditioned if inv_diag is given) that share both
        multiplies of every iteration; B, X0 (k, n) in the permuted numbering, column j solved as bicgstab(B[j]) would -- with
        plain storage bit for bit.  -> (X (k, n), iterations (k,), relative residuals (k,)), the counts those of the device.  A
        breakdown in any column raises EhybError, unless allow_breakdown: then a broken column holds its last good iterate.
        The multiplies are as wide as spmm_max_k allows (build the plan with lds_doubles = 20480 // k)."""
        return self._solve("ehyb_bicgstab_multi", B, X0, inv_diag, (max_iter, rtol, check_every), stream, allow_breakdown, multi=True)

    def bicgstab_bilu(self, b, bilu, x0=None, max_iter=1000, rtol=1e-10, check_every=10, allow_breakdown=False, stream=0):
        """ehyb_bicgstab_bilu: bicgstab right-preconditioned with the block ILU(0) z = P^T (L U)^-1 P r of `bilu` (a Bilu of the
        reordered matrix this plan was built from) instead of the diagonal.  -> (x, iterations, relative residual), breakdowns as
        bicgstab."""
        return self._solve("ehyb_bicgstab_bilu", b, x0, None, (max_iter, rtol, check_every), stream, allow_breakdown, inner=bilu, counters=1, diag=False)

    def bicgstab_bilu_multi(self, B, bilu, X0=None, max_iter=1000, rtol=1e-10, check_every=10, allow_breakdown=False, stream=0):
        """ehyb_bicgstab_bilu_multi: k independent bicgstab_bilu solves that share both multiplies and both applies of every
        iteration; B, X0 (k, n), column j solved as bicgstab_bilu(B[j]) would -- with plain storage bit for bit.  -> (X (k, n),
        iterations (k,), relative residuals (k,))."""
        return self._solve("ehyb_bicgstab_bilu_multi", B, X0, None, (max_iter, rtol, check_every), stream, allow_breakdown, multi=True, inner=bilu,
                           counters=1, diag=False)

    def gmres_bilu(self, b, bilu, x0=None, restart=30, ortho_passes=2, max_iter=1000, rtol=1e-10, allow_breakdown=False, stream=0):
        """ehyb_gmres_bilu: gmres right-preconditioned with the block ILU(0) of `bilu` (a Bilu of the reordered matrix this plan was
        built from) instead of the diagonal.  -> (x, steps, relative residual), breakdowns as gmres."""
        return self._solve("ehyb_gmres_bilu", b, x0, None, (int(restart), int(ortho_passes), max_iter, rtol), stream, allow_breakdown, inner=bilu,
                           counters=1, diag=False)

    def minres(self, b, x0=None, max_iter=1000, rtol=1e-10, check_every=10, inv_diag=None, allow_breakdown=False, stream=0):
        """ehyb_minres: MINRES for a symmetric, possibly indefinite system on the device; inv_diag: an optional POSITIVE
        diagonal preconditioner (minres_inv_diag gives 1 / |a_ii|); b, x0, inv_diag in the permuted numbering.
        -> (x, iterations, relative residual phibar / sqrt(b.M^-1 b)).  A breakdown raises EhybError, unless allow_breakdown:
        then x is the last good iterate and the counts are those of the device."""
        return self._solve("ehyb_minres", b, x0, inv_diag, (max_iter, rtol, check_every), stream, allow_breakdown)

    def minres_multi(self, B, X0=None, max_iter=1000, rtol=1e-10, check_every=10, inv_diag=None, allow_breakdown=False, stream=0):
        """ehyb_minres_multi: k independent MINRES solves that share the multiply of every iteration; B, X0 (k, n) in the
        permuted numbering, column j solved as minres(B[j]) would -- with plain storage bit for bit.  -> (X (k, n), iterations
        (k,), relative residuals (k,)), the counts those of the device.  A breakdown in any column raises EhybError, unless
        allow_breakdown: then a broken column holds its last good iterate."""
        return self._solve("ehyb_minres_multi", B, X0, inv_diag, (max_iter, rtol, check_every), stream, allow_breakdown, multi=True)

    def _lsqr(self, name, B, plan_t, X0, scalars, stream, allow_breakdown, multi):
        n, k = self.n, 1
        B = np.ascontiguousarray(np.atleast_2d(B) if multi else B, dtype=np.float64)
        if multi:
            k, nb = B.shape
            assert nb == n, (nb, n)
        db = DeviceBuffer(k * n).upload(B.ravel())
        dx = DeviceBuffer(k * n).upload(np.zeros(k * n) if X0 is None else np.ascontiguousarray(X0, dtype=np.float64).ravel())
        info = (_lib.LsqrInfo * k)()
        vectors = (C.c_void_p(db.ptr), n, C.c_void_p(dx.ptr), n, k) if multi else (C.c_void_p(db.ptr), C.c_void_p(dx.ptr))
        rc = getattr(self.lib, name)(self.h, plan_t.h if plan_t is not None else None, *vectors, *scalars, C.c_void_p(stream), info)
        if rc != 0 and not (allow_breakdown and b"breakdown" in self.lib.ehyb_last_error()):
            raise EhybError(rc, name)
        out = [i.as_dict() for i in info]
        return (dx.download().reshape(k, n), out) if multi else (dx.download(), out[0])

    def lsqr(self, b, plan_t=None, x0=None, damp=0.0, atol=1e-10, btol=1e-10, max_iter=1000, check_every=10, allow_breakdown=False,
             stream=0):
        """ehyb_lsqr: LSQR for min ||b - A x||_2 (damp > 0: + damp^2 ||x - x0||^2) on the device; a rectangular matrix goes in
        padded square (pad_square), b padded with zeros.  plan_t: a Plan of A^T in this plan's numbering (Matrix.transposed_like),
        this plan itself for a symmetric A, or None: every A^T multiply is spmv_t on this plan (reproducible up to the order of
        summation only; raises EhybError, code 1, on a plan spmv_t_supported refuses).  b, x0 in the permuted numbering.
        -> (x, info) with info = {"istop", "iters", "rnorm", "arnorm", "anorm", "xnorm"}; istop 0 = x0 already solves, 1 / 2 = the
        stop test that held, 7 = max_iter, -1 = breakdown.  A breakdown raises EhybError, unless allow_breakdown: then x is the
        last good iterate."""
        return self._lsqr("ehyb_lsqr", b, plan_t, x0, (damp, atol, btol, max_iter, check_every), stream, allow_breakdown, False)

    def lsqr_multi(self, B, plan_t=None, X0=None, damp=0.0, atol=1e-10, btol=1e-10, max_iter=1000, check_every=10, allow_breakdown=False,
                   stream=0):
        """ehyb_lsqr_multi: k independent LSQR solves that share both multiplies of every iteration; B, X0 (k, n) in the permuted
        numbering, column j solved as lsqr(B[j]) would -- with a plan_t in plain storage bit for bit.  -> (X (k, n), list of k
        info dicts).  A breakdown in any column raises EhybError, unless allow_breakdown."""
        return self._lsqr("ehyb_lsqr_multi", B, plan_t, X0, (damp, atol, btol, max_iter, check_every), stream, allow_breakdown, True)

    def gmres(self, b, x0=None, restart=30, ortho_passes=2, max_iter=1000, rtol=1e-10, inv_diag=None, allow_breakdown=False, stream=0):
        """ehyb_gmres: restarted GMRES(restart) for an unsymmetric system on the device, right Jacobi-preconditioned if inv_diag
        is given -- for the systems on which bicgstab breaks down or diverges; restart 0 = 30, at most 64; ortho_passes 1 or 2
        (classical Gram-Schmidt once or twice); b, x0, inv_diag in the permuted numbering.  -> (x, iterations, relative
        residual).  A breakdown raises EhybError, unless allow_breakdown: then x is the last good iterate and the counts are
        those of the device."""
        return self._solve("ehyb_gmres", b, x0, inv_diag, (int(restart), int(ortho_passes), max_iter, rtol), stream, allow_breakdown)

    def gmres_t(self, b, x0=None, restart=30, ortho_passes=2, max_iter=1000, rtol=1e-10, inv_diag=None, allow_breakdown=False, stream=0):
        """ehyb_gmres_t: gmres for the adjoint system A^T x = b on this plan of A (every multiply a spmv_t); arguments and
        results as gmres, inv_diag the same vector (A^T has A's diagonal).  Reproducible up to the order of summation only.
        Raises EhybError (code 1) before any launch on a plan spmv_t_supported refuses."""
        return self._solve("ehyb_gmres_t", b, x0, inv_diag, (int(restart), int(ortho_passes), max_iter, rtol), stream, allow_breakdown)

    def eigsh(self, nev, which="LA", basis=0, max_restarts=300, tol=1e-10, scale=None, v0=None, vectors=True, allow_breakdown=False,
              stream=0):
        """ehyb_eigsh: the nev (1 .. 16) largest ("LA") or smallest ("SA") algebraic eigenvalues of the plan's symmetric matrix
        and their eigenvectors by thick-restart Lanczos on the device; with `scale` of S A S, S = diag(scale).  basis 0 =
        min(max(2 nev + 1, 20), 64), at most 64; scale, v0 (None: the start vector of lambda_max) and the vectors in the
        permuted numbering.  -> (evals (found,), evecs (found, n) or None, info) with info = {"found", "nconv", "multiplies",
        "restarts", "resid" (found,)}; nconv < found means max_restarts ran out.  A multiple eigenvalue is found once.  A
        breakdown (a non-finite quantity) raises EhybError, unless allow_breakdown: then found = nconv = 0 and evals, evecs are empty."""
        n, nev = self.n, int(nev)
        ldv = n + (n & 1)
        ds = None if scale is None else DeviceBuffer(n).upload(scale)
        d0 = None if v0 is None else DeviceBuffer(n).upload(v0)
        dv = None
        if vectors:
            dv = DeviceBuffer(max(nev, 1) * ldv).upload(np.zeros(max(nev, 1) * ldv))
        evals, resid = np.zeros(max(nev, 1)), np.zeros(max(nev, 1))
        found, nconv, mult, rest = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        rc = self.lib.ehyb_eigsh(self.h, C.c_void_p(ds.ptr) if ds else None, C.c_void_p(d0.ptr) if d0 else None, nev,
                                 {"LA": 0, "SA": 1}[which], int(basis), int(max_restarts), tol, _ptr(evals, C.c_double),
                                 C.c_void_p(dv.ptr) if dv else None, ldv, C.c_void_p(stream), C.byref(found), C.byref(nconv),
                                 C.byref(mult), C.byref(rest), _ptr(resid, C.c_double))
        if rc != 0 and not (allow_breakdown and b"breakdown" in self.lib.ehyb_last_error()):
            raise EhybError(rc, "ehyb_eigsh")
        f = found.value
        info = {"found": f, "nconv": nconv.value, "multiplies": mult.value, "restarts": rest.value, "resid": resid[:f].copy()}
        X = dv.download().reshape(-1, ldv)[:f, :n].copy() if dv else None
        return evals[:f].copy(), X, info

    def svds(self, nsv, plan_t=None, basis=0, max_restarts=300, tol=1e-10, v0=None, vectors=True, allow_breakdown=False, stream=0):
        """ehyb_svds: the nsv (1 .. 16) largest singular values of the plan's matrix with their left and right singular vectors,
        by thick-restart Golub-Kahan-Lanczos bidiagonalisation on the device; a rectangular matrix goes in padded square
        (pad_square).  plan_t as in lsqr: a Plan of A^T in this plan's numbering (Matrix.transposed_like), this plan itself for a
        symmetric A, or None: every A^T multiply is spmv_t on this plan (reproducible up to the order of summation only).  basis
        0 = min(max(2 nsv + 1, 20), 64), at most 64; v0 (None: the start vector of eigsh) and the vectors in the permuted numbering.
        -> (s (found,) falling, U (found, n), V (found, n) or None with vectors=False, info) with info = {"found", "nconv",
        "multiplies" (A and A^T together), "restarts", "resid" (found,), "status" ("ok" or "breakdown")}; A V[i] = s[i] U[i] by
        construction and resid[i] estimates ||A^T U[i] - s[i] V[i]||; nconv < found means max_restarts ran out; found < nsv means
        the matrix has no more (a multiple sigma is found once).  The smallest singular values are out of reach of this method.  A
        breakdown (a non-finite quantity) raises EhybError, unless allow_breakdown: then found = nconv = 0 and s, U, V are empty."""
        n, nsv = self.n, int(nsv)
        ld = n + (n & 1)
        d0 = None if v0 is None else DeviceBuffer(n).upload(v0)
        du = dv = None
        if vectors:
            du = DeviceBuffer(max(nsv, 1) * ld).upload(np.zeros(max(nsv, 1) * ld))
            dv = DeviceBuffer(max(nsv, 1) * ld).upload(np.zeros(max(nsv, 1) * ld))
        svals, resid = np.zeros(max(nsv, 1)), np.zeros(max(nsv, 1))
        found, nconv, mult, rest = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        rc = self.lib.ehyb_svds(self.h, plan_t.h if plan_t is not None else None, C.c_void_p(d0.ptr) if d0 else None, nsv, int(basis),
                                int(max_restarts), tol, _ptr(svals, C.c_double), C.c_void_p(du.ptr) if du else None, ld,
                                C.c_void_p(dv.ptr) if dv else None, ld, C.c_void_p(stream), C.byref(found), C.byref(nconv), C.byref(mult),
                                C.byref(rest), _ptr(resid, C.c_double))
        broke = rc != 0 and b"breakdown" in self.lib.ehyb_last_error()
        if rc != 0 and not (allow_breakdown and broke):
            raise EhybError(rc, "ehyb_svds")
        f = found.value
        info = {"found": f, "nconv": nconv.value, "multiplies": mult.value, "restarts": rest.value, "resid": resid[:f].copy(),
                "status": "breakdown" if broke else "ok"}
        U = du.download().reshape(-1, ld)[:f, :n].copy() if du else None
        V = dv.download().reshape(-1, ld)[:f, :n].copy() if dv else None
        return svals[:f].copy(), U, V, info

    def norm2(self, plan_t=None, tol=1e-6, stream=0):
        """An estimate of ||A||_2: sigma_0 of svds(1) at relative residual tol.  It is a Ritz value, which approaches ||A||_2 FROM
        INSIDE: never above ||A||_2 in exact arithmetic and below it by at most about tol^2 ||A||_2 once converged.  A caller that
        needs an upper bound widens it.  0.0 for a zero matrix."""
        s = self.svds(1, plan_t=plan_t, tol=tol, vectors=False, stream=stream)[0]
        return float(s[0]) if len(s) else 0.0

    def lobpcg(self, nev, block=0, coarse=None, inv_diag=None, X0=None, max_iter=500, tol=1e-8, anorm=0.0, vectors=True,
               allow_breakdown=False, stream=0):
        """ehyb_lobpcg: the nev (1 .. 8) smallest eigenpairs of the plan's symmetric matrix by LOBPCG on the device, with a block
        of `block` vectors (0: nev) -- a block finds the copies of a multiple eigenvalue, which eigsh finds once.  Preconditioner:
        `coarse` (a Coarse of the reordered matrix, with inv_diag as in cg_coarse), inv_diag alone (Jacobi) or none.  X0 (block, n)
        or None (the start block of the header); inv_diag, X0 and the vectors in the permuted numbering.  A column has converged
        when ||A x - theta x|| <= tol * max(max |theta|, anorm).  -> (evals (nev,), X (nev, n) or None, info) with info = {"nconv",
        "iters", "multiplies", "resid" (nev,)}; nconv < nev means max_iter ran out.  A breakdown (a non-finite quantity, a basis
        of rank < block) raises EhybError, unless allow_breakdown: then nconv = 0 and evals, resid are NaN.  On a matrix whose
        lowest eigenvalues are well separated eigsh(nev, "SA") needs fewer multiplies."""
        return self._lobpcg("ehyb_lobpcg", ("nconv", "iters", "multiplies"), nev, block, inv_diag, X0, vectors, allow_breakdown,
                            lambda dd, d0, ld, evals, dv, counts, resid: self.lib.ehyb_lobpcg(
                                self.h, coarse.h if coarse is not None else None, dd, d0, ld, int(nev), int(block), int(max_iter), tol, anorm,
                                evals, dv, ld, C.c_void_p(stream), *counts, resid))

    def lobpcg_gen(self, nev, mass, block=0, coarse=None, inv_diag=None, X0=None, max_iter=500, tol=1e-8, anorm=0.0, bnorm=0.0,
                   vectors=True, allow_breakdown=False, stream=0):
        """ehyb_lobpcg_gen: the nev smallest eigenpairs of K x = lambda M x, K this plan's symmetric matrix.  `mass` is an uploaded
        Plan of the consistent mass matrix in this plan's numbering (Matrix.reorder_like) or a length-n array, the lumped mass
        diagonal in the permuted numbering.  Everything else as lobpcg(), except: a column has converged when
        ||K x - theta M x|| <= tol * max(bnorm * max |theta|, anorm) with bnorm the caller's scale of ||M|| (0: 1), the vectors
        come out with X M X^T = I, and info gains "mass_multiplies" (0 for a lumped mass)."""
        mass_plan = mass if isinstance(mass, Plan) else None
        dm = None
        if mass_plan is None:
            mass = np.ascontiguousarray(mass, dtype=np.float64)
            assert mass.shape == (self.n,), (mass.shape, self.n)
            dm = DeviceBuffer(self.n).upload(mass)
        return self._lobpcg("ehyb_lobpcg_gen", ("nconv", "iters", "multiplies", "mass_multiplies"), nev, block, inv_diag, X0, vectors,
                            allow_breakdown, lambda dd, d0, ld, evals, dv, counts, resid: self.lib.ehyb_lobpcg_gen(
                                self.h, mass_plan.h if mass_plan is not None else None, C.c_void_p(dm.ptr) if dm else None,
                                coarse.h if coarse is not None else None, dd, d0, ld, int(nev), int(block), int(max_iter), tol, anorm, bnorm,
                                evals, dv, ld, C.c_void_p(stream), *counts, resid))

    def _lobpcg(self, who, counters, nev, block, inv_diag, X0, vectors, allow_breakdown, call):
        """what lobpcg() and lobpcg_gen() share: inv_diag and X0 (padded to an even leading dimension) on the device, the buffer of the
        vectors, the counters, call(inv_diag, X0, ld, evals, vectors, the counters by reference, resid) -> rc, the breakdown rule and
        the download -> (evals, X or None, info with the counters in their order and "resid")"""
        n, nev = self.n, int(nev)
        nb = nev if int(block) == 0 else int(block)
        ld = n + (n & 1)
        dd = None if inv_diag is None else DeviceBuffer(n).upload(inv_diag)
        d0 = None
        if X0 is not None:
            X0 = np.ascontiguousarray(X0, dtype=np.float64)
            assert X0.shape == (nb, n), (X0.shape, nb, n)
            padded = np.zeros((nb, ld))
            padded[:, :n] = X0
            d0 = DeviceBuffer(nb * ld).upload(padded.ravel())
        dv = DeviceBuffer(max(nev, 1) * ld).upload(np.zeros(max(nev, 1) * ld)) if vectors else None
        evals, resid = np.zeros(max(nev, 1)), np.zeros(max(nev, 1))
        counts = {name: C.c_int(0) for name in counters}
        rc = call(*(C.c_void_p(b.ptr) if b else None for b in (dd, d0)), ld, _ptr(evals, C.c_double), C.c_void_p(dv.ptr) if dv else None,
                  [C.byref(c) for c in counts.values()], _ptr(resid, C.c_double))
        if rc != 0 and not (allow_breakdown and b"breakdown" in self.lib.ehyb_last_error()):
            raise EhybError(rc, who)
        info = {name: c.value for name, c in counts.items()}
        info["resid"] = resid[:nev].copy()
        X = dv.download().reshape(-1, ld)[:nev, :n].copy() if dv else None
        return evals[:nev].copy(), X, info

    def spectrum_bounds(self, inv_diag=None, tol=1e-4, stream=0):
        """(lmin, lmax) of D^-1 A (inv_diag None: of A) from two eigsh calls with scale = sqrt(inv_diag): the smallest and the
        largest Ritz value at relative residual tol.  Ritz values approach the ends of the spectrum FROM INSIDE: lmin is never
        below the smallest eigenvalue and lmax never above the largest (in exact arithmetic), each off by at most tol * |lmax|.
        A caller that needs an enclosing interval widens it by that margin."""
        scale = None if inv_diag is None else np.sqrt(np.asarray(inv_diag, dtype=np.float64))
        lo = self.eigsh(1, "SA", tol=tol, scale=scale, vectors=False, stream=stream)[0]
        hi = self.eigsh(1, "LA", tol=tol, scale=scale, vectors=False, stream=stream)[0]
        return float(lo[0]), float(hi[0])

    def destroy(self):
        if self.h:
            self.lib.ehyb_plan_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


COARSE_ARRAYS = {"map": (0, np.int32), "row_ptr": (1, np.int32), "rows": (2, np.int32), "E": (3, np.float64), "Einv": (4, np.float64),
                 "off": (5, np.int32), "W": (6, np.float64)}
COARSE_MAX = 2048             # EHYB_COARSE_MAX
COARSE_MAX_VECS = 8           # EHYB_COARSE_MAX_VECS


def rigid_body_modes(coords, dof):
    """The near-null space of a dof-unknowns-per-node elasticity operator from the nodes' coordinates (nodes, dof), in the
    convention of ehyb_coarse_map's dof: unknown node * dof + component, the numbering before the reorder.  dof 1: the constant;
    dof 2: two translations and the rotation (-y, x); dof 3: three translations and the three rotations about the origin,
    linearised (about x: (0, -z, y), about y: (z, 0, -x), about z: (-y, x, 0)).  -> (nv, nodes * dof); permute every row with
    vector_reorder before Coarse.from_vectors."""
    coords = np.asarray(coords, dtype=np.float64)
    if dof == 1:
        coords = coords.reshape(len(coords), -1)
    assert dof in (1, 2, 3) and coords.ndim == 2 and (dof == 1 or coords.shape[1] == dof), (dof, coords.shape)
    nodes = coords.shape[0]
    out = np.zeros((dof + (0, 0, 1, 3)[dof], nodes, dof))
    for c in range(dof):
        out[c, :, c] = 1.0
    if dof == 2:
        out[2, :, 0], out[2, :, 1] = -coords[:, 1], coords[:, 0]
    if dof == 3:
        x, y, z = coords.T
        out[3, :, 1], out[3, :, 2] = -z, y
        out[4, :, 0], out[4, :, 2] = z, -x
        out[5, :, 0], out[5, :, 1] = -y, x
    return out.reshape(len(out), nodes * dof)


class Coarse:
    """ehyb_coarse: the aggregate coarse space of Plan.cg_coarse for a reordered matrix -- the matrix the plan was built from.
    map None: ehyb_coarse_map(matrix, agg_rows, dof) (agg_rows 0: chosen from the size); otherwise the caller's (n,) map, in the
    permuted numbering like everything here.  upload=False keeps it on the host (no GPU needed).  Coarse.from_vectors builds the
    space from near-null-space vectors instead of constants; every solver takes either kind."""

    def __init__(self, matrix, agg_rows=0, dof=1, map=None, upload=True):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        self.n = matrix.n
        if map is None:
            map, nc = np.empty(max(self.n, 1), dtype=np.int32), C.c_int(0)
            _check(self.lib.ehyb_coarse_map(C.byref(matrix.c), int(agg_rows), int(dof), _ptr(map, C.c_int32), C.byref(nc)), "ehyb_coarse_map")
            map, nc = map[:self.n], nc.value
        else:
            map = np.ascontiguousarray(map, dtype=np.int32)
            assert map.shape == (self.n,), (map.shape, self.n)
            nc = int(map.max()) + 1 if self.n else 0
        _check(self.lib.ehyb_coarse_create_host(C.byref(matrix.c), _ptr(map, C.c_int32), nc, C.byref(self.h)), "ehyb_coarse_create_host")
        self.nc = nc
        if upload:
            self.upload()

    @classmethod
    def raw(cls, n, map, einv, upload=True):
        """ehyb_coarse_create_raw: an object from a map and a caller's E^-1 (nc, nc) -- for tests of the kernels."""
        self = cls.__new__(cls)
        self.lib, self.h, self.n = _lib.load(), C.c_void_p(), int(n)
        map = np.ascontiguousarray(map, dtype=np.int32)
        einv = np.ascontiguousarray(einv, dtype=np.float64)
        self.nc = einv.shape[0]
        assert map.shape == (self.n,) and einv.shape == (self.nc, self.nc)
        _check(self.lib.ehyb_coarse_create_raw(self.n, _ptr(map, C.c_int32), self.nc, _ptr(einv, C.c_double), C.byref(self.h)),
               "ehyb_coarse_create_raw")
        if upload:
            self.upload()
        return self

    @classmethod
    def from_vectors(cls, matrix, B, agg_rows=0, agg=None, upload=True):
        """ehyb_coarse_create_host_vecs: the coarse space of the local bases of B (nv, n), near-null-space vectors in the permuted
        numbering (rigid_body_modes, eigenvectors of Plan.lobpcg ...), on the aggregates `agg` (n,).  agg None:
        ehyb_coarse_map(matrix, agg_rows, 1); agg_rows 0: max(128, ceil(n nv / 1536)), which keeps nagg * nv below EHYB_COARSE_MAX
        as the default of Coarse does for dof."""
        self = cls.__new__(cls)
        self.lib, self.h, self.n = _lib.load(), C.c_void_p(), matrix.n
        B = np.ascontiguousarray(np.atleast_2d(np.asarray(B, dtype=np.float64)))
        assert B.ndim == 2 and B.shape[1] == self.n, (B.shape, self.n)
        self.nv = B.shape[0]
        if agg is None:
            if agg_rows <= 0:
                agg_rows = max(128, -(-self.n * self.nv // 1536))
            agg, nagg = np.empty(max(self.n, 1), dtype=np.int32), C.c_int(0)
            _check(self.lib.ehyb_coarse_map(C.byref(matrix.c), int(agg_rows), 1, _ptr(agg, C.c_int32), C.byref(nagg)), "ehyb_coarse_map")
            agg, nagg = agg[:self.n], nagg.value
        else:
            agg = np.ascontiguousarray(agg, dtype=np.int32)
            assert agg.shape == (self.n,), (agg.shape, self.n)
            nagg = int(agg.max()) + 1 if self.n else 0
        _check(self.lib.ehyb_coarse_create_host_vecs(C.byref(matrix.c), _ptr(agg, C.c_int32), nagg, _ptr(B, C.c_double), max(self.n, 1), self.nv,
                                                     C.byref(self.h)), "ehyb_coarse_create_host_vecs")
        self.nagg = nagg
        self.nc = int(self.array("off")[-1])
        if upload:
            self.upload()
        return self

    @classmethod
    def raw_vectors(cls, n, agg, off, W, einv, upload=True):
        """ehyb_coarse_create_raw_vecs: an object from aggregates (n,), off (nagg + 1,), W (nv, n) and a caller's E^-1 (nc, nc) --
        for tests of the kernels."""
        self = cls.__new__(cls)
        self.lib, self.h, self.n = _lib.load(), C.c_void_p(), int(n)
        agg = np.ascontiguousarray(agg, dtype=np.int32)
        off = np.ascontiguousarray(off, dtype=np.int32)
        W = np.ascontiguousarray(W, dtype=np.float64)
        einv = np.ascontiguousarray(einv, dtype=np.float64)
        self.nv, self.nagg, self.nc = W.shape[0], len(off) - 1, einv.shape[0]
        assert agg.shape == (self.n,) and W.shape == (self.nv, self.n) and einv.shape == (self.nc, self.nc) and off[-1] == self.nc
        _check(self.lib.ehyb_coarse_create_raw_vecs(self.n, _ptr(agg, C.c_int32), self.nagg, _ptr(off, C.c_int32), _ptr(W, C.c_double),
                                                    max(self.n, 1), self.nv, _ptr(einv, C.c_double), C.byref(self.h)), "ehyb_coarse_create_raw_vecs")
        if upload:
            self.upload()
        return self

    def upload(self):
        _check(self.lib.ehyb_coarse_upload(self.h), "ehyb_coarse_upload")
        return self

    def array(self, name):
        """ehyb_coarse_host_array: "map" (n,), "row_ptr" (nc + 1,), "rows" (n,), "E" and "Einv" (nc, nc) -- copies.  On an object
        of from_vectors / raw_vectors "map", "row_ptr" (nagg + 1,) and "rows" describe the aggregates, and there are "off"
        (nagg + 1,) and "W" (nv, n); on any other object these two are empty."""
        which, dtype = COARSE_ARRAYS[name]
        if name in ("off", "W") and not getattr(self, "nv", 0):
            return np.zeros(0, dtype=dtype)
        p, cnt = C.c_void_p(), C.c_int64()
        _check(self.lib.ehyb_coarse_host_array(self.h, which, C.byref(p), C.byref(cnt)), "ehyb_coarse_host_array")
        if cnt.value == 0 or not p.value:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (cnt.value * np.dtype(dtype).itemsize)).from_address(p.value)
        out = np.frombuffer(buf, dtype=dtype, count=cnt.value).copy()
        return out.reshape(self.nc, self.nc) if name in ("E", "Einv") else out.reshape(self.nv, self.n) if name == "W" else out

    def apply(self, r, inv_diag=None, stream=0):
        """ehyb_coarse_apply: z = inv_diag .* r + P E^-1 P^T r for a host vector r (permuted numbering) -> z"""
        r = np.ascontiguousarray(r, dtype=np.float64)
        assert r.shape == (self.n,)
        dr, dz = DeviceBuffer(self.n).upload(r), DeviceBuffer(self.n)
        dd = None if inv_diag is None else DeviceBuffer(self.n).upload(inv_diag)
        _check(self.lib.ehyb_coarse_apply(self.h, C.c_void_p(dd.ptr) if dd else None, C.c_void_p(dr.ptr), C.c_void_p(dz.ptr), C.c_void_p(stream)),
               "ehyb_coarse_apply")
        _check(self.lib.ehyb_dev_sync(), "ehyb_dev_sync")
        return dz.download()

    def destroy(self):
        if self.h:
            self.lib.ehyb_coarse_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


FSAI_ARRAYS = {"row_ptr": (0, np.int64), "cols": (1, np.int32), "vals": (2, np.float64), "counts": (3, np.int64)}
FSAI_MAX_ROW = 64             # EHYB_FSAI_MAX_ROW


class _BorrowedPlan(Plan):
    """a plan that belongs to another object (Fsai.plans): stats and arrays, never destroyed from here"""

    def __init__(self, handle, n):
        self.lib, self.h, self.n, self.rows = _lib.load(), C.c_void_p(handle), n, (0, n)

    def destroy(self):
        self.h = C.c_void_p()


class Fsai:
    """ehyb_fsai: the factorised sparse approximate inverse of Plan.cg_fsai for a reordered symmetric matrix -- the matrix the plan
    was built from.  row_cap 0: EHYB_FSAI_MAX_ROW (64) columns per row of G at the most; cfg: the configuration of G's plan(s)
    (None: the defaults; val_f32 = 1 keeps the preconditioner in fp32); transpose "plan": a second plan built from G^T
    (reproducible bit for bit), "spmv_t": ehyb_spmv_t on the plan of G.  upload=False keeps it on the host (no GPU needed)."""

    def __init__(self, matrix, row_cap=0, cfg=None, transpose="plan", upload=True):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        self.n = matrix.n
        self.nnz_a = matrix.nnz
        self.transpose = transpose
        _check(self.lib.ehyb_fsai_create_host(C.byref(matrix.c), int(row_cap), C.byref(cfg) if cfg else None, {"plan": 0, "spmv_t": 1}[transpose],
                                              C.byref(self.h)), "ehyb_fsai_create_host")
        if upload:
            self.upload()

    def upload(self):
        _check(self.lib.ehyb_fsai_upload(self.h), "ehyb_fsai_upload")
        return self

    def array(self, name):
        """ehyb_fsai_host_array: "row_ptr" (n + 1,) int64, "cols" and "vals" (nnz(G),) -- G in CSR form as the host computed it --,
        "counts" (2,) -- copies"""
        which, dtype = FSAI_ARRAYS[name]
        p, cnt = C.c_void_p(), C.c_int64()
        _check(self.lib.ehyb_fsai_host_array(self.h, which, C.byref(p), C.byref(cnt)), "ehyb_fsai_host_array")
        if cnt.value == 0 or not p.value:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (cnt.value * np.dtype(dtype).itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=cnt.value).copy()

    @property
    def capped_rows(self):
        return int(self.array("counts")[0])

    @property
    def fallback_rows(self):
        """rows in their Jacobi form, as of the last numeric phase (the host build, or set_values on the device)"""
        return int(self.array("counts")[1])

    @property
    def plans(self):
        """ehyb_fsai_plans -> (the plan of G, the plan of G^T or None): views for stats and arrays; they belong to this object"""
        g, t = C.c_void_p(), C.c_void_p()
        _check(self.lib.ehyb_fsai_plans(self.h, C.byref(g), C.byref(t)), "ehyb_fsai_plans")
        return _BorrowedPlan(g.value, self.n), (_BorrowedPlan(t.value, self.n) if t.value else None)

    def set_values(self, values, entry_order=None, stream=0):
        """ehyb_fsai_set_values: the numeric phase again, on the device, for new values of A on the same pattern.  values /
        entry_order as Plan.set_values takes them: numpy arrays (host) or, both of them, device pointers given as (ptr, count)."""
        if isinstance(values, tuple):
            ptr, count = values
            order = None if entry_order is None else C.c_void_p(entry_order[0])
            _check(self.lib.ehyb_fsai_set_values(self.h, C.c_void_p(ptr), count, order, 1, C.c_void_p(stream)), "ehyb_fsai_set_values")
            return
        v = np.ascontiguousarray(values, dtype=np.float64)
        o = None if entry_order is None else np.ascontiguousarray(entry_order, dtype=np.int32)
        assert o is None or o.shape == v.shape
        _check(self.lib.ehyb_fsai_set_values(self.h, v.ctypes.data_as(C.c_void_p), len(v), o.ctypes.data_as(C.c_void_p) if o is not None else None,
                                             0, C.c_void_p(stream)), "ehyb_fsai_set_values")

    def apply(self, r, stream=0):
        """ehyb_fsai_apply: z = G^T (G r) for a host vector r (permuted numbering) -> z"""
        r = np.ascontiguousarray(r, dtype=np.float64)
        assert r.shape == (self.n,)
        dr, dz = DeviceBuffer(self.n).upload(r), DeviceBuffer(self.n)
        _check(self.lib.ehyb_fsai_apply(self.h, C.c_void_p(dr.ptr), C.c_void_p(dz.ptr), C.c_void_p(stream)), "ehyb_fsai_apply")
        _check(self.lib.ehyb_dev_sync(), "ehyb_dev_sync")
        return dz.download()

    def destroy(self):
        if self.h:
            self.lib.ehyb_fsai_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


BIC_ARRAYS = {"block_ptr": (0, np.int32), "perm": (1, np.int32), "row_ptr": (2, np.int64), "cols": (3, np.int32), "vals": (4, np.float64),
              "dinv": (5, np.float64), "level_f": (6, np.int32), "level_b": (7, np.int32), "shift": (8, np.float64), "counts": (9, np.int64)}
BIC_MAX_BLOCK = 20480         # EHYB_BIC_MAX_BLOCK
BIC_ORDERS = {"stored": 0, "colour": 1}


class Bic:
    """ehyb_bic: the block incomplete Cholesky preconditioner of Plan.cg_bic for a reordered symmetric matrix -- the matrix the plan
    was built from.  An IC(0) factor of every diagonal block, applied by two triangular solves in one workgroup's LDS.
    block_rows 0: whole partitions (cut where longer than EHYB_BIC_MAX_BLOCK); order "stored": the rows as they stand,
    "colour": greedy colouring inside every block (a few levels, more iterations).  upload=False keeps it on the host (no GPU
    needed)."""
    _PREFIX, _ARRAYS = "ehyb_bic", BIC_ARRAYS      # (Bilu: the same entry points under another name)

    def _call(self, what, *args):
        name = f"{self._PREFIX}_{what}"
        _check(getattr(self.lib, name)(*args), name)

    def __init__(self, matrix, block_rows=0, order="stored", upload=True):
        self.lib = _lib.load()
        self.h = C.c_void_p()
        self.n = matrix.n
        self.order = order
        self._call("create_host", C.byref(matrix.c), int(block_rows), BIC_ORDERS[order], C.byref(self.h))
        if upload:
            self.upload()

    @classmethod
    def raw(cls, block_ptr, row_ptr, cols, vals, dinv, upload=True):
        """ehyb_bic_create_raw: an object from a caller's strictly lower L in CSR form (block-local columns) and dinv, with the
        identity order -- for tests of the kernels."""
        self = cls.__new__(cls)
        self.lib, self.h, self.order = _lib.load(), C.c_void_p(), "stored"
        bp = np.ascontiguousarray(block_ptr, dtype=np.int32)
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        cl = np.ascontiguousarray(cols, dtype=np.int32)
        vl = np.ascontiguousarray(vals, dtype=np.float64)
        dv = np.ascontiguousarray(dinv, dtype=np.float64)
        self.n = len(dv)
        assert rp.shape == (self.n + 1,) and len(cl) == len(vl) == rp[-1] and len(bp) >= 2
        if len(cl) == 0:            # (an empty array has no address worth passing; one unread element)
            cl, vl = np.zeros(1, dtype=np.int32), np.zeros(1)
        _check(self.lib.ehyb_bic_create_raw(self.n, len(bp) - 1, _ptr(bp, C.c_int32), _ptr(rp, C.c_int64), _ptr(cl, C.c_int32), _ptr(vl, C.c_double),
                                            _ptr(dv, C.c_double), C.byref(self.h)), "ehyb_bic_create_raw")
        if upload:
            self.upload()
        return self

    def upload(self):
        self._call("upload", self.h)
        return self

    def array(self, name):
        """ehyb_bic_host_array: "block_ptr" (nb + 1,), "perm" (n,), "row_ptr" (n + 1,) int64, "cols" (block-local positions) and
        "vals" (nnz(L),) -- L in CSR form in position order, strictly lower part --, "dinv", "level_f", "level_b" (n,), "shift"
        (nb,), "counts" (4,) -- copies"""
        which, dtype = self._ARRAYS[name]
        p, cnt = C.c_void_p(), C.c_int64()
        self._call("host_array", self.h, which, C.byref(p), C.byref(cnt))
        if cnt.value == 0 or not p.value:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (cnt.value * np.dtype(dtype).itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype, count=cnt.value).copy()

    @property
    def max_k(self):
        """ehyb_bic_max_k: the columns one launch of the apply kernel serves"""
        return int(getattr(self.lib, f"{self._PREFIX}_max_k")(self.h))

    @property
    def blocks(self):
        return int(self.array("counts")[0])

    @property
    def shifted_blocks(self):
        return int(self.array("counts")[1])

    @property
    def fallback_blocks(self):
        return int(self.array("counts")[2])

    @property
    def levels(self):
        """the most levels of any block, forward or backward"""
        return int(self.array("counts")[3])

    @property
    def stream_info(self):
        """ehyb_bic_stream_info -> (bytes of the two device streams, their entries without padding, the workgroup size)"""
        b, e, t = C.c_int64(), C.c_int64(), C.c_int()
        self._call("stream_info", self.h, C.byref(b), C.byref(e), C.byref(t))
        return b.value, e.value, t.value

    def apply(self, R, ld=None, active=None, Z0=None, stream=0):
        """ehyb_bic_apply: Z = P^T (L L^T)^-1 P R for host vectors (permuted numbering): R (n,) -> z (n,), or R (k, n) -> Z (k, n),
        staged on the device with leading dimension ld (default n).  Z starts as Z0 (k, n) (default NaN); active (k,) flags:
        ehyb_bic_apply_step, which leaves the columns whose flag is 0 as they were."""
        R = np.ascontiguousarray(R, dtype=np.float64)
        one = R.ndim == 1
        R2 = R.reshape(1, -1) if one else R
        k, n = R2.shape
        assert n == self.n, (n, self.n)
        ld = n if ld is None else int(ld)
        assert ld >= n
        staged, start = np.zeros((k, ld)), np.full((k, ld), np.nan)
        staged[:, :n] = R2
        if Z0 is not None:
            start[:, :n] = np.asarray(Z0, dtype=np.float64).reshape(k, n)
        dr, dz = DeviceBuffer(k * ld).upload(staged.ravel()), DeviceBuffer(k * ld).upload(start.ravel())
        if active is None:
            self._call("apply", self.h, C.c_void_p(dr.ptr), ld, C.c_void_p(dz.ptr), ld, k, C.c_void_p(stream))
        else:
            flags = np.zeros(k + (k & 1), dtype=np.int32)       # (a DeviceBuffer holds doubles: two int32 each)
            flags[:k] = np.asarray(active, dtype=np.int32)
            da = DeviceBuffer(len(flags) // 2).upload(flags.view(np.float64))
            self._call("apply_step", self.h, C.c_void_p(dr.ptr), ld, C.c_void_p(dz.ptr), ld, k, C.c_void_p(da.ptr), C.c_void_p(stream))
        _check(self.lib.ehyb_dev_sync(), "ehyb_dev_sync")
        Z = dz.download().reshape(k, ld)
        self.last_pad = Z[:, n:]          # what lies between the columns: untouched (NaN) if the kernel keeps to its rows
        return Z[0, :n].copy() if one else Z[:, :n].copy()

    def destroy(self):
        if self.h:
            getattr(self.lib, f"{self._PREFIX}_destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


BILU_ARRAYS = {"block_ptr": (0, np.int32), "perm": (1, np.int32), "l_row_ptr": (2, np.int64), "l_cols": (3, np.int32), "l_vals": (4, np.float64),
               "u_row_ptr": (5, np.int64), "u_cols": (6, np.int32), "u_vals": (7, np.float64), "u_dinv": (8, np.float64), "level_f": (9, np.int32),
               "level_b": (10, np.int32), "shift": (11, np.float64), "counts": (12, np.int64)}


class Bilu(Bic):
    """ehyb_bilu: the block ILU(0) preconditioner of Plan.gmres_bilu and Plan.bicgstab_bilu for a reordered (unsymmetric) matrix --
    the matrix the plan was built from.  L U ~ A_b on the pattern of every diagonal block (the blocks and orders of Bic), applied
    by Bic's kernel: a unit-lower forward solve and an upper backward solve in one workgroup's LDS.  upload=False keeps it on the
    host (no GPU needed).  array(name): "block_ptr", "perm", "l_row_ptr", "l_cols", "l_vals" (the strictly lower part of L),
    "u_row_ptr", "u_cols", "u_vals" (the strictly upper part of U), "u_dinv" (1 / u_ii), "level_f", "level_b", "shift", "counts".
    blocks, shifted_blocks, fallback_blocks, levels, max_k, stream_info, apply (Z = P^T (L U)^-1 P R) and destroy as Bic's."""
    _PREFIX, _ARRAYS = "ehyb_bilu", BILU_ARRAYS

    @classmethod
    def raw(cls, block_ptr, l_row_ptr, l_cols, l_vals, u_row_ptr, u_cols, u_vals, u_dinv, upload=True):
        """ehyb_bilu_create_raw: an object from a caller's strictly lower L and strictly upper U in CSR form (block-local columns)
        and 1 / u_ii, with the identity order -- for tests of the kernels."""
        self = cls.__new__(cls)
        self.lib, self.h, self.order = _lib.load(), C.c_void_p(), "stored"
        bp = np.ascontiguousarray(block_ptr, dtype=np.int32)
        dv = np.ascontiguousarray(u_dinv, dtype=np.float64)
        self.n = len(dv)
        tri = []
        for rp, cl, vl in ((l_row_ptr, l_cols, l_vals), (u_row_ptr, u_cols, u_vals)):
            rp = np.ascontiguousarray(rp, dtype=np.int64)
            cl = np.ascontiguousarray(cl, dtype=np.int32)
            vl = np.ascontiguousarray(vl, dtype=np.float64)
            assert rp.shape == (self.n + 1,) and len(cl) == len(vl) == rp[-1] and len(bp) >= 2
            if len(cl) == 0:            # (an empty array has no address worth passing; one unread element)
                cl, vl = np.zeros(1, dtype=np.int32), np.zeros(1)
            tri += [rp, cl, vl]
        self._call("create_raw", self.n, len(bp) - 1, _ptr(bp, C.c_int32), _ptr(tri[0], C.c_int64), _ptr(tri[1], C.c_int32), _ptr(tri[2], C.c_double),
                   _ptr(tri[3], C.c_int64), _ptr(tri[4], C.c_int32), _ptr(tri[5], C.c_double), _ptr(dv, C.c_double), C.byref(self.h))
        if upload:
            self.upload()
        return self


def fsai_factor_step(indptr, indices, data, g_ptr, g_cols, stream=0):
    """ehyb_fsai_factor_step: one launch of the factor kernel on A in CSR form and a pattern (host arrays) -> (g, fallback rows)"""
    ap = np.ascontiguousarray(indptr, dtype=np.int32)
    ac = np.ascontiguousarray(indices, dtype=np.int32)
    av = np.ascontiguousarray(data, dtype=np.float64)
    gp = np.ascontiguousarray(g_ptr, dtype=np.int64)
    gc = np.ascontiguousarray(g_cols, dtype=np.int32)
    n = len(ap) - 1
    assert gp.shape == (n + 1,) and len(ac) == len(av) == ap[-1] and len(gc) == gp[-1]
    g, fb = np.empty(max(len(gc), 1)), C.c_int(0)
    _check(_lib.load().ehyb_fsai_factor_step(n, _ptr(ap, C.c_int32), _ptr(ac, C.c_int32), _ptr(av, C.c_double), _ptr(gp, C.c_int64),
                                             _ptr(gc, C.c_int32), _ptr(g, C.c_double), C.byref(fb), C.c_void_p(stream)), "ehyb_fsai_factor_step")
    return g[:len(gc)], fb.value


def minres_inv_diag(diag):
    """The positive diagonal preconditioner of Plan.minres from the matrix's diagonal: 1 / |a_ii|, and 1 where a_ii = 0."""
    d = np.abs(np.asarray(diag, dtype=np.float64))
    return np.where(d > 0, 1.0 / np.where(d > 0, d, 1.0), 1.0)


def pad_square(indptr, indices, data, shape):
    """The m x n CSR matrix padded with empty rows or columns to max(m, n) square -> (indptr, indices, data) for Matrix.from_csr:
    what Plan.lsqr takes for a rectangular matrix, with b padded by zeros; the padded entries of x come back as 0.0."""
    m, n = int(shape[0]), int(shape[1])
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int32)
    assert indptr.shape == (m + 1,) and (indices.size == 0 or (0 <= indices.min() and indices.max() < n))
    if m < n:
        indptr = np.concatenate([indptr, np.full(n - m, indptr[-1], dtype=np.int64)])
    return indptr, indices, np.asarray(data, dtype=np.float64)


def small_svd(M):
    """ehyb_small_svd: M = X diag(sigma) Y^T for a dense (rows, cols) matrix with 1 <= cols <= rows <= 65 by one-sided Jacobi on
    the host -> (X (rows, cols) with orthonormal columns, sigma (cols,) falling, Y (cols, cols) orthogonal).  The same input gives
    the same bits.  Raises EhybError (code 1) for a size out of range or a non-finite entry."""
    M = np.asfortranarray(M, dtype=np.float64)
    assert M.ndim == 2
    rows, cols = M.shape
    sigma, X, Y = np.zeros(max(cols, 1)), np.zeros((rows, max(cols, 1)), order="F"), np.zeros((max(cols, 1), max(cols, 1)), order="F")
    _check(_lib.load().ehyb_small_svd(rows, cols, _ptr(M, C.c_double), max(rows, 1), _ptr(sigma, C.c_double), _ptr(X, C.c_double),
                                      _ptr(Y, C.c_double)), "ehyb_small_svd")
    return np.ascontiguousarray(X), sigma, np.ascontiguousarray(Y)


def lobpcg_rr(G, H, nb):
    """ehyb_lobpcg_rr: the Rayleigh-Ritz step of Plan.lobpcg on the host for the pencil (H, G), both (mc, mc) symmetric (only the
    upper triangles are read), mc <= 24 -> (theta (nb,) rising, Y (mc, nb) with Y^T G Y = I, rank).  Raises EhybError (code 1)
    for a non-finite entry, a negative G[i, i] or a rank below nb."""
    G = np.asfortranarray(G, dtype=np.float64)
    H = np.asfortranarray(H, dtype=np.float64)
    mc = G.shape[0]
    assert G.shape == (mc, mc) and H.shape == (mc, mc)
    theta, Y, rank = np.zeros(max(int(nb), 1)), np.zeros((mc, max(int(nb), 1)), order="F"), C.c_int(0)
    _check(_lib.load().ehyb_lobpcg_rr(mc, _ptr(G, C.c_double), _ptr(H, C.c_double), int(nb), _ptr(theta, C.c_double), _ptr(Y, C.c_double),
                                      C.byref(rank)), "ehyb_lobpcg_rr")
    return theta, np.ascontiguousarray(Y), rank.value


def cheb_coeffs(lmin, lmax, degree):
    """ehyb_cheb_coeffs -> (c0, a (degree,), b (degree,)): the coefficients of the Chebyshev preconditioner's recurrence."""
    c0 = C.c_double(0)
    a, b = np.zeros(max(int(degree), 0)), np.zeros(max(int(degree), 0))
    _check(_lib.load().ehyb_cheb_coeffs(lmin, lmax, int(degree), C.byref(c0), _ptr(a, C.c_double), _ptr(b, C.c_double)), "ehyb_cheb_coeffs")
    return c0.value, a, b


def spmv_gpu_ehyb(matrix, vector_in, max_iter, cfg=None, timing=False):
    """spmvGPuEHYB (spmv.cu:61-133): y = A_perm * x on the GPU, 10 warm-ups + max_iter runs.
    cfg None = what the drop-in symbol does by itself (storage chosen from the matrix).
    timing=True also returns the milliseconds of the max_iter timed multiplies."""
    lib = _lib.load()
    x = np.ascontiguousarray(vector_in, dtype=np.float64)
    y = np.zeros(matrix.n, dtype=np.float64)
    it = C.c_int(0)
    ms = C.c_double(0)
    _check(lib.spmvGPuEHYB_cfg(C.byref(matrix.c), _ptr(x, C.c_double), _ptr(y, C.c_double), max_iter, C.byref(it),
                               C.byref(cfg) if cfg is not None else None, C.byref(ms)), "spmvGPuEHYB")
    return (y, it.value, ms.value) if timing else (y, it.value)


def tune_decide(cost, xcc, dur, map_now):
    """ehyb_debug_tune_decide: the decision of ehyb_plan_tune on these numbers -> the new map, or None (no stable placement)"""
    cost, dur = np.ascontiguousarray(cost, dtype=np.float64), np.ascontiguousarray(dur, dtype=np.float64)
    xcc, map_now = np.ascontiguousarray(xcc, dtype=np.intc), np.ascontiguousarray(map_now, dtype=np.int32)
    n = len(cost)
    assert len(xcc) == len(dur) == len(map_now) == n
    out, stable = np.full(n, -1, dtype=np.int32), C.c_int(-1)
    _check(_lib.load().ehyb_debug_tune_decide(n, _ptr(cost, C.c_double), _ptr(xcc, C.c_int), _ptr(dur, C.c_double), _ptr(map_now, C.c_int32),
                                              _ptr(out, C.c_int32), C.byref(stable)), "ehyb_debug_tune_decide")
    return out if stable.value else None


def host_threads():
    """ehyb_host_threads: OpenMP threads of the host builder = the CPUs the process owns (affinity, cgroup quota)."""
    return int(_lib.load().ehyb_host_threads())


def device_count():
    c = C.c_int(0)
    _lib.load().ehyb_device_count(C.byref(c))
    return c.value


class SpmvGraph:
    """A captured run of multiplies of one plan (include/ehyb.h: ehyb_spmv_graph_create / ehyb_graph_launch)."""

    def __init__(self, plan, x_dev, y_dev, multiplies=1):
        self.lib = plan.lib
        self.h = C.c_void_p()
        _check(self.lib.ehyb_spmv_graph_create(plan.h, C.c_void_p(x_dev), C.c_void_p(y_dev), int(multiplies), C.byref(self.h)), "ehyb_spmv_graph_create")

    def launch(self, stream=0):
        _check(self.lib.ehyb_graph_launch(self.h, C.c_void_p(stream)), "ehyb_graph_launch")

    def destroy(self):
        if self.h:
            self.lib.ehyb_graph_destroy(self.h)
            self.h = None


class Stream:
    """ehyb_stream_create: a non-blocking HIP stream for callers without a HIP binding (tests)."""

    def __init__(self):
        self.lib = _lib.load()
        self.p = C.c_void_p()
        _check(self.lib.ehyb_stream_create(C.byref(self.p)), "ehyb_stream_create")

    @property
    def ptr(self):
        return self.p.value

    def sync(self):
        _check(self.lib.ehyb_stream_sync(self.p), "ehyb_stream_sync")

    def destroy(self):
        if self.p:
            self.lib.ehyb_stream_destroy(self.p)
            self.p = None


class DeviceBuffer:
    """hipMalloc'ed array of doubles (tests / CLI plumbing; bench.py uses torch tensors)."""

    def __init__(self, n):
        self.lib = _lib.load()
        self.n = n
        self.p = C.c_void_p()
        _check(self.lib.ehyb_dev_alloc(n * 8, C.byref(self.p)), "ehyb_dev_alloc")

    @property
    def ptr(self):
        return self.p.value

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        _check(self.lib.ehyb_h2d(self.p, a.ctypes.data_as(C.c_void_p), a.nbytes), "ehyb_h2d")
        return self

    def download(self):
        out = np.empty(self.n, dtype=np.float64)
        _check(self.lib.ehyb_d2h(out.ctypes.data_as(C.c_void_p), self.p, out.nbytes), "ehyb_d2h")
        return out

    def free(self):
        if self.p:
            self.lib.ehyb_dev_free(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
