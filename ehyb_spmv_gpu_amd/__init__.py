"""MI355X-native Explicit-Caching HYB fp64 SpMV: Python host mirror over libehyb.so.

The compute path is the HIP library built from csrc/ (see include/ehyb.h for the C-ABI);
importing this package does not load it, `ehyb_spmv_gpu_amd.host` does on first use and
raises if it has not been built.
"""
from . import host  # noqa: F401
from .host import (  # noqa: F401
    ARRAYS,
    Bic,
    Bilu,
    EHYB_PART_AUTO,
    EHYB_PART_CONTIGUOUS,
    EHYB_PART_DEGREE,
    EHYB_PART_MTMETIS,
    EHYB_PART_MULTILEVEL,
    EHYB_WINDOW_HALO,
    EHYB_WINDOW_REFERENCE,
    KERNEL_TABLE_T,
    KERNEL_TABLES,
    Coarse,
    DeviceBuffer,
    EhybError,
    Fsai,
    Matrix,
    Plan,
    SpmvGraph,
    Stream,
    cheb_coeffs,
    device_count,
    entry_order,
    fsai_factor_step,
    host_threads,
    kernel_table,
    kernel_table_t,
    lobpcg_rr,
    make_config,
    minres_inv_diag,
    pad_square,
    partition_graph,
    rigid_body_modes,
    sizing,
    small_svd,
    spmv_gpu_ehyb,
    tune_decide,
    vector_recover,
    vector_reorder,
    x_glibc,
)

__all__ = [n for n in dir() if not n.startswith("_")]
