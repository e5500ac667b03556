// y = A^T x on the plan A already has (ehyb_spmv_t): the transposed window kernel and the transposed CSR-segment residual
// (bodies: ell_t_device.h), their table, their launch path and the rule for which plans they serve.
//
//   ehyb_ell_t_kernel<THREADS, INLINE_ER>   one workgroup per work item of the forward launch.  Per segment: cnt + hn fp64
//                    accumulators in LDS (the forward kernel's x window) are zeroed; every wave takes slabs from the LDS
//                    counter, a lane loads x[its row] once and adds value * x[row] to the window column of each of its entries
//                    (ds_add_f64, the lanes of a group of equal column lists summed across lanes first; an inline residual:
//                    straight to y[global column], global_atomic_add_f64); the window is then
//                    flushed, own columns to y[base + i], halo columns to y[halo_cols[..]], with global_atomic_add_f64.
//   ehyb_er_t_kernel<256>   CSR residual and the direct shape: every lane adds value * x[row] to y[column].
// y is zeroed in-stream by a memset node first; every contribution is an atomic add, so the result is reproducible up to the order
// of summation only (bit-exact where every partial sum is exact).  No x window: the LDS budget is the forward launch's.
#include <hip/hip_runtime.h>

#include <vector>

#include "ehyb_internal.h"
#include "hip_try.h"
#include "ell_t_device.h"

using namespace ehyb;

// Up to 128 VGPRs (four waves per SIMD: one 1024-thread workgroup per CU, as the forward kernel at its default 160 KiB window):
// with the group sums the body takes 95-97, and at the forward plain kernel's 64 it spilled 132 bytes per lane.
template <int THREADS, bool INLINE_ER>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void ehyb_ell_t_kernel(const EllArgs A)
{
    ell_items_t<THREADS, INLINE_ER>(A);
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void ehyb_er_t_kernel(const int4* __restrict__ blocks, const int64_t* __restrict__ seg_ptr,
                                                            const int* __restrict__ seg_row, const int* __restrict__ col,
                                                            const double* __restrict__ val, const double* __restrict__ x, double* __restrict__ y)
{
    er_blocks_t<THREADS>(blocks, seg_ptr, seg_row, col, val, x, y);
}

// Every instantiation: rows {kind, threads, inl} of ehyb_debug_kernel_table_t, in this order
struct TKernel {
    int kind, threads;  // EHYB_KERNEL_T_WINDOW / EHYB_KERNEL_T_RESIDUAL
    bool inl;
    const void* fn;
};

static const std::vector<TKernel>& t_kernels()
{
    static const std::vector<TKernel> all = {
        {EHYB_KERNEL_T_WINDOW, 1024, false, (const void*)ehyb_ell_t_kernel<1024, false>}, {EHYB_KERNEL_T_WINDOW, 1024, true, (const void*)ehyb_ell_t_kernel<1024, true>},
        {EHYB_KERNEL_T_WINDOW, 512, false, (const void*)ehyb_ell_t_kernel<512, false>},   {EHYB_KERNEL_T_WINDOW, 512, true, (const void*)ehyb_ell_t_kernel<512, true>},
        {EHYB_KERNEL_T_WINDOW, 256, false, (const void*)ehyb_ell_t_kernel<256, false>},   {EHYB_KERNEL_T_WINDOW, 256, true, (const void*)ehyb_ell_t_kernel<256, true>},
        {EHYB_KERNEL_T_RESIDUAL, 256, false, (const void*)ehyb_er_t_kernel<256>},
    };
    return all;
}
static_assert(kKernelTableTCap >= 7, "the transposed launch log of a plan has no room for the table");

static int t_kernel_row(int kind, int threads, bool inl)
{
    const std::vector<TKernel>& table = t_kernels();
    for (size_t row = 0; row < table.size(); ++row)
        if (table[row].kind == kind && table[row].threads == threads && table[row].inl == inl) return (int)row;
    return -1;
}

// The forms the transposed kernels do not serve, in the order they are reported; null = served.  Host arithmetic only.
static const char* t_refusal(const ehyb_plan* P)
{
    const HostLayout& H = P->host;
    if (H.sym) return "symmetric pair storage (for a symmetric matrix A^T = A: call ehyb_spmv; the form's LDS has no room for halo accumulators)";
    if (H.er_panel || H.deferred.pending || H.pb_assign) return "a residual in panel form";
    if (P->cfg.val_f32 == 1) return "cfg.val_f32 = 1 (fp32 value streams)";
    if (H.row_begin != 0 || H.row_end != H.n_cols) return "a plan not over all rows (a row range)";
    if (H.col_seg_first.size() > 2) return "a plan with column segments";
    return nullptr;
}

int ehyb::spmv_t_opt_in_lds()
{
    for (const TKernel& e : t_kernels())
        if (e.kind == EHYB_KERNEL_T_WINDOW) HIP_TRY(hipFuncSetAttribute(e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, EHYB_LDS_MAX_DOUBLES * 8));
    return EHYB_OK;
}

static int launch_window_t(ehyb_plan* P, const double* x, double* y, hipStream_t st)
{
    const HostLayout& H = P->host;
    const int n_items = (int)(H.items.size() / kItemWords);
    if (n_items == 0 || H.direct) return EHYB_OK;  // direct shape: the residual kernel is the whole multiply
    const int row = t_kernel_row(EHYB_KERNEL_T_WINDOW, P->cfg.threads, H.inline_er);
    if (row < 0) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_t: ELL workgroup size %d not built (256/512/1024)", P->cfg.threads);
    EllArgs A = window_launch_args(P, x, y);
    void* args[] = {&A};
    P->mark_launched_t((size_t)row);
    (void)hipLaunchKernel(t_kernels()[(size_t)row].fn, dim3(n_items), dim3(P->cfg.threads), args, ell_lds_bytes(H, 1), st);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

static int launch_er_t(ehyb_plan* P, const double* x, double* y, hipStream_t st)
{
    const HostLayout& H = P->host;
    if (H.er_bins[3] == 0 || H.inline_er) return EHYB_OK;  // (an inline residual rode along in the window launch)
    if (P->cfg.er_threads != 256) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_t: residual workgroup size %d not built (256)", P->cfg.er_threads);
    const int row = t_kernel_row(EHYB_KERNEL_T_RESIDUAL, 256, false);
    const int n_blocks = (int)(H.er_blocks.size() / 4);
    const int4* blocks = (const int4*)P->d_er_blocks;
    void* args[] = {&blocks, &P->d_er_seg_ptr, &P->d_er_seg_row, &P->d_er_col, &P->d_er_val, &x, &y};
    P->mark_launched_t((size_t)row);
    (void)hipLaunchKernel(t_kernels()[(size_t)row].fn, dim3(n_blocks), dim3(256), args, 0, st);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" {

int ehyb_spmv_t_supported(const ehyb_plan* P)
{
    clear_error();
    if (!P) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_t_supported: null plan");
    if (const char* why = t_refusal(P)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_t: not built for %s", why);
    return EHYB_OK;
}

int ehyb_spmv_t(ehyb_plan* P, const double* x, double* y, void* stream)
{
    if (!P || !x || !y) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_t: null argument");
    if (x == y) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_t: x and y are the same vector (y is zeroed before x is read)");
    if (const char* why = t_refusal(P)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_t: not built for %s", why);
    if (!P->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_spmv_t: plan not uploaded (no CPU fallback exists)");
    const hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(y, 0, (size_t)P->host.n_cols * sizeof(double), st));  // a memset node in a captured graph
    const int rc = launch_window_t(P, x, y, st);
    return rc != EHYB_OK ? rc : launch_er_t(P, x, y, st);
}

int ehyb_debug_kernel_table_t(int32_t* rows, int cap, int* n_rows)
{
    clear_error();
    if (!n_rows || cap < 0 || (cap > 0 && !rows)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_kernel_table_t: bad arguments");
    const std::vector<TKernel>& table = t_kernels();
    *n_rows = (int)table.size();
    for (int i = 0; i < std::min(cap, *n_rows); ++i) {
        rows[EHYB_KERNEL_ROW_T * i + 0] = table[(size_t)i].kind;
        rows[EHYB_KERNEL_ROW_T * i + 1] = table[(size_t)i].threads;
        rows[EHYB_KERNEL_ROW_T * i + 2] = table[(size_t)i].inl;
    }
    return EHYB_OK;
}

int ehyb_debug_launched_t(const ehyb_plan* P, uint8_t* out, int cap)
{
    clear_error();
    const int n = (int)t_kernels().size();
    if (!P || !out || cap < n) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_launched_t: bad arguments (the table has %d rows, room for %d)", n, cap);
    for (int i = 0; i < n; ++i) out[i] = __atomic_load_n(&P->launched_t[i], __ATOMIC_RELAXED);
    return EHYB_OK;
}

}  // extern "C"
