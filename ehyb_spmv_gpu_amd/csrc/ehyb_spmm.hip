// Y = A X for k columns per pass over the matrix (ehyb_spmm, include/ehyb.h): the window kernel and the CSR-segment residual
// of ehyb_hip.hip widened to K = 2, 3, 4 columns.  The value stream, the column words, the lane maps and the slab records are
// read ONCE for all K columns; what grows with K is the x image in LDS and the x / y traffic.  A multiply moves about
// matrix + K (x + y) bytes instead of K (matrix + x + y).
//
//   ehyb_ell_k_kernel  the window kernel with the window staged INTERLEAVED: win[c*K + j] = X[col(c) + j*ldx] for own rows and
//                      halo alike, so that a lane fetches the K values of one column with one (K = 2) or two (K = 3, 4) LDS reads.
//                      Every value pair and every shared column word feeds 2 K FMAs.  Plain storage keeps acc0/acc1 per column
//                      in exactly the one-vector order (inline residual, then even and odd pair halves, then acc0 + acc1): column
//                      j of a plain-storage multiply is bit for bit ehyb_spmv of X[:, j].  Symmetric pairs: the own-row x_i, the
//                      DPP group sum and the ds_add_f64 into yacc[row*K + j] are per column; the accumulators sit behind the
//                      K-wide image.  The LDS slab counter sits behind K window capacities (the plan's k_max sees to it that
//                      this fits the 160 KiB).  Only the LDS-counter (DYN) form is built.
//   ehyb_er_k_kernel   CSR residual segments: (column, value) loaded once, x gathered K times; rows split into several
//                      segments get one fp64 atomic per column; ASSIGN serves the direct shape.
// The walk (alternation, items from the far end, the non-temporal share) is the one-vector launch's: ell_walk.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ehyb_internal.h"
#include "ell_device.h"

using namespace ehyb;

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            ::ehyb::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return _e == hipErrorNoDevice ? EHYB_ERR_NO_DEVICE : EHYB_ERR_HIP;                \
        }                                                                                     \
    } while (0)

static constexpr int kSpmmMaxK = 4;

// ------------------------------------------------------------------ the interleaved LDS image
// The K values of window column `idx`: one ds_read_b128 for K = 2, two for K = 4 (16-byte aligned: 16 K bytes per column).
template <int K>
__device__ __forceinline__ void win_load(const double* __restrict__ win, uint32_t idx, double (&w)[K])
{
    if constexpr (K == 2) {
        const double2 a = reinterpret_cast<const double2*>(win)[idx];
        w[0] = a.x, w[1] = a.y;
    } else if constexpr (K == 4) {
        const double2 a = reinterpret_cast<const double2*>(win)[2 * idx], b = reinterpret_cast<const double2*>(win)[2 * idx + 1];
        w[0] = a.x, w[1] = a.y, w[2] = b.x, w[3] = b.y;
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) w[j] = win[idx * K + j];
    }
}

template <int K>
__device__ __forceinline__ void win_store(double* __restrict__ win, int idx, const double (&w)[K])
{
    if constexpr (K == 2) {
        reinterpret_cast<double2*>(win)[idx] = make_double2(w[0], w[1]);
    } else if constexpr (K == 4) {
        reinterpret_cast<double2*>(win)[2 * idx] = make_double2(w[0], w[1]);
        reinterpret_cast<double2*>(win)[2 * idx + 1] = make_double2(w[2], w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) win[idx * K + j] = w[j];
    }
}

// ------------------------------------------------------------------ window kernel, K columns
// One entry of a slab for K columns (ell_entry of ehyb_hip.hip, per column): SYM with the lane-group sum of the mirror products.
template <int K, bool SYM>
__device__ __forceinline__ void ell_entry_k(double v, uint32_t col16, const double* __restrict__ win, double* yacc, const double (&xi)[K],
                                            int code, double (&acc)[K])
{
    double w[K];
    if (SYM) {
        const uint32_t idx = col16 & 0x7fffu;
        win_load<K>(win, idx, w);
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] = fma(v, w[j], acc[j]);
        const bool mirror = (col16 & 0x8000u) != 0;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double mine = mirror ? v * xi[j] : 0.0;
            const double n1 = next_lane(mine), n2 = next_lane(n1);
            const double sum = mine + ((code == 1 || code == 2) ? n1 : 0.0) + (code == 2 ? n2 : 0.0);
            if (mirror && code != 3) unsafeAtomicAdd(&yacc[idx * K + j], sum);  // ds_add_f64
        }
    } else {
        win_load<K>(win, col16, w);
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] = fma(v, w[j], acc[j]);
    }
}

template <int K, bool INLINE_ER, bool SYM, bool NT>
__device__ __forceinline__ void ell_slab_k(const EllArgs& A, long long ldx, long long ldy, const double* __restrict__ win, double* yacc, int s,
                                           int base, int pe, int lane)
{
    const uint4 sm = A.slab_meta[s];
    const int np = (int)(sm.w >> 16);
    const int G = (int)(sm.w & 0x3fu) + 1;
    const double2* __restrict__ v = A.ell_val + (size_t)sm.x * 64 + lane;
    const uint32_t lgb = A.lane_group[(size_t)s * 64 + lane];
    const int code = SYM ? (int)(lgb >> 6) : 0;
    const uint32_t* __restrict__ c = A.ell_col + sm.y + (SYM ? (lgb & 0x3fu) : lgb);
    double acc0[K], acc1[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc0[j] = 0.0, acc1[j] = 0.0;
    if (INLINE_ER) {
        // the inline residual first, as in the one-vector kernel: x of its global columns gathered K times
        const int ner = (int)(sm.w >> 8) & 0xff;
        const double2* __restrict__ ve = v + (size_t)np * 64;
        const uint32_t* __restrict__ ce = A.ell_col + sm.y + (size_t)np * G + lane;
        for (int q = 0; q < ner; ++q) {
            const double2 vv = ve[q * 64];
            const uint32_t ca = ce[q * 128], cb = ce[q * 128 + 64];
            double xa[K], xb[K];
#pragma unroll
            for (int j = 0; j < K; ++j) xa[j] = A.x[ca + j * ldx], xb[j] = A.x[cb + j * ldx];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                acc0[j] = fma(vv.x, xa[j], acc0[j]);
                acc1[j] = fma(vv.y, xb[j], acc1[j]);
            }
        }
    }
    const int row = (int)sm.z + lane;
    const int lrow = SYM ? (int)A.slab_lrow[(size_t)s * 64 + lane] : row - base;
    const bool has_row = SYM ? lrow != 0xFFFF : row < pe;
    double xi[K];
    if (SYM && has_row)
        win_load<K>(win, (uint32_t)lrow, xi);
    else
#pragma unroll
        for (int j = 0; j < K; ++j) xi[j] = 0.0;
    const uint32_t radd = (!SYM && (sm.w & 0x80u)) ? (uint32_t)lrow : 0u;
    const uint32_t cmask = (SYM || has_row) ? 0xffffu : 0u;
#define ELL_COL_LO(c) (SYM ? ((c) & 0xffffu) : ((((c) & 0xffffu) + radd) & cmask))
#define ELL_COL_HI(c) (SYM ? ((c) >> 16) : ((((c) >> 16) + radd) & cmask))
    // four value pairs per step (as the one-vector kernel); symmetric pairs at K = 4 take two, which keeps them within 128 VGPRs
    constexpr int STEP = (SYM && K >= 4) ? 2 : 4;
    int k = 0;
    for (; k + STEP <= np; k += STEP) {
        double2 vv[STEP];
        uint32_t cc[STEP];
#pragma unroll
        for (int q = 0; q < STEP; ++q) vv[q] = ell_load_pair<NT>(v + (k + q) * 64);
#pragma unroll
        for (int q = 0; q < STEP; ++q) cc[q] = c[(k + q) * G];
#pragma unroll
        for (int q = 0; q < STEP; ++q) {
            ell_entry_k<K, SYM>(vv[q].x, ELL_COL_LO(cc[q]), win, yacc, xi, code, acc0);
            ell_entry_k<K, SYM>(vv[q].y, ELL_COL_HI(cc[q]), win, yacc, xi, code, acc1);
        }
    }
    for (; k < np; ++k) {
        const double2 v0 = ell_load_pair<NT>(v + k * 64);
        const uint32_t c0 = c[k * G];
        ell_entry_k<K, SYM>(v0.x, ELL_COL_LO(c0), win, yacc, xi, code, acc0);
        ell_entry_k<K, SYM>(v0.y, ELL_COL_HI(c0), win, yacc, xi, code, acc1);
    }
#undef ELL_COL_LO
#undef ELL_COL_HI
    if (has_row) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (SYM)
                unsafeAtomicAdd(&yacc[lrow * K + j], acc0[j] + acc1[j]);
            else
                A.y[row + j * ldy] = acc0[j] + acc1[j];
        }
    }
}

// Stage the K-wide window of segment g and multiply its slabs (ell_segment of ehyb_hip.hip).
template <int THREADS, int K, bool INLINE_ER, bool SYM>
__device__ __forceinline__ void ell_segment_k(const EllArgs& A, long long ldx, long long ldy, double* __restrict__ win, int* __restrict__ next_slab,
                                              int g, int lane, int wave)
{
    constexpr int WAVES = THREADS / 64;
    const int4 a = A.segs[2 * g], b = A.segs[2 * g + 1];
    const int sb = a.y, se = a.z, hn = a.w;
    const int ps = b.x, pe = b.y, wl = b.z, hb = b.w;
    if (!SYM && wl == 0 && hn == 0) {
        // a partition without a window: y = 0 for every column, the residual launch adds to it
        if (!A.windowless_zero) return;
        const int r0 = max(ps, (int)A.slab_meta[sb].z), r1 = min(pe, r0 + (se - sb) * 64);
        for (int i = r0 + (int)threadIdx.x; i < r1; i += THREADS)
#pragma unroll
            for (int j = 0; j < K; ++j) A.y[i + j * ldy] = 0.0;
        return;
    }
    __syncthreads();  // every wave is done with the previous window and counter
    const int base = ps & ~1, cnt = wl + (ps & 1);
    double* yacc = win + K * (cnt + hn);
    for (int i = threadIdx.x; i < cnt; i += THREADS) {
        double w[K];
#pragma unroll
        for (int j = 0; j < K; ++j) w[j] = A.x[base + i + j * ldx];
        win_store<K>(win, i, w);
    }
    for (int i = threadIdx.x; i < hn; i += THREADS) {
        const int col = A.halo_cols[hb + i];
        double w[K];
#pragma unroll
        for (int j = 0; j < K; ++j) w[j] = A.x[col + j * ldx];
        win_store<K>(win, cnt + i, w);
    }
    if (SYM)
        for (int i = threadIdx.x; i < K * cnt; i += THREADS) yacc[i] = 0.0;
    if (threadIdx.x == 0) *next_slab = sb + WAVES;  // slabs sb..sb+WAVES-1 are pre-assigned
    __syncthreads();
    int s = sb + wave;
    const int nt_end = sb + (int)(((long long)(se - sb) * A.nt_slabs + 1023) >> 10);
    while (s < se) {
        if (s < nt_end)
            ell_slab_k<K, INLINE_ER, SYM, true>(A, ldx, ldy, win, yacc, A.reverse ? se - 1 - (s - sb) : s, base, pe, lane);
        else
            ell_slab_k<K, INLINE_ER, SYM, false>(A, ldx, ldy, win, yacc, A.reverse ? se - 1 - (s - sb) : s, base, pe, lane);
        int nx = 0;
        if (lane == 0) nx = atomicAdd(next_slab, 1);
        s = __builtin_amdgcn_readfirstlane(nx);
    }
    if (SYM) {
        __syncthreads();  // all sums and scatters of the partition are in
        for (int i = threadIdx.x + (ps & 1); i < cnt; i += THREADS)
#pragma unroll
            for (int j = 0; j < K; ++j) A.y[base + i + j * ldy] = yacc[i * K + j];
    }
}

// A K-wide window fills the CU: one workgroup per CU for every K and storage, up to 128 VGPRs.
template <int THREADS, int K, bool INLINE_ER, bool SYM>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void ehyb_ell_k_kernel(const EllArgs A, const long long ldx,
                                                                                                       const long long ldy)
{
    extern __shared__ __attribute__((aligned(16))) double win[];
    int* next_slab = reinterpret_cast<int*>(win + K * A.win_cap);  // one word behind the K window images
    const int4 it = A.items[2 * item_of_block(A.item_map, A.xcd_map, A.reverse_items)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int sg = it.x; sg < it.y; ++sg) ell_segment_k<THREADS, K, INLINE_ER, SYM>(A, ldx, ldy, win, next_slab, sg, lane, wave);
}

// ------------------------------------------------------------------ residual segments, K columns
// er_bin of ehyb_hip.hip with K columns: per column the same chain of FMAs and the same shuffle reduction.
template <int G, int THREADS, bool ASSIGN, int K>
__device__ __forceinline__ void er_bin_k(int lo, int hi, const int64_t* __restrict__ seg_ptr, const int* __restrict__ seg_row,
                                         const int* __restrict__ col, const double* __restrict__ val, const double* __restrict__ x, long long ldx,
                                         double* __restrict__ y, long long ldy)
{
    constexpr int SEGS = THREADS / G;
    const int sub = threadIdx.x % G;
    for (int base = lo; base < hi; base += SEGS) {  // uniform trip count: every lane reaches the shuffles
        const int seg = base + threadIdx.x / G;
        double acc0[K], acc1[K], y_old[K];
#pragma unroll
        for (int j = 0; j < K; ++j) acc0[j] = 0.0, acc1[j] = 0.0, y_old[j] = 0.0;
        int r = 0;
        if (seg < hi) {
            const int64_t b = seg_ptr[seg], e = seg_ptr[seg + 1];
            r = seg_row[seg];
            if (!ASSIGN && sub == 0 && r >= 0)
#pragma unroll
                for (int j = 0; j < K; ++j) y_old[j] = y[r + j * ldy];
            int64_t k = b + sub;
            for (; k + 3 * G < e; k += 4 * G) {
                const int c0 = col[k], c1 = col[k + G], c2 = col[k + 2 * G], c3 = col[k + 3 * G];
                const double v0 = val[k], v1 = val[k + G], v2 = val[k + 2 * G], v3 = val[k + 3 * G];
                double x0[K], x1[K], x2[K], x3[K];
#pragma unroll
                for (int j = 0; j < K; ++j) x0[j] = x[c0 + j * ldx], x1[j] = x[c1 + j * ldx], x2[j] = x[c2 + j * ldx], x3[j] = x[c3 + j * ldx];
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    acc0[j] = fma(v0, x0[j], acc0[j]);
                    acc1[j] = fma(v1, x1[j], acc1[j]);
                    acc0[j] = fma(v2, x2[j], acc0[j]);
                    acc1[j] = fma(v3, x3[j], acc1[j]);
                }
            }
            const bool h0 = k < e, h1 = k + G < e, h2 = k + 2 * G < e;
            const int c0 = h0 ? col[k] : 0, c1 = h1 ? col[k + G] : 0, c2 = h2 ? col[k + 2 * G] : 0;
            const double v0 = h0 ? val[k] : 0.0, v1 = h1 ? val[k + G] : 0.0, v2 = h2 ? val[k + 2 * G] : 0.0;
            double x0[K], x1[K], x2[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                x0[j] = h0 ? x[c0 + j * ldx] : 0.0;
                x1[j] = h1 ? x[c1 + j * ldx] : 0.0;
                x2[j] = h2 ? x[c2 + j * ldx] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                acc0[j] = fma(v0, x0[j], acc0[j]);
                acc1[j] = fma(v1, x1[j], acc1[j]);
                acc0[j] = fma(v2, x2[j], acc0[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            double acc = acc0[j] + acc1[j];
#pragma unroll
            for (int off = G / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, G);
            if (sub == 0 && seg < hi) {
                if (ASSIGN)
                    y[r + j * ldy] = acc;
                else if (r < 0)
                    unsafeAtomicAdd(&y[(r & 0x7fffffff) + j * ldy], acc);
                else
                    y[r + j * ldy] = y_old[j] + acc;
            }
        }
    }
}

template <int THREADS, bool ASSIGN, int K>
__global__ __launch_bounds__(THREADS) void ehyb_er_k_kernel(const int4* __restrict__ blocks, const int64_t* __restrict__ seg_ptr,
                                                            const int* __restrict__ seg_row, const int* __restrict__ col,
                                                            const double* __restrict__ val, const double* __restrict__ x, const long long ldx,
                                                            double* __restrict__ y, const long long ldy)
{
    const int4 b = blocks[blockIdx.x];
    if (b.z == 64)
        er_bin_k<64, THREADS, ASSIGN, K>(b.x, b.y, seg_ptr, seg_row, col, val, x, ldx, y, ldy);
    else if (b.z == 16)
        er_bin_k<16, THREADS, ASSIGN, K>(b.x, b.y, seg_ptr, seg_row, col, val, x, ldx, y, ldy);
    else
        er_bin_k<4, THREADS, ASSIGN, K>(b.x, b.y, seg_ptr, seg_row, col, val, x, ldx, y, ldy);
}

// ------------------------------------------------------------------ launches
// Widest pass of a plan: the K window images and the slab counter must fit the 160 KiB of LDS.
static int spmm_width(const HostLayout& H)
{
    if (H.er_panel || H.deferred.pending) return 1;  // a panel-form residual multiplies one vector per pass
    if (H.direct) return kSpmmMaxK;                   // no window
    const int64_t cap = ell_win_cap(H);
    if (cap <= 0) return kSpmmMaxK;
    return (int)std::max<int64_t>(1, std::min<int64_t>(kSpmmMaxK, ((int64_t)EHYB_LDS_MAX_DOUBLES * 8 - 16) / (8 * cap)));
}

template <int K>
static void ell_k_go(const EllArgs& A, int threads, bool inl, bool sym, int n_items, size_t lds, hipStream_t st, long long ldx, long long ldy)
{
#define ELLK_GO(T, I, S) hipLaunchKernelGGL((ehyb_ell_k_kernel<T, K, I, S>), dim3(n_items), dim3(T), lds, st, A, ldx, ldy)
#define ELLK_T(T)                   \
    if (sym) {                      \
        if (inl) ELLK_GO(T, true, true);  \
        else ELLK_GO(T, false, true);     \
    } else {                        \
        if (inl) ELLK_GO(T, true, false); \
        else ELLK_GO(T, false, false);    \
    }
    if (threads == 256) { ELLK_T(256) }
    else if (threads == 512) { ELLK_T(512) }
    else { ELLK_T(1024) }
#undef ELLK_T
#undef ELLK_GO
}

static int launch_ell_k(ehyb_plan* P, const double* X, long long ldx, double* Y, long long ldy, int k, hipStream_t st, bool inl, int walk)
{
    const HostLayout& H = P->host;
    const int n_items = (int)(H.items.size() / 8);
    if (n_items == 0 || H.direct) return EHYB_OK;
    if (H.pb_assign && H.segs.empty()) return EHYB_OK;
    if (P->cfg.threads != 256 && P->cfg.threads != 512 && P->cfg.threads != 1024)
        EHYB_FAIL(EHYB_ERR_ARG, "ELL workgroup size %d not built (256/512/1024)", P->cfg.threads);
    const size_t lds = (size_t)k * ell_win_cap(H) * 8 + 16;
    EllArgs A = ell_args(P, X, Y, nullptr);
    ell_walk(P, walk, n_items, lds, &A);
    if (k == 2) ell_k_go<2>(A, P->cfg.threads, inl, H.sym, n_items, lds, st, ldx, ldy);
    else if (k == 3) ell_k_go<3>(A, P->cfg.threads, inl, H.sym, n_items, lds, st, ldx, ldy);
    else ell_k_go<4>(A, P->cfg.threads, inl, H.sym, n_items, lds, st, ldx, ldy);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

template <int K>
static void er_k_go(const ehyb_plan* P, int n_blocks, hipStream_t st, const double* X, long long ldx, double* Y, long long ldy)
{
    if (P->host.direct)
        hipLaunchKernelGGL((ehyb_er_k_kernel<256, true, K>), dim3(n_blocks), dim3(256), 0, st, (const int4*)P->d_er_blocks, P->d_er_seg_ptr,
                           P->d_er_seg_row, P->d_er_col, P->d_er_val, X, ldx, Y, ldy);
    else
        hipLaunchKernelGGL((ehyb_er_k_kernel<256, false, K>), dim3(n_blocks), dim3(256), 0, st, (const int4*)P->d_er_blocks, P->d_er_seg_ptr,
                           P->d_er_seg_row, P->d_er_col, P->d_er_val, X, ldx, Y, ldy);
}

static int launch_er_k(ehyb_plan* P, const double* X, long long ldx, double* Y, long long ldy, int k, hipStream_t st)
{
    const HostLayout& H = P->host;
    if (H.er_bins[3] == 0) return EHYB_OK;
    const int n_blocks = (int)(H.er_blocks.size() / 4);
    if (P->cfg.er_threads != 256) EHYB_FAIL(EHYB_ERR_ARG, "residual workgroup size %d not built (256)", P->cfg.er_threads);
    if (k == 2) er_k_go<2>(P, n_blocks, st, X, ldx, Y, ldy);
    else if (k == 3) er_k_go<3>(P, n_blocks, st, X, ldx, Y, ldy);
    else er_k_go<4>(P, n_blocks, st, X, ldx, Y, ldy);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

int spmm_set_lds_attr(int lds)
{
#define LDS_ATTR(KERN) HIP_TRY(hipFuncSetAttribute((const void*)(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
#define LDS_ATTR_K(T, K)                                  \
    LDS_ATTR((ehyb_ell_k_kernel<T, K, false, false>))     \
    LDS_ATTR((ehyb_ell_k_kernel<T, K, true, false>))      \
    LDS_ATTR((ehyb_ell_k_kernel<T, K, false, true>))      \
    LDS_ATTR((ehyb_ell_k_kernel<T, K, true, true>))
#define LDS_ATTR_T(T) LDS_ATTR_K(T, 2) LDS_ATTR_K(T, 3) LDS_ATTR_K(T, 4)
    LDS_ATTR_T(256)
    LDS_ATTR_T(512)
    LDS_ATTR_T(1024)
#undef LDS_ATTR_T
#undef LDS_ATTR_K
#undef LDS_ATTR
    return EHYB_OK;
}

int ehyb_spmm_max_k(const ehyb_plan* P, int* k_max)
{
    clear_error();
    if (!P || !k_max) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm_max_k: null argument");
    *k_max = spmm_width(P->host);
    return EHYB_OK;
}

int ehyb_spmm(ehyb_plan* P, const double* X, int64_t ldx, double* Y, int64_t ldy, int k, void* stream, int walk)
{
    clear_error();
    if (!P || !X || !Y) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm: null argument");
    if (k < 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm: k = %d columns (at least 1)", k);
    const HostLayout& H = P->host;
    if (ldx < H.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm: ldx %lld < %d columns of the matrix", (long long)ldx, H.n_cols);
    if (ldy < H.row_end) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm: ldy %lld < %d rows", (long long)ldy, H.row_end);
    if (walk < -1 || walk > 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm: walk %d (EHYB_WALK_AUTO, _FIRST_TO_LAST, _LAST_TO_FIRST)", walk);
    if (!P->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_spmm: plan not uploaded (no CPU fallback exists)");
    hipStream_t st = (hipStream_t)stream;
    // ceil(k / k_max) passes over the matrix, as even as they come (k = 5 on a plan of k_max 4: 3 + 2)
    const int kmax = spmm_width(H), passes = (k + kmax - 1) / kmax;
    int j0 = 0;
    for (int p = 0; p < passes; ++p) {
        const int w = k / passes + (p < k % passes ? 1 : 0);
        const double* Xp = X + (int64_t)j0 * ldx;
        double* Yp = Y + (int64_t)j0 * ldy;
        int rc;
        if (w == 1) {
            rc = ehyb_spmv_walk(P, Xp, Yp, stream, walk);  // the one-vector launch sequence
        } else {
            rc = launch_ell_k(P, Xp, ldx, Yp, ldy, w, st, H.inline_er, walk);
            if (rc == EHYB_OK && !H.inline_er) rc = launch_er_k(P, Xp, ldx, Yp, ldy, w, st);
        }
        if (rc != EHYB_OK) return rc;
        j0 += w;
    }
    return EHYB_OK;
}
