// HIP kernels for gfx950 (MI355X, CDNA4) and the device half of the C-ABI.
//
// Kernels (replace reference kernel.cu:43-284; this file holds their thin entry points, the bodies are in ell_device.h and
// panel_device.h):
//   ehyb_ell_kernel  one workgroup per work item = a run of 64-row slabs of (nearly) equal byte
//                    count, cut into segments at partition boundaries.  Per segment:
//                      1. stage the partition's x-window into LDS -- contiguous own segment
//                         (coalesced) + gathered halo columns (the "explicit cache",
//                         kernel.cu:137-141, grown to <= 160 KiB per workgroup);
//                      2. every wave64 takes slabs from an LDS counter (the reference's per-block
//                         work queue, kernel.cu:142,164-166 -- here re-armed per segment, so
//                         nothing survives a launch); per lane one row, per step one 16-byte
//                         value pair (global_load_dwordx4, 1 KiB per wave) and one 4-byte word
//                         holding two 16-bit window-local columns (shared by lanes with equal
//                         column lists), two LDS gathers (ds_read_b64) and two fp64 FMAs
//                         (kernel.cu:150-163);
//                      3. y[row] = dot, 512 B coalesced per slab.
//                    Two more forms of the same kernel:
//                      INLINE_ER  a tiny residual rides along as extra pairs behind every slab's
//                                 ELL pairs (global columns, x gathered from L2): one launch;
//                      SYM        symmetric pair storage: one workgroup per partition, the rows'
//                                 accumulators in LDS behind the x image; an entry marked in bit 15
//                                 of its column also adds value * x[own row] to row `column`
//                                 (ds_add_f64), so an in-partition pair a_ij == a_ji is read once.
//                    ehyb_ell_k_kernel is the same kernel for K = 2, 3, 4 columns (ehyb_spmm).
//   ehyb_er_kernel   CSR residual: G lanes per segment (64/16/4 by segment length), strided
//                    coalesced (col,val) reads, x gathered from global memory (L2/MALL),
//                    wavefront shuffle reduction, y[row] += sum -- or one fp64 atomic per
//                    segment for rows split into several segments (the working form of
//                    kernel.cu:43-67 longRowKernel).  Runs on every multiply that has a residual
//                    not carried inline (the reference skips it after the first launch: SURVEY 8
//                    a-10 item 1); it is also phase 2 of the multi-GPU multiply (all remote columns).
//                    ehyb_er_k_kernel: the same for K = 2, 3, 4 columns.
//   ehyb_pb_scale_kernel / ehyb_pb_reduce_kernel  the two passes of the panel-form residual (bodies in panel_device.h, written
//                    once for K columns); ehyb_pb_scale_k_kernel / ehyb_pb_reduce_k_kernel: the same for K = 2, 3, 4 columns.
//   launch_window / launch_er_csr / launch_panel_scale + launch_panel_reduce  the one launch path of each family (of each pass
//                    of the panel family), for every K; each looks its kernel up in a table of the family's instantiations.
// No MFMA: 2 flops per 5.8-10 streamed bytes, HBM-bound.
//
// Arms tried and dropped (measurements in DESIGN.md 3.1): software-pipelined slab walk with ping-pong
// register groups, 4-deep unrolled double2 staging, early slab-record loads, batched remainder
// pairs, global slab counters with work stealing, an 8-pair step for SYM.  The decisive levers were
// bytes (shared column lists, symmetric pairs) and scheduling (equal-cost items, one resident wave).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "ehyb_internal.h"
#include "hip_try.h"
#include "col_triples.h"
#include "ell_device.h"
#include "panel_device.h"

using namespace ehyb;

// ------------------------------------------------------------------ window kernel and CSR residual (bodies: ell_device.h)
// Thin entry points over the K-templated bodies: one instantiation per (workgroup size, K, walk form, inline residual,
// storage); their names and arguments are what profiles, bench.py and tools/pmc_parse.py know.
// Plain: <= 64 VGPRs (8 waves per SIMD), so that two 1024-thread workgroups share a CU when the caller picks
// a window of <= 80 KiB; at the default 160 KiB window one runs per CU (an 8-pair step with 128 VGPRs was
// measured there too: no gain).  SYM always runs one workgroup per CU (its window holds x and the y
// accumulators): 4 waves per SIMD, up to 128 VGPRs, no spills.
// (The stamped instantiations, diagnostic, carry both forms of the column words like every other and the stamps on top: they
// get the 128 VGPRs of SYM with plain storage too, rather than spill.)
template <int THREADS, bool DYN, bool STAMP, bool INLINE_ER, bool SYM>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu((SYM || STAMP) ? 4 : 8, 8))) void ehyb_ell_kernel(const EllArgs A)
{
    ell_items<THREADS, 1, DYN, STAMP, INLINE_ER, SYM>(A, 0, 0);
}

// A K-wide window fills the CU: one workgroup per CU for every K and storage, up to 128 VGPRs.
template <int THREADS, int K, bool INLINE_ER, bool SYM>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void ehyb_ell_k_kernel(const EllArgs A, const long long ldx,
                                                                                                       const long long ldy)
{
    ell_items<THREADS, K, true, false, INLINE_ER, SYM>(A, ldx, ldy);
}

// cfg.val_f32: the one-vector kernel over a value stream held in fp32 ([pair][lane][2] floats, 8 B per lane and pair): the same
// body with float2 loads, LDS slab counter, no stamps.  Plain storage without an inline residual keeps the 64 VGPRs of the fp64
// kernel; with an inline residual the conversions on top of both forms of the column words spilled there (20 B per lane), so that
// arm takes the 128 VGPRs of SYM: one workgroup of 1024 threads per CU whatever the window.
template <int THREADS, bool INLINE_ER, bool SYM>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu((SYM || INLINE_ER) ? 4 : 8, 8))) void ehyb_ell_f32_kernel(const EllArgs A)
{
    ell_items<THREADS, 1, true, false, INLINE_ER, SYM, float2>(A, 0, 0);
}

// Two-launch form (multi-GPU phase 2, or a residual too large to ride in the window launch).
template <int THREADS, bool ASSIGN>
__global__ __launch_bounds__(THREADS) void ehyb_er_kernel(const int4* __restrict__ blocks,
                                                          const int64_t* __restrict__ seg_ptr,
                                                          const int* __restrict__ seg_row,
                                                          const int* __restrict__ col,
                                                          const double* __restrict__ val,
                                                          const double* __restrict__ x, double* __restrict__ y)
{
    er_blocks<THREADS, ASSIGN, 1>(blocks, seg_ptr, seg_row, col, val, x, 0, y, 0);
}

// cfg.val_f32: one float per residual entry
template <int THREADS, bool ASSIGN>
__global__ __launch_bounds__(THREADS) void ehyb_er_f32_kernel(const int4* __restrict__ blocks, const int64_t* __restrict__ seg_ptr,
                                                              const int* __restrict__ seg_row, const int* __restrict__ col,
                                                              const float* __restrict__ val, const double* __restrict__ x, double* __restrict__ y)
{
    er_blocks<THREADS, ASSIGN, 1, float>(blocks, seg_ptr, seg_row, col, val, x, 0, y, 0);
}

template <int THREADS, bool ASSIGN, int K>
__global__ __launch_bounds__(THREADS) void ehyb_er_k_kernel(const int4* __restrict__ blocks, const int64_t* __restrict__ seg_ptr,
                                                            const int* __restrict__ seg_row, const int* __restrict__ col,
                                                            const double* __restrict__ val, const double* __restrict__ x, const long long ldx,
                                                            double* __restrict__ y, const long long ldy)
{
    er_blocks<THREADS, ASSIGN, K>(blocks, seg_ptr, seg_row, col, val, x, ldx, y, ldy);
}

// ------------------------------------------------------------------ panel residual (bodies: panel_device.h)
// Pass 1, one vector: SUMS_DPP = the register scan (false: the LDS-sum A/B arm), PROBE = the timing-diagnostics instantiation;
// eight chunks per wave and step.
template <int THREADS, bool SUMS_DPP, bool PROBE>
__global__ __launch_bounds__(THREADS) void ehyb_pb_scale_kernel(const int2* __restrict__ items, const int4* __restrict__ units, const double* __restrict__ val,
                                                                const uint16_t* __restrict__ colf, const uint32_t* __restrict__ chunk,
                                                                const uint32_t* __restrict__ jump, const double* __restrict__ x, double* __restrict__ partial,
                                                                int panel_cols, int probe_arg, int xcd_map, int* __restrict__ queue, int n_items, int reverse)
{
    pb_scale_body<THREADS, SUMS_DPP, PROBE, 8>(items, units, val, colf, chunk, jump, x, partial, panel_cols, probe_arg, xcd_map, queue, n_items, reverse);
}

// Pass 1 for NV = 2, 3, 4 columns (ehyb_spmm).  At most 128 VGPRs: four waves per SIMD are one 1024-thread workgroup or two of
// 512 threads per CU, as for one vector.  Chunks per wave and step: 8 (NV = 2), 6, 4 -- the NV gathered x values per chunk are
// what the registers go to: 87 / 85 / 76 VGPRs, no scratch.
template <int THREADS, int NV>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void ehyb_pb_scale_k_kernel(
    const int2* __restrict__ items, const int4* __restrict__ units, const double* __restrict__ val, const uint16_t* __restrict__ colf,
    const uint32_t* __restrict__ chunk, const uint32_t* __restrict__ jump, const double* __restrict__ x, const long long ldx, double* __restrict__ partial,
    int panel_cols, int xcd_map, int* __restrict__ queue, int n_items, int reverse)
{
    pb_scale_body<THREADS, true, false, (NV == 2 ? 8 : NV == 3 ? 6 : 4), NV>(items, units, val, colf, chunk, jump, x, partial, panel_cols, 0, xcd_map, queue, n_items,
                                                                            reverse, ldx);
}

// Pass 2 (NT: partial sums and row words streamed past the caches)
template <int THREADS, bool NT>
__global__ __launch_bounds__(THREADS) void ehyb_pb_reduce_kernel(const int4* __restrict__ units, const double* __restrict__ partial,
                                                                 const uint16_t* __restrict__ row, double* __restrict__ y, int probe)
{
    pb_reduce_body<THREADS, NT, 1>(units, partial, row, y, 0, probe);
}

template <int THREADS, bool NT, int NV>
__global__ __launch_bounds__(THREADS) void ehyb_pb_reduce_k_kernel(const int4* __restrict__ units, const double* __restrict__ partial,
                                                                   const uint16_t* __restrict__ row, double* __restrict__ y, const long long ldy)
{
    pb_reduce_body<THREADS, NT, NV>(units, partial, row, y, ldy, 0);
}

// dst[i] = src[idx[i]]: the send list of a halo exchange (multi-GPU), four gathers per thread in flight
__global__ __launch_bounds__(256) void ehyb_gather_kernel(const double* __restrict__ src, const int32_t* __restrict__ idx, double* __restrict__ dst, long long n)
{
    const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    int32_t k[4];
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = base + j < n ? idx[base + j] : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = base + j < n ? src[k[j]] : 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < n) dst[base + j] = v[j];
}

// y[idx[i]] += src[i]: partial sums computed elsewhere, added into this rank's rows (an index may occur more than once)
__global__ __launch_bounds__(256) void ehyb_scatter_add_kernel(double* __restrict__ y, const int32_t* __restrict__ idx, const double* __restrict__ src, long long n)
{
    const long long base = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    int32_t k[4];
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = base + j < n ? idx[base + j] : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = base + j < n ? src[base + j] : 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < n) unsafeAtomicAdd(&y[k[j]], v[j]);
}

// streaming-read probe for the on-box bandwidth ceiling
__global__ __launch_bounds__(256) void ehyb_read_kernel(const double2* __restrict__ src, size_t n2, double* sink)
{
    double acc = 0.0;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        double2 v = src[i];
        acc += v.x + v.y;
    }
    if (acc == 123.456) sink[0] = acc;  // keep the loads alive
}

// ------------------------------------------------------------------ launches
// ---- which slabs of the window kernel's value stream stay in the Infinity Cache (ell_device.h: ell_slab_resident)
constexpr long long kInfinityCache = 256ll << 20;
// The share of the cache a pinned set may take of what the launch's other traffic leaves (chosen from tools/resident_sweep.py:
// profiles/r05_resident_sweep.txt)
constexpr double kEllKeepSafety = 0.9;

// The automatic share of a value stream of `value_bytes` that is pinned, in 1/1024: what the cache holds beside the bytes the
// launch reads again and writes with plain accesses (column words, lane maps, slab records, items, x, y, halo lists), times
// the safety factor; all of a stream that fits the cache together with them.
static int ell_auto_keep1024(long long value_bytes, long long plain_bytes)
{
    if (value_bytes <= 0 || value_bytes + plain_bytes <= kInfinityCache) return 1024;
    const double room = std::max(0.0, (double)(kInfinityCache - plain_bytes)) * kEllKeepSafety;
    return (int)std::min(1024.0, std::floor(1024.0 * room / (double)value_bytes));
}

// successive launches of the plan walk in alternating directions by themselves (cfg.ell_alternate): where the stream does not
// fit the cache but the cache is still a fair share of it.  A pinned set is the same for both directions: such plans do not alternate.
// Bytes of the window launch's value stream and of everything it reads as the DEVICE holds them: cfg.val_f32 takes 4 B off
// every value slot (stats, a property of the host layout, count 8)
static long long ell_value_bytes(const ehyb_plan* P) { return (P->cfg.val_f32 == 1 ? 4 : 8) * (long long)P->host.stats.size_block_ell; }
static long long ell_format_bytes(const ehyb_plan* P)
{
    const ehyb_stats& S = P->host.stats;
    return S.bytes_format_ell - (P->cfg.val_f32 == 1 ? 4 * (long long)(S.size_block_ell + (P->host.inline_er ? S.er_inline : 0)) : 0);
}

static bool ell_alternates(const ehyb_plan* P)
{
    const long long b = ell_format_bytes(P);
    const bool pinned = P->cfg.ell_nt == 4 || P->cfg.ell_nt == 5;
    return P->cfg.ell_alternate == 1 || (P->cfg.ell_alternate == 0 && !pinned && b > kInfinityCache && b <= (8192ll << 20));
}

// cfg.ell_nt -> (keep1024, shape) of a launch; alternating_walk: the launch is one of an alternating walk (ell_walk)
static void ell_keep_rule(const ehyb_plan* P, bool alternating_walk, int* keep1024, int* shape)
{
    const long long format_bytes = ell_format_bytes(P);
    const int nt = P->cfg.ell_nt;
    // a stream the 256 MB Infinity Cache holds whole stays there from one multiply to the next: plain loads (120 k rows, 65 MB: 15.4 us, with
    // the hint 16.2)
    const bool fits = format_bytes <= kInfinityCache;
    *shape = nt == 4 ? ELL_KEEP_SPREAD : (nt == 5 ? ELL_KEEP_BLOCK : ELL_KEEP_WALK_END);
    if (nt == 1 || nt == 2) {
        *keep1024 = nt == 2 ? 1024 : 0;   // the A/B arms: never / always the hint
    } else if (nt == 4 || nt == 5) {
        const long long value_bytes = ell_value_bytes(P);  // (the plain bytes -- everything else -- do not depend on cfg.val_f32)
        *keep1024 = P->cfg.ell_keep > 0 ? (int)((long long)P->cfg.ell_keep * 1024 / 1000) : ell_auto_keep1024(value_bytes, P->host.stats.bytes_format_ell - 8 * (long long)P->host.stats.size_block_ell);
    } else if (fits) {
        *keep1024 = 1024;
    } else if (alternating_walk) {
        // cfg.ell_nt = 3: the END of every walk -- the share of the stream the cache can hold -- is read with plain loads, so that it is
        // still there when the next launch starts from that end (half, three quarters and five quarters of that share measured level:
        // profiles/r04_nt_hints_ab.txt)
        const double keep = std::min(1.0, (double)kInfinityCache / (double)std::max<long long>(1, format_bytes));
        *keep1024 = 1024 - (int)(1024.0 * (1.0 - keep));
    } else {
        *keep1024 = 0;
    }
}

static thread_local int t_probe_n = 0;   // ehyb_debug_ell_stamps_probe: the stamped launch stages every window entry from three vectors
static EllArgs ell_args(ehyb_plan* P, const double* x, double* y, unsigned long long* stamps, double* xy_out)
{
    EllArgs A;
    A.items = (const int4*)P->d_items;
    A.segs = (const int4*)P->d_segs;
    A.halo_cols = P->d_halo_cols;
    A.slab_meta = (const uint4*)P->d_slab_meta;
    A.lane_group = P->d_lane_group;
    A.slab_lrow = P->d_slab_lrow;
    A.ell_val = (const double2*)P->d_ell_val;
    A.ell_col = P->d_ell_col;
    A.x = x;
    A.y = y;
    A.win_cap = ell_win_cap(P->host);
    A.stamps = stamps;
    A.xy_out = xy_out;
    A.reverse = 0;
    A.reverse_items = 0;
    A.probe_n = stamps ? t_probe_n : 0;
    ell_keep_rule(P, false, &A.keep1024, &A.keep_shape);
    // on by default: plain storage 143 -> 134 us on the audikw_1-like matrix; cfg.xcd_map = 2 for the A/B
    A.xcd_map = P->host.sym ? 0 : (P->cfg.xcd_map != 2 ? 1 : 0);
    A.item_map = P->d_item_map;  // symmetric pairs: items are sorted heaviest first, dispatched in that order
    A.windowless_zero = P->host.pb_assign ? 0 : 1;
    return A;
}

// (the transposed window launch, ehyb_spmv_t.hip, takes the same arguments)
EllArgs ehyb::window_launch_args(ehyb_plan* P, const double* x, double* y) { return ell_args(P, x, y, nullptr, nullptr); }

// The walk of a launch: walk >= 0 the caller's explicit direction (ehyb_spmv_walk, ehyb_spmm), -1 the plan's own alternation.
// (automatic: where the stream does not fit the cache but the cache is still a fair share of it -- the walk from the short slabs
// up costs the tail of a workgroup a few per cent: audikw_1-like, 439 MB, 83.5 -> 76.0 us; every entry stored, 729 MB, 143.3 ->
// 136.8; 120 k rows, 65 MB, 15.4 -> 16.2; kkt3d-200, 2.56 GB, 501.9 -> 473.7 once the items are taken from the far end too)
static void ell_walk(ehyb_plan* P, int walk, int n_items, size_t lds, EllArgs* A)
{
    if (walk >= 0 || ell_alternates(P)) {
        // the caller's explicit direction (ehyb_spmv_walk), else the plan's own alternation: an atomic flip, so that every one of
        // several threads launching the same plan draws a direction (plain storage: the result does not depend on it)
        A->reverse = walk >= 0 ? (walk & 1) : (P->launch_parity.fetch_xor(1, std::memory_order_relaxed) & 1);
        // more than one round of workgroups: what ran in the last round is what the cache holds, so it runs first now
        A->reverse_items = (A->reverse && n_items > kNumCU * (lds > 80 * 1024 ? 1 : 2)) ? 1 : 0;
        ell_keep_rule(P, true, &A->keep1024, &A->keep_shape);   // (cfg.ell_nt = 3: the end of an alternating walk is read with plain loads)
    }
}

// The walk direction a caller asked for (ehyb_spmv_walk) while its call is on the stack: -1 = the plan's own alternation.
static thread_local int t_walk = -1;
namespace {
struct WalkScope {
    int saved;
    explicit WalkScope(int w) : saved(t_walk) { t_walk = w; }
    ~WalkScope() { t_walk = saved; }
};
}  // namespace

// Every window-kernel instantiation: the one-vector kernel with both slab walks (DYN), plain and stamped; the k-vector kernel
// for K = 2..kSpmmMaxK with the LDS counter only.  Behind every window launch and the LDS opt-in of ehyb_plan_upload.
struct EllKernel {
    int threads, k;
    bool dyn, stamp, inl, sym;
    const void* fn;
    bool f32 = false;  // cfg.val_f32: ehyb_ell_f32_kernel
};

template <int T, int K, bool DYN, bool STAMP, bool INL, bool SYM>
static EllKernel ell_kernel()
{
    if constexpr (K == 1)
        return {T, K, DYN, STAMP, INL, SYM, (const void*)ehyb_ell_kernel<T, DYN, STAMP, INL, SYM>};
    else
        return {T, K, DYN, STAMP, INL, SYM, (const void*)ehyb_ell_k_kernel<T, K, INL, SYM>};
}

// the four forms (inline residual or not, symmetric pairs or not) of one workgroup size, K, walk and stamping
template <int T, int K, bool DYN = true, bool STAMP = false>
static void add_ell_kernels(std::vector<EllKernel>* v)
{
    v->insert(v->end(), {ell_kernel<T, K, DYN, STAMP, false, false>(), ell_kernel<T, K, DYN, STAMP, true, false>(),
                         ell_kernel<T, K, DYN, STAMP, false, true>(), ell_kernel<T, K, DYN, STAMP, true, true>()});
}

template <int T>
static void add_ell_kernels(std::vector<EllKernel>* v)
{
    add_ell_kernels<T, 1, true, false>(v);
    add_ell_kernels<T, 1, false, false>(v);
    add_ell_kernels<T, 1, true, true>(v);
    add_ell_kernels<T, 1, false, true>(v);
    add_ell_kernels<T, 2>(v);
    add_ell_kernels<T, 3>(v);
    add_ell_kernels<T, 4>(v);
    v->insert(v->end(), {{T, 1, true, false, false, false, (const void*)ehyb_ell_f32_kernel<T, false, false>, true},
                         {T, 1, true, false, true, false, (const void*)ehyb_ell_f32_kernel<T, true, false>, true},
                         {T, 1, true, false, false, true, (const void*)ehyb_ell_f32_kernel<T, false, true>, true},
                         {T, 1, true, false, true, true, (const void*)ehyb_ell_f32_kernel<T, true, true>, true}});
}

static const std::vector<EllKernel>& ell_kernels()
{
    static const std::vector<EllKernel> all = [] {
        std::vector<EllKernel> v;
        add_ell_kernels<1024>(&v);  // (the default size first: the launches look their kernel up here)
        add_ell_kernels<512>(&v);
        add_ell_kernels<256>(&v);
        return v;
    }();
    return all;
}

int ehyb::launch_window(ehyb_plan* P, const double* x, long long ldx, double* y, long long ldy, int k, hipStream_t st, bool inl, int walk,
                        unsigned long long* stamps, double* xy_out)
{
    const HostLayout& H = P->host;
    const int n_items = (int)(H.items.size() / kItemWords);
    if (n_items == 0 || H.direct) return EHYB_OK;  // direct shape: the row-segment kernel does everything
    if (H.pb_assign && H.segs.empty()) return EHYB_OK;  // no partition kept its window: pass 2 of the panel residual assigns every row
    // cfg.ell_variant: 0/1 = LDS slab counter (default), 3 = static round-robin (A/B arm, tools/sweep.py --variants; one vector only)
    const bool dyn = k > 1 || P->cfg.ell_variant != 3;
    const bool f32 = P->cfg.val_f32 == 1;
    if (f32 && (k > 1 || !dyn || stamps))
        EHYB_FAIL(EHYB_ERR_ARG, "window launch: cfg.val_f32 serves one column, the LDS slab counter and no stamps (%d columns%s%s)", k,
                  dyn ? "" : ", cfg.ell_variant = 3", stamps ? ", a stamped or probe launch" : "");
    const void* fn = nullptr;
    const std::vector<EllKernel>& table = ell_kernels();
    size_t row = 0;
    for (; row < table.size(); ++row) {
        const EllKernel& e = table[row];
        if (e.f32 == f32 && e.threads == P->cfg.threads && e.k == k && e.dyn == dyn && e.stamp == (stamps != nullptr) && e.inl == inl && e.sym == H.sym) {
            fn = e.fn;
            break;
        }
    }
    if (!fn) EHYB_FAIL(EHYB_ERR_ARG, "ELL workgroup size %d not built (256/512/1024)", P->cfg.threads);
    if (P->d_triples && k >= kNoTripleArmK && inl && H.sym)  // (plan_keeps_pair_words keeps such a plan in the pair form)
        EHYB_FAIL(EHYB_ERR_INTERNAL, "window launch: %d columns with symmetric pairs and an inline residual on triple-coded column words", k);
    const size_t lds = ell_lds_bytes(H, k);
    EllArgs A = ell_args(P, x, y, stamps, xy_out);
    if (stamps)
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    else
        ell_walk(P, walk, n_items, lds, &A);
    void* args[] = {&A, &ldx, &ldy};  // (the one-vector kernel takes A alone)
    P->mark_launched(EHYB_KERNELS_WINDOW, row);
    (void)hipLaunchKernel(fn, dim3(n_items), dim3(P->cfg.threads), args, lds, st);  // as <<< >>>: a failed launch is the last error
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

static int launch_ell(ehyb_plan* P, const double* x, double* y, hipStream_t st, bool inl)
{
    return launch_window(P, x, 0, y, 0, 1, st, inl, t_walk);
}

// y = A x with x . y as a by-product (ehyb_cg.hip): possible where ONE ELL launch writes the final y of every row from a
// window that holds the row's own x -- no residual launch of its own (empty or inline residual), halo windows, not the direct
// shape.  -> number of partial sums the launch leaves (one per workgroup), 0 = not this plan.
int ehyb::spmv_xy_partials(const ehyb_plan* P)
{
    const HostLayout& H = P->host;
    const int n_items = (int)(H.items.size() / kItemWords);
    if (!P->uploaded || H.direct || n_items == 0 || H.pb_assign || P->cfg.window_mode != EHYB_WINDOW_HALO) return 0;
    if (H.stats.nnz_er > 0 && !H.inline_er) return 0;
    return n_items;
}
int ehyb::spmv_xy(ehyb_plan* P, const double* x, double* y, void* stream, double* xy_partials)
{
    if (spmv_xy_partials(P) == 0 || !x || !y || !xy_partials) EHYB_FAIL(EHYB_ERR_STATE, "spmv_xy: not a plan that multiplies in one window launch");
    return launch_window(P, x, 0, y, 0, 1, (hipStream_t)stream, P->host.inline_er, t_walk, nullptr, xy_partials);
}

// ---- panel residual
// Every instantiation of the two passes: pass 1 in both workgroup sizes -- one vector with register-scan or LDS sums (dpp), plain
// and with the timing probes; k = 2..kSpmmMaxK with register-scan sums only --, pass 2 with and without the streaming hint (nt)
// for every k.  Behind both launches and the LDS opt-in of ehyb_plan_upload.  (A field its pass does not have holds one value.)
struct PanelKernel { int pass, threads, k; bool dpp, probe, nt; const void* fn; };

template <int T>
static void add_panel_scale_kernels(std::vector<PanelKernel>* v)
{
    v->insert(v->end(), {{1, T, 1, true, false, false, (const void*)ehyb_pb_scale_kernel<T, true, false>}, {1, T, 1, false, false, false, (const void*)ehyb_pb_scale_kernel<T, false, false>},
                         {1, T, 1, true, true, false, (const void*)ehyb_pb_scale_kernel<T, true, true>}, {1, T, 1, false, true, false, (const void*)ehyb_pb_scale_kernel<T, false, true>},
                         {1, T, 2, true, false, false, (const void*)ehyb_pb_scale_k_kernel<T, 2>}, {1, T, 3, true, false, false, (const void*)ehyb_pb_scale_k_kernel<T, 3>},
                         {1, T, 4, true, false, false, (const void*)ehyb_pb_scale_k_kernel<T, 4>}});
}
template <bool NT>
static void add_panel_reduce_kernels(std::vector<PanelKernel>* v)
{
    v->insert(v->end(), {{2, 512, 1, true, false, NT, (const void*)ehyb_pb_reduce_kernel<512, NT>}, {2, 512, 2, true, false, NT, (const void*)ehyb_pb_reduce_k_kernel<512, NT, 2>},
                         {2, 512, 3, true, false, NT, (const void*)ehyb_pb_reduce_k_kernel<512, NT, 3>}, {2, 512, 4, true, false, NT, (const void*)ehyb_pb_reduce_k_kernel<512, NT, 4>}});
}

static const std::vector<PanelKernel>& panel_kernels()
{
    static const std::vector<PanelKernel> all = [] {
        std::vector<PanelKernel> v;
        add_panel_scale_kernels<512>(&v), add_panel_scale_kernels<1024>(&v);
        add_panel_reduce_kernels<false>(&v), add_panel_reduce_kernels<true>(&v);
        return v;
    }();
    return all;
}

// (each pass is looked up by the fields it has)  -> the table row, -1: not built
static int panel_scale_kernel(int threads, int k, bool dpp, bool probe)
{
    const std::vector<PanelKernel>& table = panel_kernels();
    for (size_t row = 0; row < table.size(); ++row) {
        const PanelKernel& e = table[row];
        if (e.pass == 1 && e.threads == threads && e.k == k && e.dpp == dpp && e.probe == probe) return (int)row;
    }
    return -1;
}
static int panel_reduce_kernel(int k, bool nt)
{
    const std::vector<PanelKernel>& table = panel_kernels();
    for (size_t row = 0; row < table.size(); ++row) {
        const PanelKernel& e = table[row];
        if (e.pass == 2 && e.k == k && e.nt == nt) return (int)row;
    }
    return -1;
}

// Dynamic LDS of a pass-1 launch: k interleaved panel images, the waves' piece accumulators (LDS sums only) and the word in which
// thread 0 hands over the item; of a pass-2 launch: k accumulators per row of the largest row block.
static size_t panel_scale_lds_bytes(const HostLayout& H, int k, bool dpp, int threads) { return ((size_t)k * H.pb_panel_cols + (dpp ? 0 : threads) + 1) * 8; }
static size_t panel_reduce_lds_bytes(const HostLayout& H, int k) { return (size_t)H.pb_rows_max * k * 8; }

static int panel_items(const HostLayout& H) { return (int)(H.pb_items1.size() / 2); }

// Pass 1 (scale) over the items [item_begin, item_end) for k columns of x, ldx doubles apart; probe: ehyb_debug_panel_times only.
// (k > 1, ehyb_spmm: register-scan sums whatever cfg.er_sums says -- the LDS-sum A/B arm is one vector wide -- and no probes)
static int launch_panel_scale(ehyb_plan* P, const double* x, long long ldx, int k, hipStream_t st, int probe, int item_begin, int item_end)
{
    const HostLayout& H = P->host;
    if (item_begin < 0 || item_end > panel_items(H) || item_begin > item_end) EHYB_FAIL(EHYB_ERR_ARG, "panel launch: items [%d, %d) of %d", item_begin, item_end, panel_items(H));
    int n_items = item_end - item_begin;
    if (n_items > 0) {
        // panels of up to 9,728 columns: two 512-thread workgroups per CU (one stages while the other streams); wider
        // panels leave room for one workgroup only, which then gets the CU's 16 waves
        // (on the LDS the launch really takes: k interleaved panel images)
        const bool wide = P->cfg.er_panel_threads ? P->cfg.er_panel_threads == 1024 : (int64_t)k * H.pb_panel_cols > 9728;
        const int threads = wide ? 1024 : 512;
        const bool dpp = k > 1 || P->cfg.er_sums != 2;
        int xcd = P->cfg.xcd_map != 2 ? 1 : 0;
        // cfg.er_queue: one resident round of workgroups taking items from per-XCD queues (with stealing) instead of one
        // workgroup per item; needs the XCD map's contiguous eighths, and more items than workgroups to be worth it
        const int resident = kNumCU * (wide ? 1 : 2);
        // (automatic, cfg.er_queue = 0: from six items per resident workgroup up -- a workgroup that takes neighbouring items finds the panel
        // of the previous one still staged, and the XCDs even out: R-MAT 2^24 574 -> 544 us; with three or four items per workgroup the two
        // barriers and the atomic round trip per item cost more than that: 2^22 132 -> 138 us.  profiles/r04_d_panel_two_ab.jsonl)
        const bool want_queue = P->cfg.er_queue == 1 || (P->cfg.er_queue == 0 && n_items >= 6 * resident);
        int* queue = (want_queue && xcd && n_items > resident) ? P->d_pb_queue : nullptr;
        const int grid = queue ? resident : n_items;
        // successive launches walk the entry stream in alternating directions (cfg.ell_alternate) where it does not fit the cache
        int rev = 0;
        if (!probe && (t_walk >= 0 || P->cfg.ell_alternate == 1 || (P->cfg.ell_alternate == 0 && H.pb_bytes > kInfinityCache))) {
            // one direction per MULTIPLY: a multiply in parts (ehyb_spmv_part: one pass-1 launch per column segment) turns around
            // with its first part
            if (t_walk >= 0) rev = t_walk & 1;
            else if (item_begin == 0) rev = (P->panel_parity.fetch_xor(1, std::memory_order_relaxed) ^ 1) & 1;
            else rev = P->panel_parity.load(std::memory_order_relaxed) & 1;
        }
        const int row = panel_scale_kernel(threads, k, dpp, probe != 0);
        if (row < 0) EHYB_FAIL(EHYB_ERR_ARG, "panel pass 1 not built for %d threads, %d columns%s", threads, k, probe ? " with probes" : "");
        const int2* items = (const int2*)P->d_pb_items1 + item_begin;
        const int4* units = (const int4*)P->d_pb_units1;
        int panel_cols = H.pb_panel_cols;
        void* args1[] = {&items, &units, &P->d_pb_val, &P->d_pb_colf, &P->d_pb_chunk, &P->d_pb_jump, &x, &P->d_pb_partial, &panel_cols, &probe, &xcd, &queue, &n_items, &rev};
        void* argsk[] = {&items, &units, &P->d_pb_val, &P->d_pb_colf, &P->d_pb_chunk, &P->d_pb_jump, &x, &ldx, &P->d_pb_partial, &panel_cols, &xcd, &queue, &n_items, &rev};
        P->mark_launched(EHYB_KERNELS_PANEL, (size_t)row);
        (void)hipLaunchKernel(panel_kernels()[(size_t)row].fn, dim3(grid), dim3(threads), k == 1 ? args1 : argsk, panel_scale_lds_bytes(H, k, dpp, threads), st);
    }
    HIP_TRY(hipGetLastError());  // (as <<< >>>: a failed launch is the last error)
    return EHYB_OK;
}

// first pass-2 unit whose rows lie at or behind cfg.row_split (= number of units: no split)
static int pass2_split(const ehyb_plan* P)
{
    const HostLayout& H = P->host;
    const int u2 = (int)(H.pb_units2.size() / 4);
    if (P->cfg.row_split <= 0) return u2;
    int lo = 0, hi = u2;   // units ascend by first row
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (H.pb_units2[(size_t)mid * 4 + 2] < P->cfg.row_split) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the row blocks a pass-2 launch covers: all, those in front of cfg.row_split, those from it on
enum PanelRows { PANEL_ROWS_ALL = 0, PANEL_ROWS_BEFORE_SPLIT = 1, PANEL_ROWS_FROM_SPLIT = 2 };

// Pass 2 (reduce) into k columns of y, ldy doubles apart; probe: ehyb_debug_panel_times only.
static int launch_panel_reduce(ehyb_plan* P, double* y, long long ldy, int k, hipStream_t st, int probe, PanelRows part)
{
    const HostLayout& H = P->host;
    const int cut = part != PANEL_ROWS_ALL ? pass2_split(P) : 0;
    const int first = part == PANEL_ROWS_FROM_SPLIT ? cut : 0;
    const int n_units = (part == PANEL_ROWS_BEFORE_SPLIT ? cut : (int)(H.pb_units2.size() / 4)) - first;
    if (n_units > 0) {
        // (cfg.er_nt: 0 = by the size of what pass 2 reads -- 8 B per column and 2 B of row word per partial sum -- against half the
        // Infinity Cache, 1 / 2 = always / never)
        const bool nt = P->cfg.er_nt == 1 || (P->cfg.er_nt == 0 && H.pb_partials * (8 * k + 2) > kInfinityCache / 2);
        const int row = panel_reduce_kernel(k, nt);
        if (row < 0 || (k > 1 && probe)) EHYB_FAIL(EHYB_ERR_ARG, "panel pass 2 not built for %d columns%s", k, probe ? " with probes" : "");
        const int4* units = (const int4*)P->d_pb_units2 + first;
        void* args1[] = {&units, &P->d_pb_partial, &P->d_pb_row, &y, &probe};
        void* argsk[] = {&units, &P->d_pb_partial, &P->d_pb_row, &y, &ldy};
        P->mark_launched(EHYB_KERNELS_PANEL, (size_t)row);
        (void)hipLaunchKernel(panel_kernels()[(size_t)row].fn, dim3(n_units), dim3(512), k == 1 ? args1 : argsk, panel_reduce_lds_bytes(H, k), st);
    }
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

int ehyb::launch_panel_k(ehyb_plan* P, const double* x, long long ldx, double* y, long long ldy, int k, hipStream_t st, int walk)
{
    const int width = spmm_width(P->host);
    if (k < 1 || k > width) EHYB_FAIL(EHYB_ERR_ARG, "launch_panel_k: %d columns on a plan whose panel passes serve %d", k, width);
    WalkScope w(walk);  // reaches pass 1 the way ehyb_spmv_walk's does
    const int rc = launch_panel_scale(P, x, ldx, k, st, 0, 0, panel_items(P->host));
    return rc != EHYB_OK ? rc : launch_panel_reduce(P, y, ldy, k, st, 0, PANEL_ROWS_ALL);
}

// ---- CSR residual
// Every instantiation of the row-segment kernel (256 threads): one vector and K = 2..kSpmmMaxK, adding to what the window launch
// wrote or ASSIGNing (the direct shape: it does everything), and the one-vector kernels of cfg.val_f32.
struct ErKernel { int k; bool assign, f32; const void* fn; };

template <bool ASSIGN>
static void add_er_kernels(std::vector<ErKernel>* v)
{
    v->insert(v->end(), {{1, ASSIGN, false, (const void*)ehyb_er_kernel<256, ASSIGN>}, {2, ASSIGN, false, (const void*)ehyb_er_k_kernel<256, ASSIGN, 2>},
                         {3, ASSIGN, false, (const void*)ehyb_er_k_kernel<256, ASSIGN, 3>}, {4, ASSIGN, false, (const void*)ehyb_er_k_kernel<256, ASSIGN, 4>}});
}

static const std::vector<ErKernel>& er_kernels()
{
    static const std::vector<ErKernel> all = [] {
        std::vector<ErKernel> v;
        add_er_kernels<false>(&v), add_er_kernels<true>(&v);
        v.insert(v.end(), {{1, false, true, (const void*)ehyb_er_f32_kernel<256, false>}, {1, true, true, (const void*)ehyb_er_f32_kernel<256, true>}});  // (same arguments: d_er_val holds floats)
        return v;
    }();
    return all;
}

int ehyb::launch_er_csr(ehyb_plan* P, const double* x, long long ldx, double* y, long long ldy, int k, hipStream_t st)
{
    const HostLayout& H = P->host;
    if (H.er_bins[3] == 0) return EHYB_OK;
    const int n_blocks = (int)(H.er_blocks.size() / 4);
    if (P->cfg.er_threads != 256) EHYB_FAIL(EHYB_ERR_ARG, "residual workgroup size %d not built (256)", P->cfg.er_threads);
    const bool f32 = P->cfg.val_f32 == 1;
    if (f32 && k > 1) EHYB_FAIL(EHYB_ERR_ARG, "residual launch: cfg.val_f32 serves one column, not %d", k);
    const void* launch = nullptr;
    const std::vector<ErKernel>& table = er_kernels();
    size_t row = 0;
    for (; row < table.size(); ++row) {
        const ErKernel& e = table[row];
        if (e.k == k && e.assign == (H.direct != 0) && e.f32 == f32) {  // ASSIGN: the direct shape
            launch = e.fn;
            break;
        }
    }
    if (!launch) EHYB_FAIL(EHYB_ERR_ARG, "residual launch not built for %d columns", k);
    const int4* blocks = (const int4*)P->d_er_blocks;
    void* args1[] = {&blocks, &P->d_er_seg_ptr, &P->d_er_seg_row, &P->d_er_col, &P->d_er_val, &x, &y};
    void* argsk[] = {&blocks, &P->d_er_seg_ptr, &P->d_er_seg_row, &P->d_er_col, &P->d_er_val, &x, &ldx, &y, &ldy};
    P->mark_launched(EHYB_KERNELS_ER_CSR, row);
    (void)hipLaunchKernel(launch, dim3(n_blocks), dim3(256), k == 1 ? args1 : argsk, 0, st);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

static int launch_er(ehyb_plan* P, const double* x, double* y, hipStream_t st)
{
    if (P->host.er_panel)  // panel form: scale (x panels in LDS) then reduce (y blocks in LDS)
        return launch_panel_k(P, x, 0, y, 0, 1, st, t_walk);  // (t_walk: the scope it opens changes nothing -- the caller's walk stays)
    return launch_er_csr(P, x, 0, y, 0, 1, st);
}

template <class T, class A>
static int upload(T** dst, const std::vector<T, A>& src)
{
    *dst = nullptr;
    size_t bytes = std::max<size_t>(src.size(), 1) * sizeof(T) + 4096;  // slack: clamped prefetches
    HIP_TRY(hipMalloc((void**)dst, bytes));
    if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return EHYB_OK;
}

// cfg.val_f32: a value stream converted on the host (device_values_f32) and only the floats sent; *dst keeps its type, the
// fp32 kernels reinterpret it
static int upload_f32(const ehyb_plan* P, double** dst, const double* src, size_t n)
{
    BigVec<float> f(n);
    {
        OmpScope omp(P->cfg.host_threads);
        device_values_f32(src, n, f.data());
    }
    return upload((float**)dst, f);
}

static void free_device(ehyb_plan* P)
{
    void** ptrs[] = {(void**)&P->d_halo_cols,  (void**)&P->d_ell_val,   (void**)&P->d_ell_col,    (void**)&P->d_lane_group,
                     (void**)&P->d_slab_meta,  (void**)&P->d_items,     (void**)&P->d_segs,       (void**)&P->d_er_seg_ptr,
                     (void**)&P->d_er_seg_row, (void**)&P->d_er_col,    (void**)&P->d_er_val,     (void**)&P->d_er_blocks,
                     (void**)&P->d_slab_lrow,  (void**)&P->d_pb_val,    (void**)&P->d_pb_colf,    (void**)&P->d_pb_chunk,   (void**)&P->d_pb_jump,
                     (void**)&P->d_pb_units1,  (void**)&P->d_pb_items1,  (void**)&P->d_pb_queue,   (void**)&P->d_pb_row,    (void**)&P->d_pb_units2,  (void**)&P->d_pb_partial,
                     (void**)&P->d_item_map,   (void**)&P->d_ell_src,    (void**)&P->d_ell_src2,  (void**)&P->d_er_src,     (void**)&P->d_pb_src};
    for (void** q : ptrs) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    for (int32_t* q : P->retired_item_maps) (void)hipFree(q);
    P->retired_item_maps.clear();
    P->item_map.clear();
    P->uploaded = false;
}

extern "C" {

int ehyb_device_count(int* count)
{
    if (!count) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_device_count: null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *count = 0;
        set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return EHYB_ERR_NO_DEVICE;
    }
    *count = c;
    return EHYB_OK;
}

int ehyb_device_set(int device)
{
    HIP_TRY(hipSetDevice(device));
    return EHYB_OK;
}

int ehyb_device_name(char* buf, int len)
{
    if (!buf || len <= 0) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_device_name: bad buffer");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    snprintf(buf, (size_t)len, "%s %s CUs=%d", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return EHYB_OK;
}

int ehyb_dev_alloc(size_t bytes, void** ptr)
{
    if (!ptr) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_dev_alloc: null");
    HIP_TRY(hipMalloc(ptr, std::max<size_t>(bytes, 8)));
    return EHYB_OK;
}
int ehyb_dev_free(void* ptr)
{
    if (ptr) HIP_TRY(hipFree(ptr));
    return EHYB_OK;
}
int ehyb_h2d(void* dst, const void* src, size_t bytes)
{
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return EHYB_OK;
}
int ehyb_d2h(void* dst, const void* src, size_t bytes)
{
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return EHYB_OK;
}
int ehyb_stream_create(void** stream)
{
    if (!stream) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_stream_create: null");
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void*)s;
    return EHYB_OK;
}
int ehyb_stream_destroy(void* stream)
{
    if (stream) HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return EHYB_OK;
}
int ehyb_stream_sync(void* stream)
{
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return EHYB_OK;
}
int ehyb_dev_mem_info(size_t* free_bytes, size_t* total_bytes)
{
    if (!free_bytes || !total_bytes) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_dev_mem_info: null argument");
    HIP_TRY(hipMemGetInfo(free_bytes, total_bytes));
    return EHYB_OK;
}
int ehyb_dev_sync(void)
{
    HIP_TRY(hipDeviceSynchronize());
    return EHYB_OK;
}

int ehyb_measure_read_bw(size_t bytes, int iters, double* gbps)
{
    if (!gbps || iters < 1 || bytes < 4096) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_measure_read_bw: bad arguments");
    double2* buf = nullptr;
    double* sink = nullptr;
    size_t n2 = bytes / sizeof(double2);
    HIP_TRY(hipMalloc((void**)&buf, n2 * sizeof(double2)));
    HIP_TRY(hipMalloc((void**)&sink, 8));
    HIP_TRY(hipMemset(buf, 0x11, n2 * sizeof(double2)));
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(ehyb_read_kernel, dim3(4096), dim3(256), 0, 0, buf, n2, sink);
    HIP_TRY(hipEventRecord(a, 0));
    for (int i = 0; i < iters; ++i) hipLaunchKernelGGL(ehyb_read_kernel, dim3(4096), dim3(256), 0, 0, buf, n2, sink);
    HIP_TRY(hipEventRecord(b, 0));
    HIP_TRY(hipEventSynchronize(b));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    *gbps = (double)n2 * sizeof(double2) * iters / (ms * 1e-3) / 1e9;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    (void)hipFree(buf);
    (void)hipFree(sink);
    return EHYB_OK;
}

// Diagnostic (tools/stamps.py): one launch of the stamped instantiation of the ELL kernel.
// out[4*i + {0,1,2,3}] = entry / staged / exit wall-clock ticks (100 MHz) and XCC id of item i.
int ehyb_debug_ell_stamps(ehyb_plan* P, const double* x, double* y, unsigned long long* out_host);
int ehyb_debug_ell_stamps_probe(ehyb_plan* P, const double* x, double* y, unsigned long long* out_host, int triple_gather)
{
    t_probe_n = (triple_gather == 2) ? -1 : (triple_gather && P) ? P->host.n_cols : 0;   // 2: no halo gather (diagnostic)
    const int rc = ehyb_debug_ell_stamps(P, x, y, out_host);
    t_probe_n = 0;
    return rc;
}

int ehyb_debug_ell_stamps(ehyb_plan* P, const double* x, double* y, unsigned long long* out_host)
{
    if (!P || !P->uploaded || !out_host) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_ell_stamps: bad arguments");
    if (P->cfg.val_f32 == 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_ell_stamps: no stamped kernel is built for cfg.val_f32");
    const int n_items = (int)(P->host.items.size() / kItemWords);
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, (size_t)n_items * 32));
    HIP_TRY(hipMemset(d, 0, (size_t)n_items * 32));
    int rc = launch_window(P, x, 0, y, 0, 1, nullptr, P->host.inline_er, -1, d);
    if (rc == EHYB_OK && hipDeviceSynchronize() != hipSuccess) rc = EHYB_ERR_HIP;
    if (rc == EHYB_OK && hipMemcpy(out_host, d, (size_t)n_items * 32, hipMemcpyDeviceToHost) != hipSuccess) rc = EHYB_ERR_HIP;
    if (rc == EHYB_ERR_HIP) set_error("ehyb_debug_ell_stamps: %s", hipGetErrorString(hipGetLastError()));
    (void)hipFree(d);
    return rc;
}

int ehyb_halo_step(ehyb_plan* P, const double* x, double* y, const int32_t* send_idx, double* send_buf, int64_t n_send, int n_chunks,
                   ehyb_exchange_fn exchange, void* user, void* compute_stream, void* comm_stream)
{
    if (!P || !exchange || n_chunks < 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_halo_step: bad arguments");
    int n_segs = 1;
    (void)ehyb_plan_col_segs(P, &n_segs);
    if (n_segs != n_chunks + 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_halo_step: the plan has %d column segments, %d chunks need %d", n_segs, n_chunks, n_chunks + 1);
    int rc = ehyb_step_pack(x, send_idx, send_buf, n_send, compute_stream, comm_stream);
    if (rc == EHYB_OK) rc = ehyb_step_part(P, x, y, compute_stream, comm_stream, 0, 0, 1, EHYB_PART_FIRST);
    for (int k = 0; k < n_chunks && rc == EHYB_OK; ++k) {
        if (exchange(k, comm_stream, user) != 0) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_halo_step: the caller's exchange of chunk %d failed", k);
        rc = ehyb_step_part(P, x, y, compute_stream, comm_stream, 1, 1 + k, 2 + k, k == n_chunks - 1 ? EHYB_PART_LAST : 0);
    }
    return rc;
}

// ---- the item -> workgroup map (ehyb_plan_tune; ehyb_debug_item_map, _set_item_map, _tune_decide: see ehyb.h)
// The item workgroup b takes under the map in force: the installed map, else the built-in order -- item b for symmetric pairs or
// cfg.xcd_map = 2, else xcd_item(b, n_items) of ell_device.h (restated here for the host).
static std::vector<int32_t> item_map_now(const ehyb_plan* P)
{
    const int n_items = (int)(P->host.items.size() / kItemWords);
    if (!P->item_map.empty()) return P->item_map;
    std::vector<int32_t> map_now((size_t)n_items);
    const bool in_order = P->host.sym || P->cfg.xcd_map == 2;
    for (int b = 0; b < n_items; ++b) {
        const int k = b & 7, j = b >> 3, chunk = n_items >> 3, rem = n_items & 7;
        map_now[(size_t)b] = in_order ? b : k * chunk + std::min(k, rem) + j;
    }
    return map_now;
}

// The decision of ehyb_plan_tune, a pure host function: from the cost of every item, and the XCD (0..15) and duration of every
// workgroup of a launch under map_now, the map that puts the heaviest items on the XCD that streamed fastest, and so on down.
// -> false (map_new untouched) where a workgroup has no stable placement (xcc < 0).
static bool tune_decide(int n_items, const double* cost, const int* xcc, const double* dur, const int32_t* map_now, std::vector<int32_t>* map_new)
{
    for (int b = 0; b < n_items; ++b)
        if (xcc[b] < 0) return false;
    // how fast each XCD streamed what it was given: median over its workgroups of bytes per microsecond
    std::vector<std::vector<double>> rates(16);
    std::vector<std::vector<int>> slots(16);
    for (int b = 0; b < n_items; ++b) {
        rates[(size_t)xcc[b]].push_back(cost[map_now[b]] / std::max(dur[b], 1e-3));
        slots[(size_t)xcc[b]].push_back(b);
    }
    std::vector<std::pair<double, int>> order;  // (median rate, xcd), fastest first
    for (int k = 0; k < 16; ++k)
        if (!rates[(size_t)k].empty()) {
            std::nth_element(rates[(size_t)k].begin(), rates[(size_t)k].begin() + rates[(size_t)k].size() / 2, rates[(size_t)k].end());
            order.push_back({-rates[(size_t)k][rates[(size_t)k].size() / 2], k});
        }
    std::sort(order.begin(), order.end());
    std::vector<int> by_cost((size_t)n_items);
    for (int i = 0; i < n_items; ++i) by_cost[(size_t)i] = i;
    std::stable_sort(by_cost.begin(), by_cost.end(), [&](int a, int b2) { return cost[a] > cost[b2]; });
    // the heaviest items on the fastest XCD, and so on down: the pairing that minimises the largest cost / rate
    map_new->assign((size_t)n_items, -1);
    size_t at = 0;
    for (const auto& o : order)
        for (int b : slots[(size_t)o.second]) (*map_new)[(size_t)b] = by_cost[at++];
    return true;
}

// The install: `map` (empty: none, the built-in order) copied to the device and made the plan's map.  The device map it replaces
// is handed back: whoever keeps the new one retires it (item_map_retire), the tuner's roll-back puts it back.
static int item_map_install(ehyb_plan* P, const std::vector<int32_t>& map, int32_t** old_dev)
{
    int32_t* dm = nullptr;
    if (!map.empty() && (hipMalloc((void**)&dm, map.size() * 4) != hipSuccess || hipMemcpy(dm, map.data(), map.size() * 4, hipMemcpyHostToDevice) != hipSuccess)) {
        if (dm) (void)hipFree(dm);
        (void)hipGetLastError();
        return EHYB_ERR_HIP;
    }
    *old_dev = P->d_item_map;
    P->d_item_map = dm;
    P->item_map = map;
    return EHYB_OK;
}

static void item_map_retire(ehyb_plan* P, int32_t* old_dev)
{
    if (old_dev) P->retired_item_maps.push_back(old_dev);  // a hipGraph captured earlier may still name it: freed with the plan
}

// Tuning of the item -> workgroup map on the device the plan lives on (see ehyb.h).
int ehyb_plan_tune(ehyb_plan* P, const double* x, double* y, int reps, double* span_before_us, double* span_after_us)
{
    clear_error();
    if (!P || !P->uploaded || !x || !y) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_tune: bad arguments");
    if (P->cfg.val_f32 == 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_tune: the tuning measures stamped launches, which cfg.val_f32 has none of");
    if (span_before_us) *span_before_us = 0;
    if (span_after_us) *span_after_us = 0;
    const HostLayout& H = P->host;
    const int n_items = (int)(H.items.size() / kItemWords);
    const int resident = kNumCU * std::max(1, P->cfg.items_per_cu);
    // one resident round only: with more items than slots the later ones start wherever a CU falls free
    if (H.direct || n_items < 16 || n_items > resident || (H.pb_assign && H.segs.empty())) return EHYB_OK;
    reps = std::min(std::max(reps, 1), 16);
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, (size_t)n_items * 32));
    std::vector<unsigned long long> st((size_t)n_items * 4);
    // cost of an item: the bytes its slabs stream (values 16 B per lane and pair + column words) + its windows
    std::vector<double> cost((size_t)n_items, 0.0);
    for (int i = 0; i < n_items; ++i) {
        const int32_t* rec = &H.items[(size_t)i * kItemWords];
        double c = 0;
        for (int s = rec[ITEM_SLAB_BEGIN]; s < rec[ITEM_SLAB_END]; ++s) {
            const SlabShape shape = unpack_slab_shape(H.slab_meta[(size_t)s * kSlabWords + SLAB_SHAPE]);
            c += (double)shape.pairs * (1024.0 + 4.0 * shape.groups);
        }
        for (int g = rec[ITEM_SEG_BEGIN]; g < rec[ITEM_SEG_END]; ++g) {
            const int32_t* seg = &H.segs[(size_t)g * kSegWords];
            c += 8.0 * (seg[SEG_WIN_LEN] + seg[SEG_HALO_COUNT]) + 16.0 * (seg[SEG_ROW_END] - seg[SEG_ROW_BEGIN]);
        }
        cost[(size_t)i] = c + 1.0;
    }
    auto measure = [&](std::vector<double>* dur, std::vector<int>* xcc, double* span_us) -> int {
        // item taken by block b under the CURRENT map
        dur->assign((size_t)n_items, 0.0);
        xcc->assign((size_t)n_items, -1);
        double span = 0;
        for (int r = 0; r < reps + 1; ++r) {  // the first launch warms the caches and is not counted
            if (hipMemset(d, 0, (size_t)n_items * 32) != hipSuccess) return EHYB_ERR_HIP;
            const int rc = launch_window(P, x, 0, y, 0, 1, nullptr, H.inline_er, -1, d);
            if (rc != EHYB_OK) return rc;
            if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(st.data(), d, (size_t)n_items * 32, hipMemcpyDeviceToHost) != hipSuccess) return EHYB_ERR_HIP;
            if (r == 0) continue;
            unsigned long long t0 = ~0ull, t1 = 0;
            for (int b = 0; b < n_items; ++b) {
                (*dur)[(size_t)b] += (double)(st[(size_t)b * 4 + 2] - st[(size_t)b * 4 + 0]) / (100.0 * reps);  // 100 MHz clock -> us
                const int k = (int)st[(size_t)b * 4 + 3] & 15;
                if ((*xcc)[(size_t)b] >= 0 && (*xcc)[(size_t)b] != k) (*xcc)[(size_t)b] = -2;  // not a stable placement
                else if ((*xcc)[(size_t)b] != -2) (*xcc)[(size_t)b] = k;
                t0 = std::min(t0, st[(size_t)b * 4 + 0]);
                t1 = std::max(t1, st[(size_t)b * 4 + 2]);
            }
            span += (double)(t1 - t0) / (100.0 * reps);
        }
        *span_us = span;
        return EHYB_OK;
    };
    std::vector<double> dur;
    std::vector<int> xcc;
    double span0 = 0, span1 = 0;
    int rc = measure(&dur, &xcc, &span0);
    const std::vector<int32_t> map_now = item_map_now(P);
    std::vector<int32_t> map_new;
    const bool stable = rc == EHYB_OK && tune_decide(n_items, cost.data(), xcc.data(), dur.data(), map_now.data(), &map_new);
    if (stable) {
        int32_t* old = nullptr;
        const std::vector<int32_t> old_host = P->item_map;
        if (item_map_install(P, map_new, &old) == EHYB_OK) {
            std::vector<double> dur2;
            std::vector<int> xcc2;
            rc = measure(&dur2, &xcc2, &span1);
            if (rc != EHYB_OK || span1 >= span0) {  // no gain on this device: the map the plan had stays
                (void)hipFree(P->d_item_map);
                P->d_item_map = old;
                P->item_map = old_host;
                span1 = span0;
            } else {
                item_map_retire(P, old);
            }
        }
    }
    (void)hipFree(d);
    if (span_before_us) *span_before_us = span0;
    if (span_after_us) *span_after_us = stable ? span1 : span0;
    return rc;
}

// Diagnostics (tests/test_item_map_host.py, tests/test_gpu_item_map.py): the map in force read back, a map set by the caller,
// and the tuner's decision on the caller's numbers (see ehyb.h).
int ehyb_debug_item_map(const ehyb_plan* P, int32_t* out, int cap, int* n_items, int* installed)
{
    clear_error();
    if (!P || !n_items || !installed || cap < 0 || (cap > 0 && !out)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_item_map: bad arguments");
    const std::vector<int32_t> map_now = item_map_now(P);
    *n_items = (int)map_now.size();
    *installed = P->item_map.empty() ? 0 : 1;
    std::copy(map_now.begin(), map_now.begin() + std::min((size_t)cap, map_now.size()), out);
    return EHYB_OK;
}

int ehyb_debug_set_item_map(ehyb_plan* P, const int32_t* map, int n, int strict)
{
    clear_error();
    if (!P || n < 0 || (n > 0 && !map) || (n == 0 && map)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_set_item_map: bad arguments");
    const HostLayout& H = P->host;
    const int n_items = (int)(H.items.size() / kItemWords);
    if (H.direct || n_items == 0 || (H.pb_assign && H.segs.empty())) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_set_item_map: the plan has no window launch that takes items");
    if (map && n != n_items) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_set_item_map: %d entries for a plan of %d items", n, n_items);
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int b = 0; b < n; ++b) {
        if (map[b] < 0 || map[b] >= n_items) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_set_item_map: entry %d is %d, the plan has items 0..%d", b, map[b], n_items - 1);
        if (strict && seen[(size_t)map[b]]++) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_set_item_map: item %d is named twice (strict: a permutation)", map[b]);
    }
    if (!P->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_debug_set_item_map: the plan is not uploaded");
    HIP_TRY(hipDeviceSynchronize());  // (no launch of this plan is under way while its map changes hands)
    int32_t* old = nullptr;
    if (item_map_install(P, std::vector<int32_t>(map, map + n), &old) != EHYB_OK) EHYB_FAIL(EHYB_ERR_HIP, "ehyb_debug_set_item_map: no device memory for %d entries", n);
    item_map_retire(P, old);
    HIP_TRY(hipDeviceSynchronize());
    return EHYB_OK;
}

int ehyb_debug_tune_decide(int n_items, const double* cost, const int* xcc, const double* dur, const int32_t* map_now, int32_t* map_new, int* stable)
{
    clear_error();
    if (n_items < 1 || !cost || !xcc || !dur || !map_now || !map_new || !stable) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_tune_decide: bad arguments");
    for (int b = 0; b < n_items; ++b)
        if (xcc[b] > 15 || map_now[b] < 0 || map_now[b] >= n_items)
            EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_tune_decide: workgroup %d on XCD %d with item %d (XCDs up to 15, items 0..%d)", b, xcc[b], map_now[b], n_items - 1);
    std::vector<int32_t> out;
    *stable = tune_decide(n_items, cost, xcc, dur, map_now, &out) ? 1 : 0;
    if (*stable) std::copy(out.begin(), out.end(), map_new);
    return EHYB_OK;
}

// Diagnostic (tools/panel_sweep.py): mean time of each pass of the panel residual alone, `iters` launches each
// between HIP events on the null stream; probe switches single steps of the kernels off (results wrong then).
int ehyb_debug_panel_times(ehyb_plan* P, const double* x, double* y, int iters, int probe, double* ms_scale, double* ms_reduce)
{
    if (!P || !P->uploaded || !P->host.er_panel || iters < 1 || !ms_scale || !ms_reduce) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_panel_times: bad arguments");
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    double* out[2] = {ms_scale, ms_reduce};
    int rc = EHYB_OK;
    const auto launch = [&](int pass) { return pass == 1 ? launch_panel_scale(P, x, 0, 1, nullptr, probe, 0, panel_items(P->host)) : launch_panel_reduce(P, y, 0, 1, nullptr, probe, PANEL_ROWS_ALL); };
    for (int which = 1; which <= 2 && rc == EHYB_OK; ++which) {
        for (int i = 0; i < 3 && rc == EHYB_OK; ++i) rc = launch(which);
        (void)hipEventRecord(a, nullptr);
        for (int i = 0; i < iters && rc == EHYB_OK; ++i) rc = launch(which);
        (void)hipEventRecord(b, nullptr);
        (void)hipEventSynchronize(b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, a, b);
        *out[which - 1] = ms / iters;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return rc;
}

// Diagnostic (tests/kernel_census_cases.py): the three kernel tables as rows of ints, and a plan's launch log (see ehyb.h).
int ehyb_debug_kernel_table(int which, int32_t* rows, int cap, int* n_rows)
{
    clear_error();
    if (!n_rows || cap < 0 || (cap > 0 && !rows)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_kernel_table: bad arguments");
    std::vector<int32_t> out;
    if (which == EHYB_KERNELS_WINDOW) {
        for (const EllKernel& e : ell_kernels()) out.insert(out.end(), {e.threads, e.k, e.dyn, e.stamp, e.inl, e.sym, e.f32});
    } else if (which == EHYB_KERNELS_PANEL) {
        for (const PanelKernel& e : panel_kernels()) out.insert(out.end(), {e.pass, e.threads, e.k, e.dpp, e.probe, e.nt});
    } else if (which == EHYB_KERNELS_ER_CSR) {
        for (const ErKernel& e : er_kernels()) out.insert(out.end(), {e.k, e.assign, e.f32});
    } else {
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_kernel_table: table %d (EHYB_KERNELS_WINDOW, _PANEL, _ER_CSR)", which);
    }
    const int width = which == EHYB_KERNELS_WINDOW ? EHYB_KERNEL_ROW_WINDOW : (which == EHYB_KERNELS_PANEL ? EHYB_KERNEL_ROW_PANEL : EHYB_KERNEL_ROW_ER_CSR);
    const int n = (int)(out.size() / (size_t)width);
    if (n > kKernelTableCap) EHYB_FAIL(EHYB_ERR_INTERNAL, "ehyb_debug_kernel_table: table %d has %d rows, the launch log of a plan %d", which, n, kKernelTableCap);
    *n_rows = n;
    std::copy(out.begin(), out.begin() + (size_t)std::min(n, cap) * (size_t)width, rows);
    return EHYB_OK;
}

static int kernel_table_rows(int which)
{
    return which == EHYB_KERNELS_WINDOW ? (int)ell_kernels().size() : which == EHYB_KERNELS_PANEL ? (int)panel_kernels().size() : which == EHYB_KERNELS_ER_CSR ? (int)er_kernels().size() : -1;
}

int ehyb_debug_launched(const ehyb_plan* P, int which, uint8_t* out, int cap)
{
    clear_error();
    const int n = kernel_table_rows(which);
    if (!P || !out || n < 0 || cap < n || n > kKernelTableCap) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_launched: bad arguments (table %d has %d rows, room for %d)", which, n, cap);
    for (int i = 0; i < n; ++i) out[i] = __atomic_load_n(&P->launched[which][i], __ATOMIC_RELAXED);
    return EHYB_OK;
}

int ehyb_debug_launched_clear(ehyb_plan* P)
{
    clear_error();
    if (!P) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_debug_launched_clear: null plan");
    for (int t = 0; t < kKernelTables; ++t)
        for (int i = 0; i < kKernelTableCap; ++i) __atomic_store_n(&P->launched[t][i], (uint8_t)0, __ATOMIC_RELAXED);
    for (int i = 0; i < kKernelTableTCap; ++i) __atomic_store_n(&P->launched_t[i], (uint8_t)0, __ATOMIC_RELAXED);
    return EHYB_OK;
}

int ehyb_plan_upload(ehyb_plan* P)
{
    clear_error();
    if (!P) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_upload: null plan");
    if (P->uploaded) return EHYB_OK;
    // (before the device is looked for: a property of the plan)
    if (P->cfg.val_f32 == 1 && (P->host.er_panel || P->host.deferred.pending))
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_upload: cfg.val_f32 is not built for a residual in panel form (the panel passes read fp64 values)");
    if (P->cfg.val_f32 == 1 && P->cfg.ell_variant == 3)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_upload: cfg.val_f32 has no round-robin kernel (cfg.ell_variant = 3)");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
        EHYB_FAIL(EHYB_ERR_NO_DEVICE, "ehyb_plan_upload: no HIP device visible (the EHYB multiply has no CPU fallback)");
    HIP_TRY(hipGetDevice(&P->device));
    const HostLayout& H = P->host;
    if (H.deferred.pending) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_plan_upload: the plan's panel form was left to the device and never built");
    int rc;
#define UP(dst, src)                           \
    if ((rc = upload(&P->dst, H.src)) != EHYB_OK) { \
        free_device(P);                        \
        return rc;                             \
    }
    UP(d_halo_cols, halo_cols)
    const bool f32 = P->cfg.val_f32 == 1;
    if (f32) {
        if ((rc = upload_f32(P, &P->d_ell_val, H.ell_val.data(), H.ell_val.size())) != EHYB_OK) {
            free_device(P);
            return rc;
        }
    } else {
        UP(d_ell_val, ell_val)
    }
    if (P->cfg.ell_triples == 1) {
        // the device's own form of the column words and slab records (col_triples.h); the host arrays stay the definition
        BigVec<uint32_t> words;
        std::vector<uint32_t> meta;
        {
            OmpScope omp(P->cfg.host_threads);
            P->d_triples = device_cols(H, true, &words, &meta) != (int64_t)H.ell_col.size() || meta != H.slab_meta;
        }
        if ((rc = upload(&P->d_ell_col, words)) != EHYB_OK || (rc = upload(&P->d_slab_meta, meta)) != EHYB_OK) {
            free_device(P);
            return rc;
        }
    } else {
        UP(d_ell_col, ell_col)
        UP(d_slab_meta, slab_meta)
    }
    UP(d_lane_group, lane_group)
    UP(d_items, items)
    UP(d_segs, segs)
    UP(d_slab_lrow, slab_lrow)
    if (H.er_panel) {
        // the residual launch runs the panel form: the CSR segments stay on the host
        if (!H.pb_host_missing) {  // (else: built where they are, er_panel_dev.hip)
            UP(d_pb_val, pb_val)
            UP(d_pb_colf, pb_colf)
            UP(d_pb_chunk, pb_chunk)
            UP(d_pb_jump, pb_jump)
            UP(d_pb_row, pb_row)
        }
        UP(d_pb_units1, pb_units1)
        UP(d_pb_items1, pb_items1)
        UP(d_pb_units2, pb_units2)
        if (hipMalloc((void**)&P->d_pb_queue, 256 * sizeof(int)) != hipSuccess || hipMemset(P->d_pb_queue, 0, 256 * sizeof(int)) != hipSuccess) {
            free_device(P);
            EHYB_FAIL(EHYB_ERR_HIP, "ehyb_plan_upload: no device memory for the work queues");
        }
        // (one slot per partial sum and column of the widest pass)
        if (hipMalloc((void**)&P->d_pb_partial, (size_t)std::max<int64_t>(H.pb_partials, 1) * spmm_width(H) * 8) != hipSuccess) {
            free_device(P);
            EHYB_FAIL(EHYB_ERR_HIP, "ehyb_plan_upload: no device memory for %lld partial sums", (long long)H.pb_partials);
        }
    } else {
        UP(d_er_seg_ptr, er_seg_ptr)
        UP(d_er_seg_row, er_seg_row)
        UP(d_er_col, er_col)
        if (f32) {
            if ((rc = upload_f32(P, &P->d_er_val, H.er_val.data(), H.er_val.size())) != EHYB_OK) {
                free_device(P);
                return rc;
            }
        } else {
            UP(d_er_val, er_val)
        }
        UP(d_er_blocks, er_blocks)
    }
#undef UP
    // opt in to the full 160 KiB of LDS (the role of cudaFuncSetAttribute at kernel.cu:351,411).  The
    // attribute belongs to the kernel, not to a plan: it is set to the device maximum, so plans with
    // windows of different sizes can live side by side in one process.
    const int lds = EHYB_LDS_MAX_DOUBLES * 8;
    for (const EllKernel& e : ell_kernels())
        if (!e.stamp) HIP_TRY(hipFuncSetAttribute(e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));  // (a stamped launch opts in itself)
    for (const PanelKernel& e : panel_kernels()) HIP_TRY(hipFuncSetAttribute(e.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    if ((rc = spmv_t_opt_in_lds()) != EHYB_OK) return rc;
    P->uploaded = true;
    return EHYB_OK;
}

void ehyb_plan_destroy(ehyb_plan* P)
{
    if (!P) return;
    free_device(P);
    delete P;
}

int ehyb_spmv_phase(ehyb_plan* P, const double* x, double* y, void* stream, int phase)
{
    if (!P || !x || !y) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv: null argument");
    if (!P->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_spmv: plan not uploaded (no CPU fallback exists)");
    hipStream_t st = (hipStream_t)stream;
    int rc = EHYB_OK;
    if (phase == 0 && P->host.inline_er) return launch_ell(P, x, y, st, true);  // one launch
    if (P->host.direct && phase != 0) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_spmv_phase: a plan in the direct shape (small matrix) has no phases");
    if (phase == 0 || phase == 1) rc = launch_ell(P, x, y, st, false);
    if (rc == EHYB_OK && (phase == 0 || phase == 2)) rc = launch_er(P, x, y, st);
    return rc;
}

int ehyb_spmv(ehyb_plan* P, const double* x, double* y, void* stream)
{
    return ehyb_spmv_phase(P, x, y, stream, 0);
}

int ehyb_spmv_walk(ehyb_plan* P, const double* x, double* y, void* stream, int walk)
{
    if (walk < -1 || walk > 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_walk: walk %d (EHYB_WALK_AUTO, _FIRST_TO_LAST, _LAST_TO_FIRST)", walk);
    WalkScope w(walk);
    return ehyb_spmv_phase(P, x, y, stream, 0);
}

// ---- the pinned share of the value stream, for tools and tests (host arithmetic; no device needed)
int ehyb_ell_slab_resident(int pos, int n, int keep1024, int shape) { return ell_slab_resident(pos, n, keep1024, shape) ? 1 : 0; }

int ehyb_ell_auto_keep1024(int64_t value_bytes, int64_t plain_bytes) { return ell_auto_keep1024(value_bytes, plain_bytes); }

int64_t ehyb_plan_resident_bytes(const ehyb_plan* P)
{
    if (!P) {
        set_error("ehyb_plan_resident_bytes: null argument");
        return -1;
    }
    const HostLayout& H = P->host;
    int keep1024 = 0, shape = 0;
    ell_keep_rule(P, ell_alternates(P), &keep1024, &shape);
    int64_t bytes = 0;
    for (size_t sg = 0; sg < H.segs.size(); sg += kSegWords) {
        const int sb = H.segs[sg + SEG_SLAB_BEGIN], se = H.segs[sg + SEG_SLAB_END];
        for (int s = sb; s < se; ++s)   // (WALK_END: the walk first to last)
            if (ell_slab_resident(s - sb, se - sb, keep1024, shape))
                bytes += (int64_t)unpack_slab_shape(H.slab_meta[(size_t)s * kSlabWords + SLAB_SHAPE]).pairs * kSlabRows * (P->cfg.val_f32 == 1 ? 8 : 16);
    }
    return bytes;
}

// ---- a captured multiply (or run of multiplies) that keeps the alternation: see ehyb.h
struct ehyb_graph {
    hipGraphExec_t exec[2] = {nullptr, nullptr};   // [d]: the run starting with direction d; equal runs (even count, or a plan that does not alternate) share exec[0]
    int next = 0;
    bool two = false;
};

int ehyb_spmv_graph_create(ehyb_plan* P, const double* x, double* y, int multiplies, ehyb_graph** out)
{
    clear_error();
    if (!P || !x || !y || !out || multiplies < 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_graph_create: bad arguments");
    *out = nullptr;
    if (!P->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_spmv_graph_create: plan not uploaded");
    hipStream_t own = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
    ehyb_graph* G = new ehyb_graph;
    // a window-only plan with a pinned set reads the same slabs from the cache in either direction: every captured multiply walks first
    // to last and one executable serves (a panel residual's first pass still alternates: such plans are captured as before)
    const bool one_way = (P->cfg.ell_nt == 4 || P->cfg.ell_nt == 5) && !ell_alternates(P) && !P->host.er_panel;
    G->two = !one_way && (multiplies & 1) != 0;   // an odd run ends on the direction it began with: the next launch must begin with the other
    int rc = EHYB_OK;
    for (int d = 0; d < (G->two ? 2 : 1) && rc == EHYB_OK; ++d) {
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(own, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            rc = EHYB_ERR_HIP;
            break;
        }
        for (int i = 0; i < multiplies && rc == EHYB_OK; ++i) rc = ehyb_spmv_walk(P, x, y, (void*)own, one_way ? 0 : (d + i) & 1);
        const hipError_t e = hipStreamEndCapture(own, &g);
        if (rc == EHYB_OK && (e != hipSuccess || hipGraphInstantiate(&G->exec[d], g, nullptr, nullptr, 0) != hipSuccess)) rc = EHYB_ERR_HIP;
        if (g) (void)hipGraphDestroy(g);
    }
    (void)hipStreamDestroy(own);
    if (rc != EHYB_OK) {
        if (rc == EHYB_ERR_HIP) set_error("ehyb_spmv_graph_create: capture failed: %s", hipGetErrorString(hipGetLastError()));
        ehyb_graph_destroy(G);
        return rc;
    }
    *out = G;
    return EHYB_OK;
}

int ehyb_graph_launch(ehyb_graph* G, void* stream)
{
    if (!G || !G->exec[0]) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_graph_launch: null");
    HIP_TRY(hipGraphLaunch(G->exec[G->two ? G->next : 0], (hipStream_t)stream));
    if (G->two) G->next ^= 1;
    return EHYB_OK;
}

void ehyb_graph_destroy(ehyb_graph* G)
{
    if (!G) return;
    for (auto e : G->exec)
        if (e) (void)hipGraphExecDestroy(e);
    delete G;
}

int ehyb_plan_col_segs(const ehyb_plan* P, int* n_col_segs)
{
    if (!P || !n_col_segs) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_col_segs: null argument");
    *n_col_segs = P->host.col_seg_first.size() >= 2 ? (int)P->host.col_seg_first.size() - 1 : 1;
    return EHYB_OK;
}

// The multiply in parts (multi-GPU: x arrives column segment by column segment).
int ehyb_spmv_part(ehyb_plan* P, const double* x, double* y, void* stream, int seg_begin, int seg_end, int flags)
{
    if (!P || !x || !y) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_part: null argument");
    if (!P->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_spmv_part: plan not uploaded (no CPU fallback exists)");
    const HostLayout& H = P->host;
    int n_segs = 1;
    (void)ehyb_plan_col_segs(P, &n_segs);
    if (seg_begin < 0 || seg_end > n_segs || seg_begin > seg_end) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_part: column segments [%d, %d) of %d", seg_begin, seg_end, n_segs);
    if (H.direct || H.inline_er) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_spmv_part: this plan multiplies in one launch (direct shape or inline residual): it has no parts");
    // (every refusal in front of the first launch: a refused call enqueues nothing)
    const bool split = P->cfg.row_split > 0;
    if ((flags & EHYB_PART_LAST_FOREIGN) && !split) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_spmv_part: EHYB_PART_LAST_FOREIGN needs a plan built with cfg.row_split");
    hipStream_t st = (hipStream_t)stream;
    int rc = EHYB_OK;
    if (flags & EHYB_PART_FIRST) rc = launch_ell(P, x, y, st, false);
    if (rc != EHYB_OK || (H.er_bins[3] == 0 && !H.er_panel)) return rc;
    if (!H.er_panel) return (flags & EHYB_PART_LAST) ? launch_er(P, x, y, st) : EHYB_OK;  // CSR residual: one launch, needs all of x
    if (seg_end > seg_begin) {
        const int ib = H.pb_seg_item.empty() ? 0 : H.pb_seg_item[(size_t)seg_begin];
        const int ie = H.pb_seg_item.empty() ? panel_items(H) : H.pb_seg_item[(size_t)seg_end];
        rc = launch_panel_scale(P, x, 0, 1, st, 0, ib, ie);
    }
    // the closing pass: all row blocks, or -- with cfg.row_split -- the foreign rows first (EHYB_PART_LAST_FOREIGN, as soon as
    // segment 0's pass 1 is enqueued) and the rows in front of the split at the end
    if (rc == EHYB_OK && (flags & EHYB_PART_LAST_FOREIGN)) rc = launch_panel_reduce(P, y, 0, 1, st, 0, PANEL_ROWS_FROM_SPLIT);
    if (rc == EHYB_OK && (flags & EHYB_PART_LAST)) rc = launch_panel_reduce(P, y, 0, 1, st, 0, split ? PANEL_ROWS_BEFORE_SPLIT : PANEL_ROWS_ALL);
    return rc;
}

int ehyb_gather(const double* src, const int32_t* idx, double* dst, int64_t n, void* stream)
{
    if (n < 0 || (n > 0 && (!src || !idx || !dst))) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_gather: bad arguments");
    if (n == 0) return EHYB_OK;
    hipLaunchKernelGGL(ehyb_gather_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, src, idx, dst, (long long)n);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

int ehyb_scatter_add(double* y, const int32_t* idx, const double* src, int64_t n, void* stream)
{
    if (n < 0 || (n > 0 && (!y || !idx || !src))) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_scatter_add: bad arguments");
    if (n == 0) return EHYB_OK;
    hipLaunchKernelGGL(ehyb_scatter_add_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, y, idx, src, (long long)n);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

// "`waiter` waits for everything enqueued on `on` so far": an event record + a stream wait.  The events are a small
// per-thread, per-DEVICE ring, made once and reused (recording an event again while an earlier wait on it is pending is
// well defined: a wait refers to the record that preceded it); a thread that drives plans on several devices gets one ring
// for each, and the rings are destroyed when the thread ends.
namespace {
struct EventRings {
    static constexpr int kRing = 16, kDevices = 16;
    hipEvent_t ring[kDevices][kRing] = {};
    int next[kDevices] = {};
    ~EventRings()
    {
        for (auto& dev : ring)
            for (hipEvent_t e : dev)
                if (e) (void)hipEventDestroy(e);
    }
};
}  // namespace
static int stream_wait_stream(hipStream_t waiter, hipStream_t on)
{
    static thread_local EventRings R;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= EventRings::kDevices) EHYB_FAIL(EHYB_ERR_ARG, "stream_wait_stream: device %d", dev);
    hipEvent_t& e = R.ring[dev][R.next[dev]];
    R.next[dev] = (R.next[dev] + 1) % EventRings::kRing;
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(e, on));
    HIP_TRY(hipStreamWaitEvent(waiter, e, 0));
    return EHYB_OK;
}

int ehyb_step_pack(const double* x, const int32_t* idx, double* send_buf, int64_t n, void* compute_stream, void* comm_stream)
{
    int rc = ehyb_gather(x, idx, send_buf, n, compute_stream);
    if (rc == EHYB_OK && comm_stream != compute_stream) rc = stream_wait_stream((hipStream_t)comm_stream, (hipStream_t)compute_stream);
    return rc;
}

int ehyb_step_part(ehyb_plan* P, const double* x, double* y, void* compute_stream, void* comm_stream, int wait_comm, int seg_begin, int seg_end,
                   int flags)
{
    if (wait_comm && comm_stream != compute_stream) {
        const int rc = stream_wait_stream((hipStream_t)compute_stream, (hipStream_t)comm_stream);
        if (rc != EHYB_OK) return rc;
    }
    return ehyb_spmv_part(P, x, y, compute_stream, seg_begin, seg_end, flags);
}

int ehyb_spmv_bench(ehyb_plan* P, const double* x, double* y, void* stream, int warmup, int iters,
                    double* ms_total, double* ms_ell, double* ms_er)
{
    if (!P || iters < 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_bench: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    // The loop of the reference (spmv.cu:108-116): MAXIter multiplies of the same x, back to back.
    // It is replayed from a hipGraph of kBatch multiplies (the legacy default stream cannot be
    // captured: a private blocking stream stands in for it), and the host never runs more than
    // 2 x kThrottle multiplies ahead of the device: with 15 us kernels an unthrottled loop of a few
    // hundred launches outran the device far enough to hit a one-off ~80 ms stall inside the
    // runtime, which a 500-iteration measurement reported as 183 us per multiply instead of 15.
    constexpr int kBatch = 32, kThrottle = 256;
    struct Loop {
        hipStream_t own = nullptr;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        hipEvent_t a = nullptr, b = nullptr, t[2] = {nullptr, nullptr};
        ~Loop()
        {
            if (exec) (void)hipGraphExecDestroy(exec);
            if (graph) (void)hipGraphDestroy(graph);
            for (hipEvent_t e : {a, b, t[0], t[1]})
                if (e) (void)hipEventDestroy(e);
            if (own) (void)hipStreamDestroy(own);
        }
    } L;
    if (!st) {
        HIP_TRY(hipStreamCreate(&L.own));
        st = L.own;
        stream = (void*)L.own;
    }
    int rc;
    for (int i = 0; i < warmup; ++i)
        if ((rc = ehyb_spmv(P, x, y, stream)) != EHYB_OK) return rc;
    if (P->cfg.graphs != 2 && iters >= 2 * kBatch && hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        int erc = EHYB_OK;
        for (int i = 0; i < kBatch && erc == EHYB_OK; ++i) erc = ehyb_spmv(P, x, y, stream);
        const hipError_t eend = hipStreamEndCapture(st, &L.graph);
        if (erc != EHYB_OK || eend != hipSuccess || hipGraphInstantiate(&L.exec, L.graph, nullptr, nullptr, 0) != hipSuccess)
            L.exec = nullptr;
        (void)hipGetLastError();
    }
    HIP_TRY(hipEventCreate(&L.a));
    HIP_TRY(hipEventCreate(&L.b));
    HIP_TRY(hipEventCreate(&L.t[0]));
    HIP_TRY(hipEventCreate(&L.t[1]));
    HIP_TRY(hipEventRecord(L.a, st));
    int done = 0, marks = 0, since = 0;
    while (done < iters) {
        if (L.exec && done + kBatch <= iters) {
            HIP_TRY(hipGraphLaunch(L.exec, st));
            done += kBatch;
            since += kBatch;
        } else {
            if ((rc = ehyb_spmv(P, x, y, stream)) != EHYB_OK) return rc;
            ++done;
            ++since;
        }
        if (since >= kThrottle) {  // wait for the mark before the one just set
            HIP_TRY(hipEventRecord(L.t[marks & 1], st));
            if (marks > 0) HIP_TRY(hipEventSynchronize(L.t[(marks - 1) & 1]));
            ++marks;
            since = 0;
        }
    }
    HIP_TRY(hipEventRecord(L.b, st));
    HIP_TRY(hipEventSynchronize(L.b));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, L.a, L.b));
    if (ms_total) *ms_total = ms;
    if (ms_ell || ms_er) {
        const int n = std::min(iters, 200);
        struct Events {  // destroyed on every way out of this block
            std::vector<hipEvent_t> v;
            ~Events()
            {
                for (hipEvent_t e : v)
                    if (e) (void)hipEventDestroy(e);
            }
        } evs;
        evs.v.assign((size_t)3 * n, nullptr);
        std::vector<hipEvent_t>& ev = evs.v;
        for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
        for (int i = 0; i < n; ++i) {
            const bool fused = P->host.inline_er;
            HIP_TRY(hipEventRecord(ev[3 * i + 0], st));
            if ((rc = launch_ell(P, x, y, st, fused)) != EHYB_OK) return rc;
            HIP_TRY(hipEventRecord(ev[3 * i + 1], st));
            if (!fused && (rc = launch_er(P, x, y, st)) != EHYB_OK) return rc;
            HIP_TRY(hipEventRecord(ev[3 * i + 2], st));
        }
        HIP_TRY(hipEventSynchronize(ev.back()));
        double se = 0, sr = 0;
        for (int i = 0; i < n; ++i) {
            float t1 = 0, t2 = 0;
            HIP_TRY(hipEventElapsedTime(&t1, ev[3 * i + 0], ev[3 * i + 1]));
            HIP_TRY(hipEventElapsedTime(&t2, ev[3 * i + 1], ev[3 * i + 2]));
            se += t1;
            sr += t2;
        }
        if (ms_ell) *ms_ell = se / n;
        if (ms_er) *ms_er = sr / n;
    }
    return EHYB_OK;
}

int ehyb_spmv_host(ehyb_plan* P, const double* x_host, double* y_host, int iters)
{
    if (!P || !x_host || !y_host || iters < 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmv_host: bad arguments");
    if (!P->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_spmv_host: plan not uploaded (no CPU fallback exists)");
    const size_t n = (size_t)P->host.n_cols;
    double *dx = nullptr, *dy = nullptr;
    HIP_TRY(hipMalloc((void**)&dx, n * 8));
    HIP_TRY(hipMalloc((void**)&dy, n * 8));
    HIP_TRY(hipMemcpy(dx, x_host, n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dy, 0, n * 8));
    int rc = EHYB_OK;
    for (int i = 0; i < iters && rc == EHYB_OK; ++i) rc = ehyb_spmv(P, dx, dy, nullptr);
    if (rc == EHYB_OK) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(y_host + P->host.row_begin, dy + P->host.row_begin,
                          (size_t)(P->host.row_end - P->host.row_begin) * 8, hipMemcpyDeviceToHost));
    }
    (void)hipFree(dx);
    (void)hipFree(dy);
    return rc;
}

int ehyb_plan_create(const matrixCOO* m, const ehyb_config* cfg, ehyb_plan** plan)
{
    if (!m) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_create: null matrix");
    return ehyb_plan_create_segs(m, 0, m->dimension, cfg, 0, nullptr, plan);
}

// Build + upload.  What the device can build is left to it (cfg.symbolic): the host lays out the windows and leaves a
// panel-form residual as the entries in row order; the device deals them out (er_panel_dev.hip).
int ehyb_plan_create_segs(const matrixCOO* m, int row_begin, int row_end, const ehyb_config* cfg, int n_col_segs, const int* col_seg_first,
                          ehyb_plan** plan)
{
    clear_error();
    if (!plan) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_create: null output");
    *plan = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1)
        EHYB_FAIL(EHYB_ERR_NO_DEVICE, "ehyb_plan_create: no HIP device visible (the EHYB multiply has no CPU fallback)");
    const double t0 = wall_seconds();
    // The device builder holds ~80 bytes of temporaries per residual entry at its peak (sort keys and payloads twice, rows,
    // columns, values, the streams): where the device has not got that free -- every entry of the rows taken as residual, the
    // most it can be -- the panel form is built on the host instead (same arrays, slower).
    bool on_device_ok = true;
    if (m && m->rowIdx && row_begin >= 0 && row_end <= m->dimension && row_begin < row_end) {
        size_t free_b = 0, total_b = 0;
        const double need = 80.0 * (double)((int64_t)m->rowIdx[row_end] - m->rowIdx[row_begin]) + 268435456.0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || (double)free_b < need) on_device_ok = false;
    }
    int rc = create_host_plan(m, row_begin, row_end, cfg, n_col_segs, col_seg_first, on_device_ok, plan);
    if (rc != EHYB_OK) return rc;
    const double t1 = wall_seconds();
    bool on_device = (*plan)->host.deferred.pending;
    if (on_device) rc = build_panel_on_device(*plan);
    if (on_device && rc != EHYB_OK && (rc == EHYB_ERR_HIP || rc == EHYB_ERR_ALLOC)) {
        // the device ran out of memory after all (ranks that share a device can each pass the check above before the other
        // allocates) or a sort failed: the matrix is still with the caller -- build the whole layout again with the panel form on the
        // host (the same arrays, slower) instead of giving up
        const std::string why = ehyb_last_error();
        (void)hipGetLastError();
        ehyb_plan_destroy(*plan);
        *plan = nullptr;
        rc = create_host_plan(m, row_begin, row_end, cfg, n_col_segs, col_seg_first, false, plan);
        if (rc != EHYB_OK) return rc;
        if ((*plan)->cfg.verbose) printf("plan: the device builder failed (%s): panel form rebuilt on the host\n", why.c_str());
        on_device = false;
    }
    const double t2 = wall_seconds();
    if (rc == EHYB_OK) rc = ehyb_plan_upload(*plan);
    if (rc != EHYB_OK) {
        ehyb_plan_destroy(*plan);
        *plan = nullptr;
        return rc;
    }
    if ((*plan)->cfg.verbose)
        printf("plan: host layout %.3f s, panel form %s %.3f s, upload %.3f s\n", t1 - t0, on_device ? "on the device" : "(host, included)", t2 - t1,
               wall_seconds() - t2);
    return rc;
}

// The drop-in entry point (reference spmv.cu:61-133).  cfg == NULL: defaults, storage chosen from
// the matrix (sym_storage_suits) -- no environment variable takes part.
int spmvGPuEHYB_cfg(matrixCOO* localMatrix, const double* vectorIn, double* vectorOut, const int MAXIter,
                    int* realIter, const ehyb_config* cfg_in, double* ms_total)
{
    clear_error();
    if (!localMatrix || !vectorIn || !vectorOut || MAXIter < 0)
        EHYB_FAIL(EHYB_ERR_ARG, "spmvGPuEHYB: bad arguments");
    ehyb_config cfg;
    memset(&cfg, 0, sizeof cfg);  // zero = default; the sizes follow from the mode fields
    if (cfg_in)
        cfg = *cfg_in;
    else if (sym_storage_suits(localMatrix))
        cfg.sym_pairs = 1;
    ehyb_plan* P = nullptr;
    int rc = ehyb_plan_create(localMatrix, &cfg, &P);  // COO2EHYB + upload (spmv.cu:73-81)
    if (rc != EHYB_OK) return rc;
    printf("sizeER is %lld\n", (long long)P->host.stats.size_er);  // spmv.cu:82
    const size_t n = (size_t)localMatrix->dimension;
    double *dx = nullptr, *dy = nullptr;
    auto fail = [&](int code) {
        if (dx) (void)hipFree(dx);
        if (dy) (void)hipFree(dy);
        ehyb_plan_destroy(P);
        return code;
    };
    if (hipMalloc((void**)&dx, n * 8) != hipSuccess || hipMalloc((void**)&dy, n * 8) != hipSuccess) {
        set_error("spmvGPuEHYB: device allocation of the vectors failed");
        return fail(EHYB_ERR_HIP);
    }
    if (hipMemcpy(dx, vectorIn, n * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(dy, 0, n * 8) != hipSuccess) {
        set_error("spmvGPuEHYB: upload of x failed");
        return fail(EHYB_ERR_HIP);
    }
    double ms = 0;
    const int iters = std::max(1, MAXIter);
    // part of the warm-up: the heaviest work items onto the XCDs of THIS device that stream fastest (a few stamped
    // launches; keeps what it finds only if the launch got shorter; its failure is not the multiply's)
    if (ehyb_plan_tune(P, dx, dy, 3, nullptr, nullptr) != EHYB_OK) clear_error();
    rc = ehyb_spmv_bench(P, dx, dy, nullptr, 10, iters, &ms, nullptr, nullptr);  // spmv.cu:100-116
    if (rc != EHYB_OK) return fail(rc);
    if (hipMemcpy(vectorOut, dy, n * 8, hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("spmvGPuEHYB: download of y failed");
        return fail(EHYB_ERR_HIP);
    }
    printf("iter is %d, time is %f ms, GPU Gflops is %f\n ", iters, ms,
           (1e-9 * ((double)localMatrix->totalNum * 2) * 1000 * iters) / ms);  // spmv.cu:121-122
    if (realIter) *realIter = iters;
    if (ms_total) *ms_total = ms;
    fail(EHYB_OK);
    return EHYB_OK;
}

int spmvGPuEHYB_status(matrixCOO* localMatrix, const double* vectorIn, double* vectorOut, const int MAXIter,
                       int* realIter)
{
    return spmvGPuEHYB_cfg(localMatrix, vectorIn, vectorOut, MAXIter, realIter, nullptr, nullptr);
}

void spmvGPuEHYB(matrixCOO* localMatrix, const double* vectorIn, double* vectorOut, const int MAXIter,
                 int* realIter)
{
    int rc = spmvGPuEHYB_status(localMatrix, vectorIn, vectorOut, MAXIter, realIter);
    if (rc != EHYB_OK) {
        fprintf(stderr, "spmvGPuEHYB failed (%d): %s\n", rc, ehyb_last_error());
        exit(rc);
    }
}

}  // extern "C"
