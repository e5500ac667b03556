// The window kernel and the CSR-segment residual, device side, written once for K = 1..4 columns (ehyb_hip.hip instantiates
// them: ehyb_ell_kernel / ehyb_er_kernel are K = 1, ehyb_ell_k_kernel / ehyb_er_k_kernel K = 2, 3, 4).  Column j of X and Y is
// ldx / ldy doubles behind column 0; the value stream, the column words, the lane maps and the slab records are read ONCE for all K
// columns, what grows with K is the x image in LDS and the x / y traffic.  The window is staged INTERLEAVED, win[c*K + j] =
// X[col(c) + j*ldx] for own rows and halo alike, so that a lane fetches the K values of one column with one (K = 2) or two (K = 4)
// LDS reads.  Per column the order of the sums is the one-vector order (inline residual, then even and odd pair halves, then
// acc0 + acc1): column j of a plain-storage multiply is bit for bit the one-vector multiply of X[:, j].  At K = 1 every piece
// reduces to the one-vector code (win_load<1> is win[idx], yacc = win + cnt + hn).  Only K = 1 has the round-robin walk (DYN =
// false), the diagnostic stamps (STAMP, probe_n) and x . y on the side (xy_out); symmetric pairs at K = 4 step two value pairs
// instead of four.  Internal: nothing here is part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "ehyb_internal.h"

// (global namespace, as before the split: the kernels' symbol names stay what profiles and tools know)
struct EllArgs {
    const int4* __restrict__ items;
    const int4* __restrict__ segs;
    const int* __restrict__ halo_cols;
    const uint4* __restrict__ slab_meta;
    const uint8_t* __restrict__ lane_group;
    const uint16_t* __restrict__ slab_lrow;  // SYM: the row (place in the LDS image) of every lane, 0xFFFF = none
    const double2* __restrict__ ell_val;
    const uint32_t* __restrict__ ell_col;
    const double* __restrict__ x;
    double* __restrict__ y;
    int win_cap;
    const int* __restrict__ item_map;  // non-null (ehyb_plan_tune): workgroup b takes item item_map[b]
    int xcd_map;  // 1: workgroup b takes item xcd_item(b), so that each XCD works on one contiguous run of items
    int windowless_zero;  // 1: a partition without a window gets y = 0 here; 0: the panel residual's second pass assigns its y
    unsigned long long* __restrict__ stamps;
    // non-null (ehyb_cg): the workgroup also leaves sum over its rows of y[row] * x[row] in xy_out[blockIdx.x] -- the p.q of
    // a conjugate-gradient step falls out of the multiply (the rows' x sits in the window, y in registers or accumulators)
    double* __restrict__ xy_out;
    // 1: the workgroup walks the slabs of a segment last to first.  Back-to-back multiplies of one plan alternate (cfg.ell_alternate):
    // what the previous launch streamed LAST is what still sits in the 256 MB Infinity Cache, and this launch reads it FIRST.
    int reverse;
    int reverse_items;  // with reverse, and more items than resident workgroups: workgroup b takes the items from the far end too
    // diagnostic launches only (stamps != null; ehyb_debug_ell_stamps_probe): > 0 = every window entry is staged from THREE vectors instead of
    // one (x and two shifted copies of it, `probe_n` entries long) -- what folding CG's direction update p = z + beta p into the staging
    // would gather (r, the old p, 1 / diag): how much longer the launch gets is the price of that fold
    int probe_n;
    // The value stream is read ONCE per multiply: loaded with the non-temporal hint it streams past the caches, which then hold what is read
    // again (column words shared by lanes, lane maps, x) -- 0.69 -> 0.78 of the peak for a launch that walks first to last, every entry stored
    // 1126 -> 1290 GFLOP/s (profiles/r04_nt_hints_ab.txt).  The slabs that ell_slab_resident(.., keep1024, keep_shape) marks are read with
    // plain loads instead, so that the 256 MB Infinity Cache keeps them for the next launch; every other slab with the hint.
    int keep1024;    // share of a segment's slabs read with plain loads, in 1/1024 (0 = none, 1024 = all)
    int keep_shape;  // ELL_KEEP_*: which slabs those are
};

// Which slabs of a segment are read with plain loads (and so stay in the Infinity Cache), the rest with the non-temporal hint.
//   SPREAD, BLOCK: a FIXED set, a function of the slab's index in its segment -- the same slabs in every launch, whatever the walk
//     direction, so that after the first launch nothing but x, y and the column words allocates in the cache and nothing evicts the set.
//     SPREAD picks evenly over the index (Bresenham; the slabs of a partition are sorted by length, so evenly over the bytes too), BLOCK
//     the first keep1024 / 1024 of the segment.  Both mark floor(n * keep1024 / 1024) slabs, never more than the share asked for.
//   WALK_END (cfg.ell_nt = 3, rounds 4-5): a function of the walk POSITION -- the last keep1024 / 1024 of every walk, which the
//     next launch of an alternating plan reads first.
enum { ELL_KEEP_WALK_END = 0, ELL_KEEP_SPREAD = 1, ELL_KEEP_BLOCK = 2 };

// pos: SPREAD, BLOCK the slab's index in its segment of n slabs; WALK_END its position in the walk
__host__ __device__ inline bool ell_slab_resident(int pos, int n, int keep1024, int shape)
{
    if (shape == ELL_KEEP_SPREAD) return (((long long)(pos + 1) * keep1024) >> 10) != (((long long)pos * keep1024) >> 10);
    if (shape == ELL_KEEP_BLOCK) return pos < (int)(((long long)n * keep1024) >> 10);
    return pos >= (int)(((long long)n * (1024 - keep1024) + 1023) >> 10);
}

// Workgroups are handed to the 8 XCDs round robin (b mod 8).  With this map XCD k gets the k-th
// contiguous eighth of the items: neighbouring partitions, whose halo columns are each other's
// rows, then share one L2.
__device__ __forceinline__ int xcd_item(int b, int n)
{
    const int k = b & 7, j = b >> 3, chunk = n >> 3, rem = n & 7;
    return k * chunk + min(k, rem) + j;
}

// Which work item workgroup b takes: the tuned map of the plan (ehyb_plan_tune: the heaviest items on the XCDs that were
// measured fastest), else one contiguous run of items per XCD (plain storage), else item b.
__device__ __forceinline__ int item_of_block(const int* __restrict__ item_map, int xcd_map, int from_the_end = 0)
{
    const int b = from_the_end ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
    return item_map ? item_map[b] : (xcd_map ? xcd_item(b, (int)gridDim.x) : b);
}

// The value of the next lane (lane + 1), 0 behind the last one: two DPP moves, no LDS traffic.
__device__ __forceinline__ double next_lane(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// the (value, value) pair of one lane: plain, or past the caches
template <bool NT>
__device__ __forceinline__ double2 ell_load_pair(const double2* __restrict__ p)
{
    if (NT) {
        double2 r;
        r.x = __builtin_nontemporal_load(&p->x);
        r.y = __builtin_nontemporal_load(&p->y);
        return r;
    }
    return *p;
}
// cfg.val_f32: the pair as the device holds it in fp32 -- one 8-byte load.  A step keeps what its loads return (float2: half the
// registers of a double2 while the loads are in flight) and converts each half to fp64 once, where the pair is first used
// (ell_pair); everything behind that is the fp64 code.
template <bool NT>
__device__ __forceinline__ float2 ell_load_pair(const float2* __restrict__ p)
{
    if (NT) {
        typedef float pair_f32 __attribute__((ext_vector_type(2)));
        const pair_f32 r = __builtin_nontemporal_load(reinterpret_cast<const pair_f32*>(p));
        return make_float2(r.x, r.y);
    }
    return *p;
}
__device__ __forceinline__ const double2& ell_pair(const double2& r) { return r; }
__device__ __forceinline__ double2 ell_pair(const float2& r) { return make_double2((double)r.x, (double)r.y); }
// a pair used where it is loaded (single pairs behind the steps, the inline residual)
template <bool NT, class VP>
__device__ __forceinline__ double2 ell_load_pair_f64(const VP* __restrict__ p)
{
    if constexpr (sizeof(VP) == sizeof(double2))
        return ell_load_pair<NT>(p);
    else
        return ell_pair(ell_load_pair<NT>(p));
}
template <class VP>
__device__ __forceinline__ VP ell_zero_pair();
template <>
__device__ __forceinline__ double2 ell_zero_pair<double2>() { return make_double2(0.0, 0.0); }
template <>
__device__ __forceinline__ float2 ell_zero_pair<float2>() { return make_float2(0.0f, 0.0f); }
// fp32 values: the loads of a step are issued before its first conversion (left to itself the scheduler converts and multiplies
// each pair behind its own load, one load in flight per wave); nothing for fp64, whose kernels stay as they are
template <class VP>
__device__ __forceinline__ void ell_loads_issued()
{
    if constexpr (sizeof(VP) == sizeof(float2)) __builtin_amdgcn_sched_barrier(0);
}

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

// ------------------------------------------------------------------ window kernel
// items[2b]   = {first segment, end segment, -, -}      items[2b+1] = residual bins of the item
// segs[2g]    = {partition, first slab, end slab, halo count}
// segs[2g+1]  = {first row, end row, contiguous window length, halo start}
// DYN   waves take slabs from an LDS counter (the reference's per-block queue, kernel.cu:142,
//       164-166; here re-armed per segment) -- the default; false: slabs dealt round-robin (A/B arm).
//       A third arm -- global per-segment counters plus idle workgroups helping the busiest segment
//       -- was measured and dropped: the device-scope atomic per slab cost 6 % by itself and the
//       helping, at ~2 slabs per wave, evened the finish times without shortening the launch.
// STAMP:   diagnostic instantiation (tools/stamps.py only): thread 0 records the 100 MHz wall clock
//          at entry, after the first staging and at exit into a buffer of its own.
// INLINE_ER: slabs also multiply the residual pairs stored behind their ELL pairs (tiny residuals).

// One entry of a slab for K columns: gather x from the window; SYM: bit 15 of the column says "this entry also
// stands for its mirror image": value * x[own row] goes to row `column`'s accumulator in LDS.
// Lanes of a group (equal column lists: the unknowns of a node) send their mirror products to the
// SAME accumulator.  Summed across the lanes first (`code`: this lane adds for itself and the next
// 0/1/2 lanes, 3 = a lane before it adds for this one), a group of three costs one ds_add_f64
// instead of three that the hardware has to serialise.
// (ell_entry_at: the same with the column and its mirror flag apart, as the triple-coded slabs have them)
template <int K, bool SYM>
__device__ __forceinline__ void ell_entry_at(double v, uint32_t idx, bool mirror, const double* __restrict__ win, double* yacc, const double (&xi)[K],
                                             int code, double (&acc)[K])
{
    double w[K];
    if (SYM) {
        win_load<K>(win, idx, w);
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] = fma(v, w[j], acc[j]);
        if constexpr (K == 1) {  // (written without the loop: even one trip of it costs the one-vector kernel a VGPR)
            const double mine = mirror ? v * xi[0] : 0.0;
            const double n1 = next_lane(mine), n2 = next_lane(n1);
            const double sum = mine + ((code == 1 || code == 2) ? n1 : 0.0) + (code == 2 ? n2 : 0.0);
            if (mirror && code != 3) unsafeAtomicAdd(&yacc[idx], sum);  // ds_add_f64
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double mine = mirror ? v * xi[j] : 0.0;
                const double n1 = next_lane(mine), n2 = next_lane(n1);
                const double sum = mine + ((code == 1 || code == 2) ? n1 : 0.0) + (code == 2 ? n2 : 0.0);
                if (mirror && code != 3) unsafeAtomicAdd(&yacc[idx * K + j], sum);
            }
        }
    } else {
        win_load<K>(win, idx, w);
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] = fma(v, w[j], acc[j]);
    }
}

template <int K, bool SYM>
__device__ __forceinline__ void ell_entry(double v, uint32_t col16, const double* __restrict__ win, double* yacc, const double (&xi)[K],
                                          int code, double (&acc)[K])
{
    ell_entry_at<K, SYM>(v, SYM ? (col16 & 0x7fffu) : col16, SYM && (col16 & 0x8000u) != 0, win, yacc, xi, code, acc);
}

// The three value pairs of one column word (A, B) of a triple-coded slab: columns (A, A+1), (A+2, B), (B+1, B+2).  A base carries
// the mirror flag of its triple in bit 15 (symmetric pairs).  No mask for lanes without a row (plain storage): the slab is not
// relative, so the columns of any group of it lie in the window, and such a lane writes nothing.  `pairs` < 3: the first one or two.
template <int K, bool SYM>
__device__ __forceinline__ void ell_triple_word(const double2& v0, const double2& v1, const double2& v2, uint32_t w, int pairs,
                                                const double* __restrict__ win, double* yacc, const double (&xi)[K], int code,
                                                double (&acc0)[K], double (&acc1)[K])
{
    const uint32_t a = w & (SYM ? 0x7fffu : 0xffffu), b = SYM ? (w >> 16) & 0x7fffu : w >> 16;
    const bool ma = SYM && (w & 0x8000u) != 0, mb = SYM && (w & 0x80000000u) != 0;
    ell_entry_at<K, SYM>(v0.x, a, ma, win, yacc, xi, code, acc0);
    ell_entry_at<K, SYM>(v0.y, a + 1, ma, win, yacc, xi, code, acc1);
    if (pairs < 2) return;
    ell_entry_at<K, SYM>(v1.x, a + 2, ma, win, yacc, xi, code, acc0);
    ell_entry_at<K, SYM>(v1.y, b, mb, win, yacc, xi, code, acc1);
    if (pairs < 3) return;
    ell_entry_at<K, SYM>(v2.x, b + 1, mb, win, yacc, xi, code, acc0);
    ell_entry_at<K, SYM>(v2.y, b + 2, mb, win, yacc, xi, code, acc1);
}

// One slab of 64 rows.  xy (K = 1, A.xy_out set): the lane's running sum of y[row] * x[row].
// VP: the value pair as the device holds it -- double2, or float2 (cfg.val_f32: A.ell_val reinterpreted, same offsets in pairs).
template <int K, bool INLINE_ER, bool SYM, bool NT, class VP = double2>
__device__ __forceinline__ void ell_slab(const EllArgs& A, long long ldx, long long ldy, const double* __restrict__ win, double* yacc, int s,
                                         int base, int pe, int lane, double& xy)
{
    // slab record {first value pair, first column word, first row, pairs << 16 | residual pairs << 8 | groups - 1}
    const uint4 sm = A.slab_meta[s];
    const int np = (int)(sm.w >> 16);
    const int G = (int)(sm.w & 0x3fu) + 1;  // lanes with equal column lists share one word per pair
    const VP* __restrict__ v = reinterpret_cast<const VP*>(A.ell_val) + (size_t)sm.x * 64 + lane;
    // the lane's group (bits 0-5) and, with symmetric pairs, its part in the group's sum (bits 6-7)
    const uint32_t lgb = A.lane_group[(size_t)s * 64 + lane];
    const int code = SYM ? (int)(lgb >> 6) : 0;
    const uint32_t* __restrict__ c = A.ell_col + sm.y + (SYM ? (lgb & 0x3fu) : lgb);
    double acc0[K], acc1[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc0[j] = 0.0, acc1[j] = 0.0;
    if (INLINE_ER) {
        // Inline residual (tiny residuals only): `ner` more pairs behind the slab's ELL pairs, their
        // columns global -- [pair][2][lane] 32-bit words behind the slab's shared column words.
        // First, so that the loads are in flight while the ELL pairs stream; only the gather of x
        // from global memory (L2) waits for them.  No second launch, no read-modify-write of y.
        const int ner = (int)(sm.w >> 8) & 0xff;
        const VP* __restrict__ ve = v + (size_t)np * 64;
        const uint32_t* __restrict__ ce = A.ell_col + sm.y + (size_t)np * G + lane;
        for (int q = 0; q < ner; ++q) {
            const double2 vv = ell_load_pair_f64<false>(ve + q * 64);
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
    // Plain: lane l works on row sm.z + l.  SYM: the rows of a partition sit in its slabs longest
    // first (any order will do: sums go to the LDS accumulators by row), slab_lrow names the row.
    const int row = (int)sm.z + lane;
    const int lrow = SYM ? (int)A.slab_lrow[(size_t)s * 64 + lane] : row - base;  // place in the LDS image
    const bool has_row = SYM ? lrow != 0xFFFF : row < pe;
    double xi[K];
    if (SYM && has_row)
        win_load<K>(win, (uint32_t)lrow, xi);
    else
#pragma unroll
        for (int j = 0; j < K; ++j) xi[j] = 0.0;
    // bit 7 of the record: the slab's columns are stored relative to the lane's own row (bands and
    // stencils: rows with equal offsets share their words); lanes without a row read column 0
    const uint32_t radd = (!SYM && (sm.w & 0x80u)) ? (uint32_t)lrow : 0u;
    const uint32_t cmask = (SYM || has_row) ? 0xffffu : 0u;
#define ELL_COL_LO(c) (SYM ? ((c) & 0xffffu) : ((((c) & 0xffffu) + radd) & cmask))
#define ELL_COL_HI(c) (SYM ? ((c) >> 16) : ((((c) >> 16) + radd) & cmask))
    // bit 6 of the record (device copy only, col_triples.h): the slab's column words hold one 16-bit base per node triple, two
    // per word.  Wave-uniform.  The pairs come in the order, and on the accumulators, of the pair form below.
    //   one vector, symmetric pairs (up to 128 VGPRs): six value pairs and two column words per step, then one step of three;
    //   plain storage at K = 1 (64 VGPRs) and K = 2, 3: a word's three pairs per step -- six spill;
    //   K = 4: a word's three pairs, the third loaded once the first has been multiplied;
    // then one or two pairs from one more word.
    // (K = 4 with symmetric pairs AND an inline residual spilled with both forms in it, 128 VGPRs: col_triples.cpp codes no slab
    // of a plan that can take that kernel, and the arm is left out of it)
    constexpr bool kTriples = !(K >= ehyb::kNoTripleArmK && SYM && INLINE_ER);
    if (kTriples && (sm.w & 0x40u)) {
        // Running pointers and a count.  The empty asm hides where the pointers come from: without it the compiler hoists this
        // arm's lane addresses (ell_val + lane + a constant, ...) out of the walk over the slabs, next to the ones of the pair
        // form, and the kernels built for 64 VGPRs have no registers for both -- they spilled.
        const VP* vp = v;
        const uint32_t* cp = c;
        asm volatile("" : "+v"(vp), "+v"(cp));
        int left = np;
        if constexpr (K >= 4) {
#pragma nounroll
            for (; left >= 3; left -= 3, vp += 3 * 64, cp += G) {
                // (one pair in flight: the barriers keep the next pair's load behind this pair's products -- registers)
                const uint32_t w0 = cp[0];
                const uint32_t a = w0 & (SYM ? 0x7fffu : 0xffffu), b = SYM ? (w0 >> 16) & 0x7fffu : w0 >> 16;
                const bool ma = SYM && (w0 & 0x8000u) != 0, mb = SYM && (w0 & 0x80000000u) != 0;
                const double2 v0 = ell_load_pair<NT>(vp);
                ell_entry_at<K, SYM>(v0.x, a, ma, win, yacc, xi, code, acc0);
                ell_entry_at<K, SYM>(v0.y, a + 1, ma, win, yacc, xi, code, acc1);
                __builtin_amdgcn_sched_barrier(0);
                const double2 v1 = ell_load_pair<NT>(vp + 64);
                ell_entry_at<K, SYM>(v1.x, a + 2, ma, win, yacc, xi, code, acc0);
                ell_entry_at<K, SYM>(v1.y, b, mb, win, yacc, xi, code, acc1);
                __builtin_amdgcn_sched_barrier(0);
                const double2 v2 = ell_load_pair<NT>(vp + 2 * 64);
                ell_entry_at<K, SYM>(v2.x, b + 1, mb, win, yacc, xi, code, acc0);
                ell_entry_at<K, SYM>(v2.y, b + 2, mb, win, yacc, xi, code, acc1);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            if constexpr (SYM && K == 1) {
                for (; left >= 6; left -= 6, vp += 6 * 64, cp += 2 * G) {
                    VP vv[6];
#pragma unroll
                    for (int q = 0; q < 6; ++q) vv[q] = ell_load_pair<NT>(vp + q * 64);
                    const uint32_t w0 = cp[0], w1 = cp[G];
                    ell_loads_issued<VP>();
                    ell_triple_word<K, SYM>(ell_pair(vv[0]), ell_pair(vv[1]), ell_pair(vv[2]), w0, 3, win, yacc, xi, code, acc0, acc1);
                    ell_triple_word<K, SYM>(ell_pair(vv[3]), ell_pair(vv[4]), ell_pair(vv[5]), w1, 3, win, yacc, xi, code, acc0, acc1);
                }
            }
#pragma nounroll
            for (; left >= 3; left -= 3, vp += 3 * 64, cp += G) {
                VP vv[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) vv[q] = ell_load_pair<NT>(vp + q * 64);
                const uint32_t w0 = cp[0];
                ell_loads_issued<VP>();
                ell_triple_word<K, SYM>(ell_pair(vv[0]), ell_pair(vv[1]), ell_pair(vv[2]), w0, 3, win, yacc, xi, code, acc0, acc1);
            }
        }
        if constexpr (K >= 4) {
            if (left > 0) {  // (wave-uniform, as `left > 1`)
                const uint32_t w0 = cp[0];
                const uint32_t a = w0 & (SYM ? 0x7fffu : 0xffffu), b = SYM ? (w0 >> 16) & 0x7fffu : w0 >> 16;
                const bool ma = SYM && (w0 & 0x8000u) != 0, mb = SYM && (w0 & 0x80000000u) != 0;
                const double2 v0 = ell_load_pair<NT>(vp);
                ell_entry_at<K, SYM>(v0.x, a, ma, win, yacc, xi, code, acc0);
                ell_entry_at<K, SYM>(v0.y, a + 1, ma, win, yacc, xi, code, acc1);
                __builtin_amdgcn_sched_barrier(0);
                if (left > 1) {
                    const double2 v1 = ell_load_pair<NT>(vp + 64);
                    ell_entry_at<K, SYM>(v1.x, a + 2, ma, win, yacc, xi, code, acc0);
                    ell_entry_at<K, SYM>(v1.y, b, mb, win, yacc, xi, code, acc1);
                }
            }
        } else if (left > 0) {
            const VP v0 = ell_load_pair<NT>(vp);
            VP v1 = ell_zero_pair<VP>();
            if (left > 1) v1 = ell_load_pair<NT>(vp + 64);
            const uint32_t w0 = cp[0];
            ell_loads_issued<VP>();
            ell_triple_word<K, SYM>(ell_pair(v0), ell_pair(v1), ell_pair(v1), w0, left, win, yacc, xi, code, acc0, acc1);
        }
    } else {
    // Four value pairs per step; symmetric pairs at K = 4 take two, which keeps them within 128 VGPRs.
    // (an 8-pair step for SYM, 128 VGPRs at 16 waves per CU, measured 1 % slower than four at K = 1)
    constexpr int STEP = (SYM && K >= 4) ? 2 : 4;
    int k = 0;
    for (; k + STEP <= np; k += STEP) {
        VP vv[STEP];
        uint32_t cc[STEP];
#pragma unroll
        for (int q = 0; q < STEP; ++q) vv[q] = ell_load_pair<NT>(v + (k + q) * 64);
#pragma unroll
        for (int q = 0; q < STEP; ++q) cc[q] = c[(k + q) * G];
        ell_loads_issued<VP>();
#pragma unroll
        for (int q = 0; q < STEP; ++q) {
            ell_entry<K, SYM>(ell_pair(vv[q]).x, ELL_COL_LO(cc[q]), win, yacc, xi, code, acc0);
            ell_entry<K, SYM>(ell_pair(vv[q]).y, ELL_COL_HI(cc[q]), win, yacc, xi, code, acc1);
        }
    }
    for (; k < np; ++k) {
        const double2 v0 = ell_load_pair_f64<NT>(v + k * 64);
        const uint32_t c0 = c[k * G];
        ell_entry<K, SYM>(v0.x, ELL_COL_LO(c0), win, yacc, xi, code, acc0);
        ell_entry<K, SYM>(v0.y, ELL_COL_HI(c0), win, yacc, xi, code, acc1);
    }
    }
#undef ELL_COL_LO
#undef ELL_COL_HI
    if (has_row) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (SYM)
                unsafeAtomicAdd(&yacc[lrow * K + j], acc0[j] + acc1[j]);  // other lanes scatter into the same accumulator
            else
                A.y[row + j * ldy] = acc0[j] + acc1[j];
        }
        if (!SYM && K == 1 && A.xy_out != nullptr) xy = fma(acc0[0] + acc1[0], win[lrow], xy);  // (own rows are in the window)
    }
}

// Stage the window of segment g and multiply its slabs.
// SYM (symmetric pair storage): the segment is a whole partition; its rows' accumulators sit in LDS
// right behind the K-wide x image, take the lanes' own sums and the scattered mirror products, and are
// written to y in one coalesced sweep at the end.
template <int THREADS, int K, bool DYN, bool INLINE_ER, bool SYM, bool STAMP, class VP = double2>
__device__ __forceinline__ void ell_segment(const EllArgs& A, long long ldx, long long ldy, double* __restrict__ win,
                                            int* __restrict__ next_slab, int g, int lane, int wave, double& xy)
{
    constexpr int WAVES = THREADS / 64;
    const int4 a = A.segs[2 * g], b = A.segs[2 * g + 1];
    const int sb = a.y, se = a.z, hn = a.w;
    const int ps = b.x, pe = b.y, wl = b.z, hb = b.w;
    if (!SYM && wl == 0 && hn == 0) {
        // a partition whose rows all went to the residual (its window did not pay, plan.cpp): nothing to
        // stage, no slab to walk -- the residual launch adds to y, so y = 0 in one coalesced sweep
        // (walking its empty slabs cost 22 us on R-MAT 2^22, 70 us on 2^24)
        if (!A.windowless_zero) return;  // pb_assign: pass 2 of the panel residual is the only writer of these rows
        const int r0 = max(ps, (int)A.slab_meta[sb].z), r1 = min(pe, r0 + (se - sb) * 64);
        for (int i = r0 + (int)threadIdx.x; i < r1; i += THREADS)
#pragma unroll
            for (int j = 0; j < K; ++j) A.y[i + j * ldy] = 0.0;
        return;
    }
    __syncthreads();  // every wave is done with the previous window and counter
    // The LDS image starts at the even row at or below the partition start (the layout builder
    // numbers window-local columns from there); win[0] may hold x[ps-1], unused.
    const int base = ps & ~1, cnt = wl + (ps & 1);
    double* yacc = win + K * (cnt + hn);
    // (SYM: batching all of a thread's staging loads -- indices, then x, stores last -- measured no
    // faster than these loops: 6.1 vs 6.5 us of staging; the halo gathers set the pace)
    if (STAMP && A.probe_n > 0) {   // (diagnostic instantiation only: compiled out of the product's kernels)
        const int n = A.probe_n, o1 = n / 3, o2 = 2 * (n / 3);
        for (int i = threadIdx.x; i < cnt; i += THREADS) {
            const int c = min(base + i, n - 1);
            win[i] = A.x[c] + 1e-300 * (A.x[(c + o1) % n] + A.x[(c + o2) % n]);
        }
        for (int i = threadIdx.x; i < hn; i += THREADS) {
            const int c = A.halo_cols[hb + i];
            win[cnt + i] = A.x[c] + 1e-300 * (A.x[(c + o1) % n] + A.x[(c + o2) % n]);
        }
    } else if (STAMP && A.probe_n < 0) {   // (diagnostic: no halo gather at all -- results wrong, the launch span is what hiding the gather could reach at best)
        for (int i = threadIdx.x; i < cnt; i += THREADS) win[i] = A.x[base + i];
        for (int i = threadIdx.x; i < hn; i += THREADS) win[cnt + i] = 1.0;
    } else {
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
    }
    if (SYM)
        for (int i = threadIdx.x; i < K * cnt; i += THREADS) yacc[i] = 0.0;
    if (DYN && threadIdx.x == 0) *next_slab = sb + WAVES;  // slabs sb..sb+WAVES-1 are pre-assigned
    __syncthreads();
    // diagnostic launches only (tools/stamps.py): when the first window of the item was staged
    // (a run-time test in every one-vector kernel, absent from the k-vector ones, whose launches never stamp)
    if (K == 1 && A.stamps != nullptr && threadIdx.x == 0 &&
        g == A.items[2 * item_of_block(A.item_map, A.xcd_map)].x)
        A.stamps[4 * blockIdx.x + 1] = wall_clock64();
    int s = sb + wave;  // (logical position in the segment's walk; the slab it stands for depends on the direction)
    while (s < se) {
        const int slab = A.reverse ? se - 1 - (s - sb) : s;
        if (ell_slab_resident((A.keep_shape == ELL_KEEP_WALK_END ? s : slab) - sb, se - sb, A.keep1024, A.keep_shape))
            ell_slab<K, INLINE_ER, SYM, false, VP>(A, ldx, ldy, win, yacc, slab, base, pe, lane, xy);
        else
            ell_slab<K, INLINE_ER, SYM, true, VP>(A, ldx, ldy, win, yacc, slab, base, pe, lane, xy);   // value stream past the caches
        if (DYN) {
            int nx = 0;
            if (lane == 0) nx = atomicAdd(next_slab, 1);
            s = __builtin_amdgcn_readfirstlane(nx);
        } else {
            s += WAVES;
        }
    }
    if (SYM) {
        __syncthreads();  // all sums and scatters of the partition are in
        // (Folding the pairs that straddle two partitions as well -- 13 % fewer bytes on the bench
        // matrix -- would need y zeroed first and this write-out plus one add per halo column done
        // with global atomics: that alone was measured at +12.5 us per launch, more than the bytes save.)
        if (K == 1 && A.xy_out != nullptr) {
            for (int i = threadIdx.x + (ps & 1); i < cnt; i += THREADS) {
                A.y[base + i] = yacc[i];
                xy = fma(yacc[i], win[i], xy);
            }
        } else {
            for (int i = threadIdx.x + (ps & 1); i < cnt; i += THREADS)
#pragma unroll
                for (int j = 0; j < K; ++j) A.y[base + i + j * ldy] = yacc[i * K + j];
        }
    }
}

// The body of the window kernel: one workgroup per work item, its segments one after the other.  The LDS slab counter
// sits right behind the K window images.
template <int THREADS, int K, bool DYN, bool STAMP, bool INLINE_ER, bool SYM, class VP = double2>
__device__ __forceinline__ void ell_items(const EllArgs& A, long long ldx, long long ldy)
{
    static_assert(K == 1 || (DYN && !STAMP), "the k-vector window kernel is built with the LDS counter only, without stamps");
    extern __shared__ __attribute__((aligned(16))) double win[];
    int* next_slab = reinterpret_cast<int*>(win + K * A.win_cap);
    if (STAMP && threadIdx.x == 0) A.stamps[4 * blockIdx.x + 0] = wall_clock64();
    const int4 it = A.items[2 * item_of_block(A.item_map, A.xcd_map, A.reverse_items)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double xy = 0.0;
    for (int sg = it.x; sg < it.y; ++sg) ell_segment<THREADS, K, DYN, INLINE_ER, SYM, STAMP, VP>(A, ldx, ldy, win, next_slab, sg, lane, wave, xy);
    if (K == 1 && A.xy_out != nullptr) {  // (wave-uniform: a kernel argument)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) xy += __shfl_xor(xy, off, 64);
        __syncthreads();  // every wave is done with the last window
        if (lane == 0) win[wave] = xy;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
            for (int w = 0; w < THREADS / 64; ++w) t += win[w];  // fixed order
            A.xy_out[blockIdx.x] = t;
        }
    }
    if (STAMP) {
        __syncthreads();
        if (threadIdx.x == 0) {
            A.stamps[4 * blockIdx.x + 2] = wall_clock64();
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            A.stamps[4 * blockIdx.x + 3] = xcc;
        }
    }
}

// ------------------------------------------------------------------ residual segments
// Residual segments [lo, hi) multiplied by one workgroup: G lanes per segment (64 / 16 / 4 by
// segment length, longest first), strided coalesced (col,val) reads, x gathered from global
// memory K times, shuffle reduction per column, then y[row] += sum -- plain for rows with one segment (rows are
// unique, kernel.cu:69-77), one fp64 atomic per segment and column for split rows (the working form of
// kernel.cu:43-67).  Called from ehyb_er_kernel / ehyb_er_k_kernel, which run behind the window launch.
// ASSIGN (direct shape, small matrices): y[row] = sum -- every row has exactly one segment.
// Most residual rows are short (R-MAT 2^22: 22 entries on average), so a lane has one to four entries
// and the time goes into the CHAIN of dependent loads, not into bandwidth: segment bounds -> (column,
// value) -> x[column] -> y.  Everything that does not depend on the products is therefore requested up
// front (row number and the old y with the bounds), and a lane's column/value loads are issued four at
// a time before the first gather of x (measured on R-MAT 2^22: DESIGN.md 3.2).
// VT: a value as the device holds it -- double, or float (cfg.val_f32), converted to fp64 where it is loaded.
template <int G, int THREADS, bool ASSIGN, int K, class VT = double>
__device__ __forceinline__ void er_bin(int lo, int hi, const int64_t* __restrict__ seg_ptr, const int* __restrict__ seg_row,
                                       const int* __restrict__ col, const VT* __restrict__ val, const double* __restrict__ x, long long ldx,
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
            if (!ASSIGN && sub == 0 && r >= 0)  // in flight while the products are formed
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
            // up to three more, again all requested before the first use
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

// One workgroup per descriptor {seg_lo, seg_hi, lanes per segment}: a single pass of same-bin segments.
template <int THREADS, bool ASSIGN, int K, class VT = double>
__device__ __forceinline__ void er_blocks(const int4* __restrict__ blocks, const int64_t* __restrict__ seg_ptr, const int* __restrict__ seg_row,
                                          const int* __restrict__ col, const VT* __restrict__ val, const double* __restrict__ x, long long ldx,
                                          double* __restrict__ y, long long ldy)
{
    const int4 b = blocks[blockIdx.x];  // (the XCD map of the window kernel was tried here: no difference on R-MAT)
    if (b.z == 64)
        er_bin<64, THREADS, ASSIGN, K, VT>(b.x, b.y, seg_ptr, seg_row, col, val, x, ldx, y, ldy);
    else if (b.z == 16)
        er_bin<16, THREADS, ASSIGN, K, VT>(b.x, b.y, seg_ptr, seg_row, col, val, x, ldx, y, ldy);
    else
        er_bin<4, THREADS, ASSIGN, K, VT>(b.x, b.y, seg_ptr, seg_row, col, val, x, ldx, y, ldy);
}

// ------------------------------------------------------------------ host side (ehyb_hip.hip)
namespace ehyb {
// (kSpmmMaxK, ell_win_cap, ell_lds_bytes and spmm_width are in ehyb_internal.h: the transcoder of the column words uses them too)
// The window launch of a multiply for k = 1..kSpmmMaxK columns ldx / ldy doubles apart.  walk: >= 0 explicit, -1 the plan's own
// alternation.  k = 1 only: stamps (diagnostic; no walk of its own) and xy_out (x . y on the side).
int launch_window(ehyb_plan* P, const double* x, long long ldx, double* y, long long ldy, int k, hipStream_t st, bool inl, int walk,
                  unsigned long long* stamps = nullptr, double* xy_out = nullptr);
// Both passes of the panel-form residual for k = 2..spmm_width columns (k = 1: the one-vector launch of ehyb_spmv)
int launch_panel_k(ehyb_plan* P, const double* x, long long ldx, double* y, long long ldy, int k, hipStream_t st, int walk);
// The CSR-segment residual launch for k columns (none where the plan has no CSR segments)
int launch_er_csr(ehyb_plan* P, const double* x, long long ldx, double* y, long long ldy, int k, hipStream_t st);
// The kernel arguments of a one-vector window launch that walks first to last: the device arrays, the window capacity, the item
// and XCD maps and the rule for which slabs are read with plain loads.  The transposed launch (ehyb_spmv_t.hip) takes the same.
EllArgs window_launch_args(ehyb_plan* P, const double* x, double* y);
}  // namespace ehyb
