// The TRANSPOSED multiply y = A^T x on the layout the forward kernels read (ehyb_spmv_t.hip instantiates these bodies): plain
// storage, fp64 values, one vector.  The LDS window of a partition -- own rows plus halo, the forward kernel's x image -- is a
// window of ACCUMULATORS here: a lane multiplies the entries of its row by x[row] and adds each product to the entry's window
// column (ds_add_f64); the window is then flushed to y with the fp64 global atomic add.  x is not staged at all, so the LDS
// budget is the forward launch's.  y must be zero on entry (the launch path zeroes it in-stream).
//
// Work items, segments, the item map and the rule for plain against non-temporal value loads are the forward launch's
// (EllArgs, item_of_block, ell_slab_resident: ell_device.h); the column words are decoded as ell_slab decodes them.  A
// partition cut into several segments (several work items) flushes one window per segment: every contribution to y is an atomic
// add, so nothing depends on who flushes first.  Internal: nothing here is part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "ell_device.h"

// value * x[row] into the two window columns of a pair; lanes without a row add nothing.
// Lanes of one group (equal column lists: the unknowns of a node) send their products to the SAME LDS word, which the hardware
// serialises.  They are summed across the lanes first with the next_lane DPP moves -- `code` bit 0: this lane adds, for itself
// and (bits 1, 2) for the next and the second next lane of its group; the other lanes of the three add nothing -- so a group of
// three costs one ds_add_f64 per column instead of three (the bench matrix with every entry stored: 148 -> 133 us per launch,
// profiles/spmv_t_group_sums_ab.jsonl).  Every lane of the wave takes part in the moves: the callers' loops are wave-uniform.
__device__ __forceinline__ void ell_t_pair(double* __restrict__ acc, const double2& v, uint32_t c_lo, uint32_t c_hi, double xi, bool has_row, int code)
{
    const double p0 = has_row ? v.x * xi : 0.0, p1 = has_row ? v.y * xi : 0.0;
    const double a1 = next_lane(p0), a2 = next_lane(a1), b1 = next_lane(p1), b2 = next_lane(b1);
    const double s0 = p0 + ((code & 2) ? a1 : 0.0) + ((code & 4) ? a2 : 0.0);
    const double s1 = p1 + ((code & 2) ? b1 : 0.0) + ((code & 4) ? b2 : 0.0);
    // (lanes without a row are the last of a slab: a lane that adds has a row if any of its three has)
    if (has_row && (code & 1)) {
        unsafeAtomicAdd(&acc[c_lo], s0);  // ds_add_f64
        unsafeAtomicAdd(&acc[c_hi], s1);
    }
}

// The lane's part in the sums of its group, from the group numbers of the slab's lanes (plain plans do not carry the codes that
// symmetric pair storage keeps in bits 6-7 of lane_group): runs of lanes with equal group are cut into threes from the run's
// first lane; bit 0 = first of its three, bit 1 / 2 = the next / second next lane belongs to the same run.
__device__ __forceinline__ int ell_t_group_code(uint32_t g, int lane)
{
    const int gn = __builtin_amdgcn_update_dpp(0, (int)g, 0x130 /* wave_shl:1: lane + 1's */, 0xf, 0xf, true);
    const unsigned long long ends = __ballot(lane == 63 || gn != (int)g);  // runs end at these lanes
    const unsigned long long starts = (ends << 1) | 1ull;
    const int first = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));  // the run's first lane (bit 0 is set)
    const bool same1 = !((ends >> lane) & 1ull);
    const bool same2 = same1 && !((ends >> (lane + 1)) & 1ull);  // (same1: lane < 63)
    return ((lane - first) % 3 == 0 ? 1 : 0) | (same1 ? 2 : 0) | (same2 ? 4 : 0);
}

// a product of the inline residual straight into y[global column]; an exact zero (padding: value 0.0, column 0) changes nothing
// in a y that started at zero and is left out, 0 * inf = NaN is not
__device__ __forceinline__ void ell_t_global(double* __restrict__ y, uint32_t col, double p)
{
    if (p != 0.0) unsafeAtomicAdd(&y[col], p);  // global_atomic_add_f64
}

// One slab of 64 rows: lane l holds row sm.z + l and scatters its entries.
template <bool INLINE_ER, bool NT>
__device__ __forceinline__ void ell_slab_t(const EllArgs& A, double* __restrict__ acc, int s, int base, int pe, int lane)
{
    // slab record {first value pair, first column word, first row, pairs << 16 | residual pairs << 8 | flags | groups - 1}
    const uint4 sm = A.slab_meta[s];
    const int np = (int)(sm.w >> 16);
    const int G = (int)(sm.w & 0x3fu) + 1;
    const double2* __restrict__ v = A.ell_val + (size_t)sm.x * 64 + lane;
    const uint32_t lgb = A.lane_group[(size_t)s * 64 + lane];
    const uint32_t* __restrict__ c = A.ell_col + sm.y + lgb;
    const int row = (int)sm.z + lane;
    const int lrow = row - base;
    const bool has_row = row < pe;
    const double xi = has_row ? A.x[row] : 0.0;  // coalesced, once per slab
    // relative columns differ from lane to lane of a group: every lane adds for itself there (bit 7 is wave-uniform)
    const int code = !(sm.w & 0x80u) ? ell_t_group_code(lgb, lane) : 1;
    if (INLINE_ER) {
        // `ner` more pairs behind the slab's ELL pairs, their columns global: [pair][2][lane] words behind the shared column words
        const int ner = (int)(sm.w >> 8) & 0xff;
        const double2* __restrict__ ve = v + (size_t)np * 64;
        const uint32_t* __restrict__ ce = A.ell_col + sm.y + (size_t)np * G + lane;
        for (int q = 0; q < ner; ++q) {
            const double2 vv = ve[q * 64];
            const uint32_t ca = ce[q * 128], cb = ce[q * 128 + 64];
            if (has_row) {
                ell_t_global(A.y, ca, vv.x * xi);
                ell_t_global(A.y, cb, vv.y * xi);
            }
        }
    }
    if (sm.w & 0x40u) {
        // triple-coded column words (device copy only, col_triples.h): one word (A, B) per three pairs, columns (A, A+1),
        // (A+2, B), (B+1, B+2); the last word of a slab may stand for one or two pairs.  Never relative.
        const double2* vp = v;
        const uint32_t* cp = c;
        int left = np;
#pragma nounroll
        for (; left >= 3; left -= 3, vp += 3 * 64, cp += G) {
            const double2 v0 = ell_load_pair<NT>(vp), v1 = ell_load_pair<NT>(vp + 64), v2 = ell_load_pair<NT>(vp + 2 * 64);
            const uint32_t w = cp[0], a = w & 0xffffu, b = w >> 16;
            ell_t_pair(acc, v0, a, a + 1, xi, has_row, code);
            ell_t_pair(acc, v1, a + 2, b, xi, has_row, code);
            ell_t_pair(acc, v2, b + 1, b + 2, xi, has_row, code);
        }
        if (left > 0) {  // (wave-uniform, as `left > 1`)
            const double2 v0 = ell_load_pair<NT>(vp);
            double2 v1 = make_double2(0.0, 0.0);
            if (left > 1) v1 = ell_load_pair<NT>(vp + 64);
            const uint32_t w = cp[0], a = w & 0xffffu, b = w >> 16;
            ell_t_pair(acc, v0, a, a + 1, xi, has_row, code);
            if (left > 1) ell_t_pair(acc, v1, a + 2, b, xi, has_row, code);
        }
    } else {
        // pair form: one word = two 16-bit window columns; bit 7 of the record: relative to the lane's own row
        const uint32_t radd = (sm.w & 0x80u) ? (uint32_t)lrow : 0u;
        int k = 0;
#pragma nounroll
        for (; k + 4 <= np; k += 4) {
            double2 vv[4];
            uint32_t cc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) vv[q] = ell_load_pair<NT>(v + (k + q) * 64);
#pragma unroll
            for (int q = 0; q < 4; ++q) cc[q] = c[(k + q) * G];
#pragma unroll
            for (int q = 0; q < 4; ++q) ell_t_pair(acc, vv[q], ((cc[q] & 0xffffu) + radd) & 0xffffu, ((cc[q] >> 16) + radd) & 0xffffu, xi, has_row, code);
        }
        for (; k < np; ++k) {
            const double2 v0 = ell_load_pair<NT>(v + k * 64);
            const uint32_t c0 = c[k * G];
            ell_t_pair(acc, v0, ((c0 & 0xffffu) + radd) & 0xffffu, ((c0 >> 16) + radd) & 0xffffu, xi, has_row, code);
        }
    }
}

// Segment g: zero the window's accumulators, scatter the segment's slabs into them, flush them to y.
template <int THREADS, bool INLINE_ER>
__device__ __forceinline__ void ell_segment_t(const EllArgs& A, double* __restrict__ acc, int* __restrict__ next_slab, int g, int lane, int wave)
{
    constexpr int WAVES = THREADS / 64;
    const int4 a = A.segs[2 * g], b = A.segs[2 * g + 1];
    const int sb = a.y, se = a.z, hn = a.w;
    const int ps = b.x, pe = b.y, wl = b.z, hb = b.w;
    if (wl == 0 && hn == 0) return;  // a partition without a window: its rows are the residual's
    __syncthreads();  // every wave is done with the previous window and counter
    // acc[i] stands for column base + i, i < cnt; acc[cnt + i] for halo_cols[hb + i].  acc[0] of an odd-start partition is row
    // ps - 1, which is not the partition's: padding slots (value 0.0, column 0) land there, and it is never flushed.
    const int base = ps & ~1, cnt = wl + (ps & 1);
    for (int i = threadIdx.x; i < cnt + hn; i += THREADS) acc[i] = 0.0;
    if (threadIdx.x == 0) *next_slab = sb + WAVES;  // slabs sb..sb+WAVES-1 are pre-assigned
    __syncthreads();
    int s = sb + wave;
    while (s < se) {
        if (ell_slab_resident(s - sb, se - sb, A.keep1024, A.keep_shape))
            ell_slab_t<INLINE_ER, false>(A, acc, s, base, pe, lane);
        else
            ell_slab_t<INLINE_ER, true>(A, acc, s, base, pe, lane);  // value stream past the caches
        int nx = 0;
        if (lane == 0) nx = atomicAdd(next_slab, 1);
        s = __builtin_amdgcn_readfirstlane(nx);
    }
    __syncthreads();  // every add of the segment is in
    // (an exact zero adds nothing to a y that started at zero)
    for (int i = threadIdx.x + (ps & 1); i < cnt; i += THREADS) {
        const double t = acc[i];
        if (t != 0.0) unsafeAtomicAdd(&A.y[base + i], t);
    }
    for (int i = threadIdx.x; i < hn; i += THREADS) {
        const double t = acc[cnt + i];
        if (t != 0.0) unsafeAtomicAdd(&A.y[A.halo_cols[hb + i]], t);
    }
}

// One workgroup per work item, its segments one after the other; the LDS slab counter sits right behind the window.
template <int THREADS, bool INLINE_ER>
__device__ __forceinline__ void ell_items_t(const EllArgs& A)
{
    extern __shared__ __attribute__((aligned(16))) double win[];
    int* next_slab = reinterpret_cast<int*>(win + A.win_cap);
    const int4 it = A.items[2 * item_of_block(A.item_map, A.xcd_map)];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int sg = it.x; sg < it.y; ++sg) ell_segment_t<THREADS, INLINE_ER>(A, win, next_slab, sg, lane, wave);
}

// ------------------------------------------------------------------ residual segments, transposed
// The descriptors, bins and lanes per segment of er_bin: G lanes walk a segment's (column, value) entries strided and coalesced,
// and each adds value * x[row] to y[column].  Split rows need nothing special: a segment only READS its row's x.
template <int G, int THREADS>
__device__ __forceinline__ void er_bin_t(int lo, int hi, const int64_t* __restrict__ seg_ptr, const int* __restrict__ seg_row,
                                         const int* __restrict__ col, const double* __restrict__ val, const double* __restrict__ x,
                                         double* __restrict__ y)
{
    constexpr int SEGS = THREADS / G;
    const int sub = threadIdx.x % G;
    for (int base = lo; base < hi; base += SEGS) {
        const int seg = base + threadIdx.x / G;
        if (seg >= hi) continue;
        const int64_t b = seg_ptr[seg], e = seg_ptr[seg + 1];
        const double xi = x[seg_row[seg] & 0x7fffffff];
        int64_t k = b + sub;
        for (; k + 3 * G < e; k += 4 * G) {  // four entries of a lane requested before the first add
            const int c0 = col[k], c1 = col[k + G], c2 = col[k + 2 * G], c3 = col[k + 3 * G];
            const double v0 = val[k], v1 = val[k + G], v2 = val[k + 2 * G], v3 = val[k + 3 * G];
            unsafeAtomicAdd(&y[c0], v0 * xi);
            unsafeAtomicAdd(&y[c1], v1 * xi);
            unsafeAtomicAdd(&y[c2], v2 * xi);
            unsafeAtomicAdd(&y[c3], v3 * xi);
        }
        for (; k < e; k += G) unsafeAtomicAdd(&y[col[k]], val[k] * xi);
    }
}

template <int THREADS>
__device__ __forceinline__ void er_blocks_t(const int4* __restrict__ blocks, const int64_t* __restrict__ seg_ptr, const int* __restrict__ seg_row,
                                            const int* __restrict__ col, const double* __restrict__ val, const double* __restrict__ x,
                                            double* __restrict__ y)
{
    const int4 b = blocks[blockIdx.x];
    if (b.z == 64)
        er_bin_t<64, THREADS>(b.x, b.y, seg_ptr, seg_row, col, val, x, y);
    else if (b.z == 16)
        er_bin_t<16, THREADS>(b.x, b.y, seg_ptr, seg_row, col, val, x, y);
    else
        er_bin_t<4, THREADS>(b.x, b.y, seg_ptr, seg_row, col, val, x, y);
}
