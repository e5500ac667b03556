// The two passes of the panel-form residual (host side: er_panel.cpp), device side, written once for NV = 1..4 columns
// (ehyb_hip.hip instantiates them: ehyb_pb_scale_kernel / ehyb_pb_reduce_kernel are NV = 1, ehyb_pb_scale_k_kernel /
// ehyb_pb_reduce_k_kernel NV = 2, 3, 4).  Column j of X and Y is ldx / ldy doubles behind column 0.  With NV columns the panel
// image is interleaved, win[c NV + j] = X[first + c + j ldx], and so are the partial sums, partial[slot NV + j]; values, column
// words, chunk records and jump lists are read once for all NV, and the decode of a chunk is done once for the NV products.
// Only NV = 1 has the LDS-sum arm (SUMS_DPP = false) and the timing probes (PROBE).  Internal: nothing here is part of the C-ABI.
// Steps of pass 1 are helpers as far as the K-wide kernels keep their instruction stream with them: the queue protocol and the
// K-wide staging are written out in pb_scale_body, because as helpers -- although inlined -- they reordered every K-wide kernel
// (profiles/r07_panel_refactor_isa.txt).  The helpers take plain pointers: __restrict__ on a parameter changed more than the order.
#pragma once
#include <hip/hip_runtime.h>

#include "ehyb_internal.h"
#include "ell_device.h"  // xcd_item

// ------------------------------------------------------------------ NV doubles side by side
// The NV values of one column in the interleaved panel image, the NV partial sums of one slot, the NV accumulators of one row:
// 16-byte accesses where the address allows (NV = 2, 4: base 16-byte aligned, index a multiple of 2), plain doubles for NV = 1, 3.
// (NT: streamed past the caches)
template <int NV, bool NT = false>
__device__ __forceinline__ void get_n(const double* p, double (&o)[NV])
{
    if constexpr (NV == 2 || NV == 4) {
        typedef double dbl2 __attribute__((ext_vector_type(2)));
        const dbl2* p2 = reinterpret_cast<const dbl2*>(p);
#pragma unroll
        for (int h = 0; h < NV / 2; ++h) {
            const dbl2 t = NT ? __builtin_nontemporal_load(p2 + h) : p2[h];
            o[2 * h] = t.x, o[2 * h + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int n = 0; n < NV; ++n) o[n] = NT ? __builtin_nontemporal_load(p + n) : p[n];
    }
}

template <int NV>
__device__ __forceinline__ void put_n(double* p, const double (&v)[NV])
{
    if constexpr (NV == 2 || NV == 4) {
        typedef double dbl2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int h = 0; h < NV / 2; ++h) {
            const dbl2 t = {v[2 * h], v[2 * h + 1]};
            reinterpret_cast<dbl2*>(p)[h] = t;
        }
    } else {
#pragma unroll
        for (int n = 0; n < NV; ++n) p[n] = v[n];
    }
}

// ------------------------------------------------------------------ pass 1: the sums of a chunk's pieces
// Pass 1: one workgroup per unit {first column, columns, first entry, end entry}.  The unit's panel of
// x is staged in LDS; (value, 16-bit column word) are streamed, eight 64-entry chunks per wave and step.
// The column word carries two flags from which a lane works out the slot of its partial (er_panel.cpp,
// encode_panel_slots): bit 15 = first entry of a piece (entries of one row that are neighbours in the
// chunk), bit 14 = the piece's slot is not the previous piece's + 1: a "jump", with an entry in the jump list
// from which every lane behind it (up to the next jump) gets its slot by adding the pieces begun before its own.
// The products of a piece are summed in registers and its last lane stores the partial.
// One step of a segmented inclusive scan over the 64 lanes of a wave, in registers (DPP moves, no LDS): every lane takes
// (sum, flag) of the lane CTRL names -- row_shr:d inside the rows of 16 lanes, row_bcast15 / row_bcast31 across them --
// and adds the sum unless a piece has begun between that lane and itself (flag).  Lanes without a source read zeros.
// The flags, and with them every branch, belong to the chunk and are worked out once; only the sums are per column.  (The
// flag's move goes first: behind the lo / hi moves the K-wide kernels grow by 70-180 instructions.)
template <int CTRL, int ROW_MASK, int NV>
__device__ __forceinline__ void seg_scan_step_n(double (&v)[NV], uint32_t& f)
{
    const uint32_t fp = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)f, CTRL, ROW_MASK, 0xf, true);
#pragma unroll
    for (int n = 0; n < NV; ++n) {
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v[n]), CTRL, ROW_MASK, 0xf, true);
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v[n]), CTRL, ROW_MASK, 0xf, true);
        v[n] += f ? 0.0 : __hiloint2double(hi, lo);
    }
    f |= fp;
}

template <int CTRL, int ROW_MASK, int NV>
__device__ __forceinline__ void wave_sum_step_n(double (&v)[NV])
{
#pragma unroll
    for (int n = 0; n < NV; ++n)
        v[n] += __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v[n]), CTRL, ROW_MASK, 0xf, true),
                                 __builtin_amdgcn_update_dpp(0, __double2loint(v[n]), CTRL, ROW_MASK, 0xf, true));
}

// Sums of the pieces of one 64-entry chunk: afterwards the LAST lane of every piece holds the piece's sums.  `heads` =
// ballot of the first lanes of the pieces (bit 0 always set).  Only the steps the chunk needs are run (wave-uniform
// branches on the ballot): none when every lane is its own piece -- most chunks of the sparse panels --, row_shr:1 alone
// when no piece is longer than two lanes, and so on; a hub row's 64-lane piece takes all six.
template <int NV>
__device__ __forceinline__ void piece_sums_n(double (&v)[NV], unsigned long long heads, bool head)
{
    const unsigned long long nh = ~heads;  // lanes that continue a piece
    if (nh == 0ull) return;
    if (heads == 1ull) {
        // the whole chunk is one piece -- a hub row in a hub panel, a third of the entries of a degree-ordered R-MAT: plain
        // sums over the wave, no flags to carry (half the instructions of the segmented steps); lane 63 holds them
        wave_sum_step_n<0x111, 0xf>(v);
        wave_sum_step_n<0x112, 0xf>(v);
        wave_sum_step_n<0x114, 0xf>(v);
        wave_sum_step_n<0x118, 0xf>(v);
        wave_sum_step_n<0x142, 0xa>(v);
        wave_sum_step_n<0x143, 0xc>(v);
        return;
    }
    uint32_t f = head ? 1u : 0u;
    seg_scan_step_n<0x111, 0xf>(v, f);  // row_shr:1
    const unsigned long long r2 = nh & (nh >> 1);
    if (r2 != 0ull) {  // a piece of three lanes or more
        seg_scan_step_n<0x112, 0xf>(v, f);  // row_shr:2
        const unsigned long long r4 = r2 & (r2 >> 2);
        if (r4 != 0ull) {  // five or more
            seg_scan_step_n<0x114, 0xf>(v, f);  // row_shr:4
            const unsigned long long r8 = r4 & (r4 >> 4);
            if (r8 != 0ull) seg_scan_step_n<0x118, 0xf>(v, f);  // nine or more: row_shr:8
        }
    }
    if (nh & 0x0001000100010000ull) {  // a piece crosses from one row of 16 lanes into the next
        seg_scan_step_n<0x142, 0xa>(v, f);  // row_bcast15: lane 15 -> row 1, lane 47 -> row 3
        seg_scan_step_n<0x143, 0xc>(v, f);  // row_bcast31: lane 31 -> rows 2 and 3
    }
}

// The LDS-sum arm (SUMS_DPP = false, cfg.er_sums = 2; one vector only): some lanes share a slot, so the piece sums are formed
// in this wave's 64 LDS words `scr` (zero between uses), one ds_add_f64 per lane, one read + one store of zero per piece.
// -> the piece's sum in its first lane (`stores`), the lane's own product elsewhere.  (Shuffle trees -- six ds_bpermute
// rounds per chunk -- cost 17 us of a 127 us launch here and 17 of 80 in pass 2.)
__device__ __forceinline__ double pb_lds_piece_sum(double* scr, uint32_t piece, bool stores, double prod)
{
    double sum = prod;
    unsafeAtomicAdd(&scr[piece], prod);
    if (stores) sum = scr[piece];
    __builtin_amdgcn_wave_barrier();
    scr[piece] = 0.0;
    return sum;
}

// ------------------------------------------------------------------ pass 1: items
// An ITEM = a run of units of (nearly) equal total cost, cut by the host (er_panel.cpp); every unit is a stretch of one
// panel's entries and stages that panel once.
// queue == null: one workgroup per item (workgroup b takes item xcd_item(b) / b).
// queue != null (cfg.er_queue = 1, an A/B arm -- see DESIGN.md 3.2): one RESIDENT round of workgroups, each taking items until none is left.  The
// hardware deals workgroups to the 8 XCDs round robin, so with one item per workgroup every XCD gets an eighth of the
// work whatever its speed -- and two of the eight XCDs of every box measured stream 8-12 % slower than the fastest, which
// the whole launch then waits for.  Here XCD k's workgroups take the items of the k-th contiguous eighth (queue[16 k] =
// items taken: the units of one panel still meet in one L2), and a workgroup whose own eighth is used up takes from the
// eighth with the most items left.  Exit: every workgroup leaves when every queue is empty (counts only grow); the last
// one to leave (queue[128] = workgroups gone) zeroes the counts for the next launch.
// the last workgroup to leave re-arms the queues for the next launch
__device__ __forceinline__ void pb_queue_leave(int* queue)
{
    if (queue != nullptr && threadIdx.x == 0 && atomicAdd(&queue[128], 1) == (int)gridDim.x - 1) {
        for (int k = 0; k < 8; ++k) __hip_atomic_store(&queue[16 * k], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&queue[128], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------ pass 1: staging a panel
// All of a thread's loads in flight before the first store (a 64 KiB panel is 16 double2 loads per thread; one load per loop
// trip would pay the memory latency 16 times).
// One vector: `cols` columns from xp (panels start on even columns: 16-byte loads).
template <int THREADS>
__device__ __forceinline__ void pb_stage_panel(double* win, const double* xp, int cols)
{
    const double2* __restrict__ xp2 = reinterpret_cast<const double2*>(xp);
    double2* win2 = reinterpret_cast<double2*>(win);
    const int n2 = cols >> 1;
    for (int i0 = 0; i0 < n2; i0 += 8 * THREADS) {
        double2 t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + j * THREADS + (int)threadIdx.x;
            t[j] = i < n2 ? xp2[i] : double2{0.0, 0.0};
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + j * THREADS + (int)threadIdx.x;
            if (i < n2) win2[i] = t[j];
        }
    }
    if ((cols & 1) && threadIdx.x == 0) win[cols - 1] = xp[cols - 1];
}

// ------------------------------------------------------------------ pass 1: a chunk's decode
// From a lane's column word `cw` and the chunk's jump entries (lane l holds the l-th in `jv`):
//   heads  ballot of the first lanes of the chunk's pieces
//   piece  the lane's piece, counted within the chunk
//   slot   where the lane stores its piece's partial sum; 0xFFFFFFFF: nothing to store (also what the padding piece yields).
//          Who stores: the piece's last lane (register scan) or its first (LDS sums); every lane of a piece computes the same slot.
//   flags  bit 0: every lane is its own piece, no sums needed; bit 1: this lane begins a piece
template <bool SUMS_DPP>
__device__ __forceinline__ void pb_decode_chunk(uint32_t cw, uint32_t jv, int lane, unsigned long long& heads, uint32_t& piece, uint32_t& slot, uint32_t& flags)
{
    const bool head = (cw & 0x8000u) != 0, jmp = (cw & 0x4000u) != 0;
    heads = __ballot(head);
    const unsigned long long jumps = __ballot(jmp);
    // pieces / jumps begun in the lanes below this one (v_mbcnt), plus its own
    const uint32_t hc = __builtin_amdgcn_mbcnt_hi((uint32_t)(heads >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)heads, 0u)) + (head ? 1u : 0u);
    const uint32_t jc = __builtin_amdgcn_mbcnt_hi((uint32_t)(jumps >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)jumps, 0u)) + (jmp ? 1u : 0u);
    // the entry of the last jump at or below this lane sits in lane jc - 1 (lane 0 is always a jump)
    const uint32_t base = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((jc - 1u) << 2), (int)jv);
    piece = hc - 1u;
    const bool stores = SUMS_DPP ? (lane == 63 || ((heads >> (lane + 1)) & 1ull)) : head;
    slot = stores ? base + hc - 1u : 0xFFFFFFFFu;
    flags = (heads == ~0ull ? 1u : 0u) | (head ? 2u : 0u);
}

// ------------------------------------------------------------------ pass 1
// SUMS_DPP (cfg.er_sums, the default): the products of a piece are added by the register scan above and the piece's
// LAST lane stores the partial; false = round 2's way: ds_add_f64 into 64 LDS words per wave, the FIRST lane reads the
// sum back and stores it (kept as the A/B arm: the LDS pipe of a CU was what bound pass 1 -- DESIGN.md 3.2).
// xcd_map: workgroup b takes unit xcd_item(b): the units of one panel (neighbours in the unit list) then run on ONE XCD at
// about the same time and stage their panel from its L2 instead of each from the fabric.
// PROBE: the timing-diagnostics instantiation (ehyb_debug_panel_times only); the product's own launches run PROBE = false,
// where every probe test folds away (they cost six vector instructions of ~70 per chunk).
// KCH = chunks per wave and step (8: 24 independent vector loads in flight per lane at 4 waves per SIMD).
// (Round 4 measured an instantiation for TWO 1024-thread workgroups per CU -- 9,728-column panels, KCH = 6, 59 VGPRs, 8 waves per SIMD, one
// workgroup staging while the other streams: R-MAT 2^22 140 against 132 us, 2^24 665 against 574 us, profiles/r04_d_panel_two_ab.jsonl -- the
// narrower panels' extra partial sums cost more than the occupancy gives; pass 1 alone ran level.  Removed again.)
// NV = columns of X per pass (ehyb_spmm); NV = 1 is the one-vector kernel.
template <int THREADS, bool SUMS_DPP, bool PROBE, int KCH, int NV = 1>
__device__ __forceinline__ void pb_scale_body(const int2* __restrict__ items, const int4* __restrict__ units, const double* __restrict__ val,
                                              const uint16_t* __restrict__ colf, const uint32_t* __restrict__ chunk, const uint32_t* __restrict__ jump,
                                              const double* __restrict__ x, double* __restrict__ partial, int panel_cols, int probe_arg, int xcd_map,
                                              int* __restrict__ queue, int n_items, int reverse, long long ldx = 0)
{
    static_assert(NV == 1 || (SUMS_DPP && !PROBE), "the K-wide pass 1 has register-scan sums and no probes");
    const int probe = PROBE ? probe_arg : 0;
    // probe (tools/panel_sweep.py, timing diagnostics only, results wrong): 1 no lane sums, 2 no stores,
    // 4 no LDS gather, 8 no panel staging
    extern __shared__ __attribute__((aligned(16))) double win[];
    constexpr int WAVES = THREADS / 64;
    // (the item handed from thread 0 to the workgroup: one word behind the panel and the piece accumulators, in the dynamic
    // allocation -- a static __shared__ word on top of a 160 KiB dynamic limit is refused by hipFuncSetAttribute)
    int& s_item = *reinterpret_cast<int*>(win + NV * panel_cols + (SUMS_DPP ? 0 : THREADS));
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* scr = win + panel_cols + 64 * wave;  // this wave's 64 piece accumulators, behind the panel (!SUMS_DPP only)
    if (!SUMS_DPP) scr[lane] = 0.0;
    int staged_x = -1, staged_n = -1;  // the panel in this workgroup's LDS (first column, columns): wave-uniform
    int my_q = 0;  // thread 0's queue: at first the XCD's own
    if (queue != nullptr && threadIdx.x == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        my_q = (int)(xcc & 7u);
    }
    for (;;) {
        int2 it;
        if (queue != nullptr) {
            __syncthreads();  // every wave is done with the previous item's panel, and with s_item
            if (threadIdx.x == 0) {  // takes the next item from the queues, its own first (my_q: the queue it is at); -1: none left anywhere
                int item = -1;
                for (;;) {
                    const int first = (int)((long long)n_items * my_q / 8), len = (int)((long long)n_items * (my_q + 1) / 8) - first;
                    const int idx = len > 0 ? atomicAdd(&queue[16 * my_q], 1) : len;
                    if (idx < len) {
                        item = reverse ? first + len - 1 - idx : first + idx;   // (alternating walk: every eighth from its far end)
                        break;
                    }
                    int best = -1, most = 0;  // own eighth used up: the one with the most items left
                    for (int k = 0; k < 8; ++k) {
                        const int lk = (int)((long long)n_items * (k + 1) / 8) - (int)((long long)n_items * k / 8);
                        const int left = lk - __hip_atomic_load(&queue[16 * k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (left > most) most = left, best = k;
                    }
                    if (best < 0) break;  // nothing left anywhere
                    my_q = best;
                }
                s_item = item;
            }
            __syncthreads();
            const int item = s_item;
            if (item < 0) break;
            it = items[item];
        } else {
            // reverse (successive launches alternate, as the ELL launch does): the items last to first, the units of an item last to
            // first, a unit's chunks last to first -- this launch starts with what the one before it left in the Infinity Cache
            const int idx = xcd_map ? xcd_item(blockIdx.x, gridDim.x) : (int)blockIdx.x;
            it = items[reverse ? (int)gridDim.x - 1 - idx : idx];
        }
        for (int ui = it.x; ui < it.y; ++ui) {
            const int un = reverse ? it.y - 1 - (ui - it.x) : ui;
            const int4 u = units[un];
            // the panel this workgroup staged last is still in its LDS: a unit of the same panel (the next stretch of a hub panel's
            // entries -- with the work queues a workgroup takes neighbouring items) streams straight away
            const bool staged_already = u.x == staged_x && u.y == staged_n;
            if (!staged_already && (ui != it.x || staged_n >= 0)) __syncthreads();  // every wave is done with the previous panel
            staged_x = u.x, staged_n = u.y;
            if constexpr (NV > 1) {
                // NV columns of X, interleaved: a thread takes the NV values of a column (each load coalesced along its own column of X,
                // which may start on an odd double: plain 8-byte loads) and stores them side by side
                if (!staged_already) {
                    constexpr int UN = NV == 2 ? 8 : 4;  // columns per thread and trip: 16 / 12 / 16 loads in flight
                    const double* __restrict__ xp = x + u.x;
                    for (int i0 = 0; i0 < u.y; i0 += UN * THREADS) {
                        double t[UN][NV];
#pragma unroll
                        for (int j = 0; j < UN; ++j) {
                            const int i = i0 + j * THREADS + (int)threadIdx.x;
#pragma unroll
                            for (int n = 0; n < NV; ++n) t[j][n] = i < u.y ? xp[i + n * ldx] : 0.0;
                        }
#pragma unroll
                        for (int j = 0; j < UN; ++j) {
                            const int i = i0 + j * THREADS + (int)threadIdx.x;
                            if (i < u.y) put_n<NV>(win + (size_t)i * NV, t[j]);
                        }
                    }
                }
            } else {
                if (!(probe & 8) && !staged_already) pb_stage_panel<THREADS>(win, x + u.x, u.y);  // (probe 8: no staging)
            }
            if (!staged_already) __syncthreads();
            const int c0 = u.z >> 6, c1 = u.w >> 6;  // chunks of 64 entries
            constexpr int K = KCH;  // chunks per wave and step: 24 independent vector loads in flight per lane at K = 8
            // The jump-list range of a chunk is known from the chunk records alone (wave-uniform, scalar loads): they are
            // fetched one step ahead, so that the jump entries travel together with the values and column words instead
            // of behind them (a gather that waits for the flags doubled the latency per step: 345 -> 470 us on R-MAT 2^24).
            uint32_t f0[K], fn[K];
            // the wave's steps: chunks c0 + K (wave + t WAVES) .., t = 0 .. steps - 1, walked up or down
            const int first = c0 + K * wave;
            const int steps = first < c1 ? (c1 - first + K * WAVES - 1) / (K * WAVES) : 0;
            const int dc = reverse ? -K * WAVES : K * WAVES;
            const int cstart = reverse ? first + (steps - 1) * K * WAVES : first;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int cj = max(c0, min(cstart + j, c1 - 1));
                f0[j] = chunk[cj];
                fn[j] = chunk[cj + 1] - f0[j];
            }
            int c = cstart;
            for (int t = 0; t < steps; ++t, c += dc) {
                double v[K];
                uint32_t cw[K], jv[K];
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const int cj = c + j < c1 ? c + j : c;  // wave-uniform
                    const size_t pos = (size_t)cj * 64 + lane;
                    // (streamed past the caches: every entry is read once per multiply, and what the caches hold instead -- the x panels the units of a
                    // hub panel stage again and again, the partial sums pass 2 is about to read -- is read again.  R-MAT 2^22: 128.0 -> 124.0 us)
                    v[j] = __builtin_nontemporal_load(&val[pos]);
                    cw[j] = __builtin_nontemporal_load(&colf[pos]);
                    jv[j] = (uint32_t)lane < fn[j] ? jump[f0[j] + lane] : 0u;  // lane l: the chunk's l-th jump entry
                }
                uint32_t g0[K], gn[K];  // the records of the next step
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const int cj = max(c0, min(c + dc + j, c1 - 1));
                    g0[j] = chunk[cj];
                    gn[j] = chunk[cj + 1] - g0[j];
                }
                uint32_t slot[K], piece[K];
                unsigned long long hd[K];
                double xw[K][NV];
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    uint32_t flags;
                    pb_decode_chunk<SUMS_DPP>(cw[j], jv[j], lane, hd[j], piece[j], slot[j], flags);
                    const uint32_t cl = cw[j] & 0x3FFFu;
                    if (probe & 4)
                        xw[j][0] = (double)cl;
                    else
                        get_n<NV>(win + cl * NV, xw[j]);
                    cw[j] = flags;
                }
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    if (c + j < c1) {  // wave-uniform
                        double sum[NV];
#pragma unroll
                        for (int n = 0; n < NV; ++n) sum[n] = v[j] * xw[j][n];
                        if (SUMS_DPP) {
                            if (!(probe & 1)) piece_sums_n<NV>(sum, hd[j], (cw[j] & 2u) != 0);
                        } else if (!(cw[j] & 1u) && !(probe & 1)) {
                            sum[0] = pb_lds_piece_sum(scr, piece[j], slot[j] != 0xFFFFFFFFu, sum[0]);
                        }
                        if (slot[j] != 0xFFFFFFFFu && (!(probe & 2) || sum[0] == 123.456)) {
                            if (probe & 256)
                                __builtin_nontemporal_store(sum[0], &partial[slot[j]]);
                            else
                                put_n<NV>(partial + (size_t)slot[j] * NV, sum);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < K; ++j) f0[j] = g0[j], fn[j] = gn[j];
            }
        }
        if (queue == nullptr) break;
    }
    pb_queue_leave(queue);
}

// ------------------------------------------------------------------ pass 2
// Pass 2: one workgroup per unit {first partial, end partial, first row, rows}.  The row block's
// accumulators live in LDS; (partial, 16-bit local row) are streamed and added (ds_add_f64); finally
// y[row] += accumulator for the rows that received something (the ELL launch has written y before) -- or,
// for a block of rows whose partitions have no window (rows < 0 in the unit), y[row] = accumulator for
// every row: the ELL launch leaves those rows alone.
// NT: the partial sums and their row words are streamed past the caches -- where they are more than the Infinity Cache can hold between the
// passes anyway (R-MAT 2^24: 460 MB; 520 -> 487 us with it, because the next multiply then finds more of the entry stream's tail there);
// where they fit (2^22: 89 MB) pass 2 reads them from that cache and the hint costs 3 us.
// The write-back of pass 2 for one column: the accumulators of the block's rows, NV doubles apart in LDS.
template <int THREADS, int NV>
__device__ __forceinline__ void pb_write_back(double* __restrict__ yp, const double* yacc, int rows, bool assign, int probe)
{
    constexpr int K = 8;
    // y[row] += accumulator for the rows that received something: the loads of a batch first, then the stores
    if (probe & 64) return;
    if (assign) {
        for (int i = threadIdx.x; i < rows; i += THREADS) yp[i] = yacc[i * NV];
        return;
    }
    for (int i0 = 0; i0 < rows; i0 += K * THREADS) {
        double a[K], yo[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int i = i0 + j * THREADS + (int)threadIdx.x;
            a[j] = i < rows ? yacc[i * NV] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int i = i0 + j * THREADS + (int)threadIdx.x;
            yo[j] = a[j] != 0.0 ? yp[i] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int i = i0 + j * THREADS + (int)threadIdx.x;
            if (a[j] != 0.0) yp[i] = yo[j] + a[j];
        }
    }
}

// NV columns (ehyb_spmm): partial[slot NV + j], accumulators yacc[row NV + j], one row word per slot for the NV adds; NV = 1 is the
// one-vector kernel (the only one with probes: the K-wide entry points pass 0).
template <int THREADS, bool NT, int NV>
__device__ __forceinline__ void pb_reduce_body(const int4* __restrict__ units, const double* __restrict__ partial, const uint16_t* __restrict__ row,
                                               double* __restrict__ y, long long ldy, int probe)
{
    // probe (timing diagnostics only): 16 no lane sums, 32 no LDS adds, 64 no write-back, 128 no zeroing
    extern __shared__ __attribute__((aligned(16))) double yacc[];
    int4 u = units[blockIdx.x];
    const bool assign = u.w < 0;  // the block is the only writer of its rows (partitions without a window): y = sum, zeros included
    u.w = assign ? -u.w : u.w;
    if (!(probe & 128))
        for (int i = threadIdx.x; i < u.w * NV; i += THREADS) yacc[i] = 0.0;
    __syncthreads();
    constexpr int KP = NV == 1 ? 8 : NV == 2 ? 4 : 2;  // partials per thread and step: 16 (12 for three columns) independent loads in flight
    // every wave runs the same number of steps (the shuffles need all 64 lanes)
    for (int base = u.x; base < u.y; base += KP * THREADS) {
        double v[KP][NV];
        uint32_t r[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const int i = base + j * THREADS + (int)threadIdx.x;
            const bool in = i < u.y;
            // (a lane past the end loads nothing with one vector; K wide it loads the unit's first partial sums -- in range: u.x < u.y
            // inside the loop -- and drops them)
            if (NV > 1 || in)
                get_n<NV, NT>(partial + (size_t)(in ? i : u.x) * NV, v[j]);
            else
                v[j][0] = 0.0;
            r[j] = in ? (uint32_t)(NT ? __builtin_nontemporal_load(&row[i]) : row[i]) : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            // (summing equal neighbouring rows across lanes first was measured: 17 us of an 80 us launch
            // for nothing -- the LDS adds serialise the few same-row neighbours by themselves)
            if (r[j] != 0xFFFFFFFFu && (!(probe & 32) || v[j][0] == 123.456)) {
#pragma unroll
                for (int n = 0; n < NV; ++n) unsafeAtomicAdd(&yacc[r[j] * NV + n], v[j][n]);  // ds_add_f64
            }
        }
    }
    __syncthreads();
    if constexpr (NV == 1) {
        pb_write_back<THREADS, 1>(y + u.z, yacc, u.w, assign, probe);
    } else {
#pragma unroll
        for (int n = 0; n < NV; ++n) pb_write_back<THREADS, NV>(y + u.z + n * ldy, yacc + n, u.w, assign, 0);
    }
}
