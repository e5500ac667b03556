// Device pieces of the window kernel shared by its one-vector form (ehyb_hip.hip) and its k-vector form
// (ehyb_spmm.hip): the launch arguments, the item maps, the DPP lane shift and the value-pair load.
// Internal: nothing here is part of the C-ABI.
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
    // 1126 -> 1290 GFLOP/s (profiles/r04_nt_hints_ab.txt).  nt_slabs: the slabs at walk positions below nt_slabs/1024 of a segment are read
    // that way; the rest, the END of the walk, with plain loads -- what an alternating walk wants the Infinity Cache to keep for the next launch.
    int nt_slabs;
};

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

// Host side of a window launch (ehyb_hip.hip), shared with the k-vector launches
EllArgs ell_args(ehyb_plan* P, const double* x, double* y, unsigned long long* stamps, double* xy_out = nullptr);
// the walk direction and non-temporal share of a launch: walk >= 0 explicit, -1 the plan's own alternation (flips it)
void ell_walk(ehyb_plan* P, int walk, int n_items, size_t lds, EllArgs* A);
// ehyb_plan_upload: the k-vector window kernels (ehyb_spmm.hip) opt in to `lds` bytes of dynamic LDS
int spmm_set_lds_attr(int lds);

namespace ehyb {
// Doubles of the LDS x image per vector (the window, with symmetric pair storage the y accumulators behind it); the kernel's
// slab counter sits right behind the image(s).
inline int ell_win_cap(const HostLayout& H) { return (H.lds_doubles + 1) / 2 * 2; }

}  // namespace ehyb
