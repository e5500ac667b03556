// What ehyb_gmres.hip and ehyb_eigsh.hip share on the device: the slot and tail layout behind ehyb_gmres_layout, the small helpers
// of the pair walk, and the two tall-skinny kernels of the orthogonalisation -- dots (c_i = v_i . w for a growing basis) and update
// (w -= sum c_i v_i, the coefficients re-added from per-workgroup partials in a fixed order).  Each file that includes this header
// gets its own copy of the kernels (an unnamed namespace), compiled from the same text.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "ehyb_internal.h"
#include "solve_loop.h"

namespace {

constexpr int kM = EHYB_GMRES_MAX_RESTART;  // steps per cycle at most
constexpr int kCols = kM + 1;               // basis columns at most
constexpr int kGroup = 8;                   // basis columns per register group

// partial slots, kMaxGrid doubles each; c_i lives in slot G_C0 + i.  G_WW holds r.r after start and w.w after the last update.
enum { G_BB = 0, G_WW = 1, G_C0 = 2, G_COUNT = G_C0 + kCols };
// the tail, in doubles.  T_FLAGS: the ints status and counter; T_CYCLE: the int counter at the cycle start.
enum {
    T_FLAGS = 0,
    T_CYCLE = 1,
    T_RHO = 2,
    T_BB = 3,
    T_CS = 4,
    T_SN = T_CS + kM,
    T_GT = T_SN + kM,
    T_G = T_GT + kCols,
    T_H = T_G + kM,
    T_R = T_H + 2 * kCols,
    T_COUNT = T_R + kM * kM
};
// (the status word's F_* and ST_* values and uniform() are vec_reduce.h's, the same for every solver)

__device__ __forceinline__ double* gslot(double* s, int which) { return s + (size_t)which * kMaxGrid; }
__device__ __forceinline__ const double* gslot(const double* s, int which) { return s + (size_t)which * kMaxGrid; }

// the status as the workgroup found it on entry, the same in every thread (workgroup 0 of the launch may set it later)
__device__ __forceinline__ bool running(const double* tail)
{
    __shared__ int st;
    if (threadIdx.x == 0) st = __atomic_load_n(&((const int*)(tail + T_FLAGS))[F_STATUS], __ATOMIC_RELAXED);
    __syncthreads();
    return uniform(st == ST_RUNNING);
}

__device__ __forceinline__ double2 load2(const double* p) { return *reinterpret_cast<const double2*>(p); }
__device__ __forceinline__ void store2(double* p, double2 v) { *reinterpret_cast<double2*>(p) = v; }

// The kernels walk PAIRS of elements: pair p = (2p, 2p + 1) with p = block * 256 + thread, stride grid * 256, one 16-byte access
// per vector and pair; for an odd n the last element is a pair of one and goes through 8-byte accesses.

// one register group: columns g0 .. g0 + m - 1 (m <= 8; FULL: m = 8, no tests in the loop) against w
template <bool FULL>
__device__ __forceinline__ void dots_group(int n, size_t ld, const double* __restrict__ V, const double* __restrict__ w, int g0, int m,
                                           double* __restrict__ s)
{
    double acc[kGroup];
#pragma unroll
    for (int c = 0; c < kGroup; ++c) acc[c] = 0.0;
    const double* v0 = V + (size_t)g0 * ld;
    const int stride = (int)gridDim.x * kThreads;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        if (i + 1 < (size_t)n) {
            const double2 wv = load2(w + i);
            double2 vv[kGroup];
#pragma unroll
            for (int c = 0; c < kGroup; ++c)
                if (FULL || c < m) vv[c] = load2(v0 + (size_t)c * ld + i);
#pragma unroll
            for (int c = 0; c < kGroup; ++c)
                if (FULL || c < m) acc[c] = fma(vv[c].y, wv.y, fma(vv[c].x, wv.x, acc[c]));
        } else {
            const double wi = w[i];
#pragma unroll
            for (int c = 0; c < kGroup; ++c)
                if (FULL || c < m) acc[c] = fma(v0[(size_t)c * ld + i], wi, acc[c]);
        }
    }
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < kGroup; ++c)
            if (FULL || c < m) gslot(s, G_C0 + g0 + c)[blockIdx.x] = acc[c];
    }
}

// partials of c_i = v_i . w for i < cnt
__global__ __launch_bounds__(kThreads) void gmres_dots_kernel(int n, long long ld, const double* __restrict__ V, const double* __restrict__ w,
                                                              int cnt, double* __restrict__ s, const double* tail)
{
    if (!running(tail)) return;
    int g0 = 0;
    for (; g0 + kGroup <= cnt; g0 += kGroup) dots_group<true>(n, (size_t)ld, V, w, g0, kGroup, s);
    if (g0 < cnt) dots_group<false>(n, (size_t)ld, V, w, g0, cnt - g0, s);
}

// w -= sum_{i < cnt} c_i v_i with c_i re-added from the partials; workgroup 0: Hessenberg copy `pass` = copy pass - 1 + c
// (pass 0: c); last: the partials of w.w
__global__ __launch_bounds__(kThreads) void gmres_update_kernel(int n, long long ld_, const double* __restrict__ V, double* __restrict__ w,
                                                                int cnt, double* __restrict__ s, double* tail, int pass, int last)
{
    if (!running(tail)) return;
    __shared__ double c_sh[kCols + kGroup];
    for (int g0 = 0; g0 < cnt; g0 += kGroup) {
        double sums[kGroup];
#pragma unroll
        for (int c = 0; c < kGroup; ++c) sums[c] = g0 + c < cnt ? partials_of(gslot(s, G_C0 + g0 + c)) : 0.0;
        block_sum_n(sums);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < kGroup; ++c) c_sh[g0 + c] = sums[c];
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && (int)threadIdx.x < cnt) {
        const double c = c_sh[threadIdx.x];
        tail[T_H + pass * kCols + threadIdx.x] = pass > 0 ? tail[T_H + (pass - 1) * kCols + threadIdx.x] + c : c;
    }
    const size_t ld = (size_t)ld_;
    const int stride = (int)gridDim.x * kThreads;
    double ww = 0.0;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        if (i + 1 < (size_t)n) {
            double2 wv = load2(w + i);
            int c0 = 0;
            for (; c0 + kGroup <= cnt; c0 += kGroup) {
                double2 vv[kGroup];
#pragma unroll
                for (int c = 0; c < kGroup; ++c) vv[c] = load2(V + (size_t)(c0 + c) * ld + i);
#pragma unroll
                for (int c = 0; c < kGroup; ++c) {
                    const double ci = c_sh[c0 + c];
                    wv.x = fma(-ci, vv[c].x, wv.x);
                    wv.y = fma(-ci, vv[c].y, wv.y);
                }
            }
            for (; c0 < cnt; ++c0) {
                const double2 v = load2(V + (size_t)c0 * ld + i);
                const double ci = c_sh[c0];
                wv.x = fma(-ci, v.x, wv.x);
                wv.y = fma(-ci, v.y, wv.y);
            }
            store2(w + i, wv);
            ww = fma(wv.y, wv.y, fma(wv.x, wv.x, ww));
        } else {
            double wi = w[i];
            for (int c0 = 0; c0 < cnt; ++c0) wi = fma(-c_sh[c0], V[(size_t)c0 * ld + i], wi);
            w[i] = wi;
            ww = fma(wi, wi, ww);
        }
    }
    if (last) put_partial(ww, gslot(s, G_WW));
}

// ------------------------------------------------------------------ what a driver owns
struct DeviceArray {
    double* p = nullptr;
    ~DeviceArray()
    {
        if (p) (void)hipFree(p);
    }
};

struct CycleGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    ~CycleGraph()
    {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
    }
};

// ------------------------------------------------------------------ the *_step building blocks
constexpr int kStepGrid = kMaxGrid / 2;

inline double* step_tail(double* s) { return s + (size_t)G_COUNT * kMaxGrid; }

// the basis and the vectors walked in pairs: an even leading dimension >= n and 16-byte aligned pointers (NULL passes: the
// caller lists what it requires in check_step)
inline int check_pairs(const char* who, int n, int64_t ld, std::initializer_list<const void*> aligned)
{
    bool ok = ld >= n && (ld & 1) == 0;
    for (const void* a : aligned) ok = ok && ((uintptr_t)a & 15) == 0;
    if (!ok) EHYB_FAIL(EHYB_ERR_ARG, "%s: the leading dimension must be even and >= n, the vectors 16-byte aligned", who);
    return EHYB_OK;
}

}  // namespace
