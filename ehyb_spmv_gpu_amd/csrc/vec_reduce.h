// Fixed-order reductions of the device-resident solvers.  A vector kernel writes one partial sum per workgroup (put_partial);
// the kernel that needs the scalar adds the partials of a slot up again (block_sum_n over partials_of) -- every workgroup for
// itself, in the same order, so every workgroup gets the same bits and a solve is reproducible run to run.  No atomics.
// Behind them: the per-column status words of the solvers that stop on the device.
#pragma once

#include <hip/hip_runtime.h>

namespace {

#ifndef EHYB_CG_THREADS
#define EHYB_CG_THREADS 256
#endif
constexpr int kThreads = EHYB_CG_THREADS;
constexpr int kMaxGrid = 1024;  // partial sums per dot product

// sum over the workgroup, returned to every thread; fixed order
__device__ __forceinline__ double block_sum(double v)
{
    __shared__ double part[kThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();  // a previous call's readers are done with part[]
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += part[w];
    return s;
}

__device__ __forceinline__ void put_partial(double v, double* __restrict__ part)
{
    const double s = block_sum(v);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// the sums of block_sum for N values at once: per value the same shuffle tree and the same order over the waves
template <int N>
__device__ __forceinline__ void block_sum_n(double (&v)[N])
{
    __shared__ double part[N][kThreads / 64];
#pragma unroll
    for (int c = 0; c < N; ++c) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_xor(v[c], off, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) part[c][threadIdx.x >> 6] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; ++c) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) s += part[c][w];
        v[c] = s;
    }
}

__device__ __forceinline__ double partials_of(const double* __restrict__ part)
{
    double v = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += kThreads) v += part[i];
    return v;
}

// slot `which` of column col, where a column has COUNT slots (the solver's A_COUNT or B_COUNT) of kMaxGrid partials
template <int COUNT, typename T>
__device__ __forceinline__ T* slot(T* s, int col, int which)
{
    return s + ((size_t)col * COUNT + which) * kMaxGrid;
}

// ------------------------------------------------------------------ the status of a column
// The solvers that stop on the device keep two ints per column: the status word and the device's iteration counter.  Where they
// live is the solver's business (ehyb_bicgstab_layout, ehyb_minres_layout, ehyb_gmres_layout); running and set_status take
// whatever yields column col's int* flags.
enum { F_STATUS = 0, F_ITERS = 1, F_COUNT = 2 };
enum { ST_RUNNING = 0, ST_CONVERGED = 1, ST_BREAKDOWN = 2 };

__device__ __forceinline__ bool usable_divisor(double d) { return d != 0.0 && isfinite(d); }
// a decision every thread of the workgroup takes alike (it comes from the status words, carried state or sums in the fixed
// order), as a scalar: the branches on it are not divergent
__device__ __forceinline__ bool uniform(bool b) { return __builtin_amdgcn_readfirstlane((int)b) != 0; }

// on[c]: column c0 + c was running when the workgroup entered, the same in every thread (a sibling workgroup of the launch may
// set a status).  -> any column running
template <int K, class FlagsOf>
__device__ __forceinline__ bool running(FlagsOf&& flags_of, int c0, bool (&on)[K])
{
    __shared__ int st[K];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) st[c] = __atomic_load_n(&flags_of(c0 + c)[F_STATUS], __ATOMIC_RELAXED);
    }
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = uniform(st[c] == ST_RUNNING);
        any = any || on[c];
    }
    return any;
}

template <class FlagsOf>
__device__ __forceinline__ void set_status(FlagsOf&& flags_of, int col, int status)
{
    if (threadIdx.x == 0) __atomic_store_n(&flags_of(col)[F_STATUS], status, __ATOMIC_RELAXED);
}

}  // namespace
