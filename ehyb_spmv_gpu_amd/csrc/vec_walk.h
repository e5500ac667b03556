// The index walk of the K-column vector kernels of the device-resident solvers (their sums and status words: vec_reduce.h).
#pragma once

#include <hip/hip_runtime.h>

#include "vec_reduce.h"

namespace {

// One thread serves K columns at index i = block * kThreads + thread, i + stride, ... (stride = grid * kThreads): trips of U
// strides while a whole trip fits below n, then single strides -- the same trip at U = 1, so a kernel states its loads and its
// arithmetic once.  A thread meets its indices in rising order whatever U is, and a trip takes its columns in order and a
// column's strides in order: a sum a kernel accumulates per column (fma into one accumulator per use) has the same bits for
// every U and every K, so U is free per kernel and per K and is chosen to keep the loads of a trip in registers.
//
// Every load of a trip is issued before its first store: first what the columns share at an index (shared(i): one value of
// any type, InvDiag's 1/diag for most kernels), then load(c, i, in, sh) for every live column and stride, which fills in[NV], the
// kernel's inputs at one (column, index); only then use(c, i, in, sh) does the arithmetic and the stores.  A kernel may
// therefore write a vector it reads.  A column with live[c] false is skipped.
template <int K, int U, int NV, class Shared, class Load, class Use>
__device__ __forceinline__ void walk_trip(int i, int stride, const bool (&live)[K], Shared&& shared, Load&& load, Use&& use)
{
    decltype(shared(0)) sh[U];
    double in[K][U][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) sh[u] = shared(i + u * stride);
#pragma unroll
    for (int c = 0; c < K; ++c) {
        if (!live[c]) continue;
#pragma unroll
        for (int u = 0; u < U; ++u) load(c, i + u * stride, in[c][u], sh[u]);
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        if (!live[c]) continue;
#pragma unroll
        for (int u = 0; u < U; ++u) use(c, i + u * stride, in[c][u], sh[u]);
    }
}

template <int K, int U, int NV, class Shared, class Load, class Use>
__device__ __forceinline__ void walk(int n, const bool (&live)[K], Shared&& shared, Load&& load, Use&& use)
{
    const int stride = (int)gridDim.x * kThreads;
    int i = blockIdx.x * kThreads + threadIdx.x;
    for (; i + (U - 1) * stride < n; i += U * stride) walk_trip<K, U, NV>(i, stride, live, shared, load, use);
    if constexpr (U > 1) {
        for (; i < n; i += stride) walk_trip<K, 1, NV>(i, stride, live, shared, load, use);
    }
}

// U of the kernels that do not choose one per K (CG, Chebyshev, coarse, FSAI, refine)
constexpr int kWalkU = 4;

// shared(i) of the kernels that apply the diagonal preconditioner: 1/diag at i.  Without one (dinv null) the kernels do not
// multiply -- they branch on dinv themselves -- and the 1.0 is never used.
struct InvDiag {
    const double* __restrict__ dinv;
    __device__ __forceinline__ double operator()(int i) const { return dinv ? dinv[i] : 1.0; }
};
// ... and of the kernels whose columns share nothing
struct NoShared {
    __device__ __forceinline__ int operator()(int) const { return 0; }
};

}  // namespace
