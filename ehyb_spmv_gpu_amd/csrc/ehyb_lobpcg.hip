// LOBPCG for the nev smallest eigenpairs of the plan's symmetric matrix (ehyb_lobpcg): a block of nb vectors X, their
// preconditioned residuals W and the previous directions P span the trial space S = [X | P | W] of at most 24 columns; the host
// solves the projected problem S^T A S y = theta S^T S y (ehyb_lobpcg_rr) and the device rotates S and A S into the next X and P.
// The multiplies are ehyb_spmm, the rotation is the kernel of ehyb_eigsh_rotate_step, the preconditioner is ehyb_coarse_apply,
// inv_diag or nothing.  New here: the Gram kernel, the residual kernel and their fixed-order sums.
//
// The Gram kernel.  [G | H] = S^T [S | AS] has at most 24 x 48 entries and n terms each: it is cut into 8 x 8 blocks, of which
// the upper triangle holds at most 6 per matrix, and ONE WAVE of a workgroup of twelve owns one block for the whole launch, its
// 64 sums in registers (lane l adds rows l and l + 64 of every tile).  A workgroup walks tiles of 128 rows: all twelve waves
// copy the 2 mc columns of the tile into LDS with 16-byte loads -- each column leaves HBM once -- and every wave then reads its
// 8 + 8 columns from LDS.  The loads of the next tile are in flight while the blocks of this one are summed.  At the end a wave
// adds its lanes with the shuffle tree and lane 0 writes the block's entries of the upper triangle into the workgroup's own
// slot; a second launch adds the slots in rising order and mirrors the triangle.  No atomics, no "last workgroup".
//
// ehyb_lobpcg_gen is the same driver for the pencil K x = lambda M x: a third image BS = M S beside S and AS (stored and rotated
// for a mass plan, formed as m o s inside the kernels for a lumped mass), G = S^T BS, R = AX - theta BX.  Without a mass the driver
// launches the kernels above and nothing else.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "coarse.h"
#include "ehyb_internal.h"
#include "gmres_device.h"
#include "solve_loop.h"

using namespace ehyb;

namespace {

constexpr int kBlock = EHYB_LOBPCG_MAX_BLOCK;  // vectors in X at most
constexpr int kS = 3 * kBlock;                 // columns of S at most
constexpr int kGramWaves = 12;                 // six blocks of the upper triangle for G, six for H
constexpr int kGramThreads = 64 * kGramWaves;
constexpr int kGramRows = 128;                 // rows of a tile: one pair per lane and column
constexpr int kGramGrid = 256;                 // workgroups at most: one per CU
constexpr int kGramSlot = 2 * kS * kS;         // doubles of a workgroup's slot: G, then H, column-major with leading dimension 24
static_assert(kGramGrid * kGramSlot == EHYB_LOBPCG_SCRATCH_DOUBLES, "the header states the scratch of ehyb_lobpcg_gram_step");
static_assert(kBlock == kGroup, "a register group is a block of X");

// block b of the upper triangle, (0,0) (0,1) (1,1) (0,2) (1,2) (2,2): g column groups use the first g (g + 1) / 2
__device__ const int kBlockI[6] = {0, 0, 1, 0, 1, 2};
__device__ const int kBlockJ[6] = {0, 1, 1, 2, 2, 2};

inline int gram_grid(int n) { return std::max(1, std::min((n + kGramRows - 1) / kGramRows, kGramGrid)); }

__global__ __launch_bounds__(kGramThreads) void lobpcg_gram_kernel(int n, long long ld_, const double* __restrict__ S,
                                                                   const double* __restrict__ AS, int mc, double* __restrict__ part)
{
    // column q < 24 of the tile is column q of S, column 24 + q column q of AS; columns >= mc stay zero
    __shared__ __attribute__((aligned(16))) double tile[2 * kS * kGramRows];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = threadIdx.x; k < 2 * kS * kGramRows; k += kGramThreads) tile[k] = 0.0;
    const int groups = (mc + kGroup - 1) / kGroup;
    const int b = wave % 6;
    const bool is_h = wave >= 6, active = b < groups * (groups + 1) / 2;
    const int gi = kBlockI[b], gj = kBlockJ[b];
    const double* a_sh = tile + (size_t)gi * kGroup * kGramRows;
    const double* b_sh = tile + (size_t)((is_h ? kS : 0) + gj * kGroup) * kGramRows;
    const size_t ld = (size_t)ld_;
    const long long tiles = ((long long)n + kGramRows - 1) / kGramRows;

    // a wave copies columns wave, wave + 12, wave + 24, wave + 36 of the tile, lane l the pair (2l, 2l + 1) of each
    double2 pre[4];
    auto fetch = [&](long long t) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = wave + kGramWaves * k, c = q < kS ? q : q - kS;
            if (c >= mc) continue;
            const double* col = (q < kS ? S : AS) + (size_t)c * ld;
            const long long i = t * kGramRows + 2 * lane;
            if (i + 1 < n)
                pre[k] = load2(col + i);
            else
                pre[k] = {i < n ? col[i] : 0.0, 0.0};
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = wave + kGramWaves * k, c = q < kS ? q : q - kS;
            if (c < mc) store2(tile + (size_t)q * kGramRows + 2 * lane, pre[k]);
        }
    };

    double acc[kGroup][kGroup];
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
#pragma unroll
        for (int j = 0; j < kGroup; ++j) acc[i][j] = 0.0;
    }
    long long t = blockIdx.x;
    if (t < tiles) fetch(t);
    __syncthreads();  // the zeros are in place
    for (; t < tiles; t += gridDim.x) {
        put();
        __syncthreads();
        if (t + gridDim.x < tiles) fetch(t + gridDim.x);
        if (active) {
#pragma unroll 1  // 64 sums fill the registers of a wave that shares its SIMD with two more
            for (int r = lane; r < kGramRows; r += 64) {
                double a[kGroup];
#pragma unroll
                for (int i = 0; i < kGroup; ++i) a[i] = a_sh[i * kGramRows + r];
#pragma unroll
                for (int j = 0; j < kGroup; ++j) {
                    const double bj = b_sh[j * kGramRows + r];
#pragma unroll
                    for (int i = 0; i < kGroup; ++i) acc[i][j] = fma(a[i], bj, acc[i][j]);
                }
            }
        }
        __syncthreads();  // the tile is free
    }
    if (!active) return;
    double* slot = part + (size_t)blockIdx.x * kGramSlot + (is_h ? kS * kS : 0);
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            double v = acc[i][j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            const int I = gi * kGroup + i, J = gj * kGroup + j;
            if (lane == 0 && I <= J && J < mc) slot[I + J * kS] = v;
        }
    }
}

// G[i, j] = G[j, i] = the slots' entry (i, j), i <= j, added in rising order of the workgroups; H likewise.  One thread per entry.
__global__ __launch_bounds__(kThreads) void lobpcg_gram_sum_kernel(const double* __restrict__ part, int grid, int mc, double* __restrict__ G,
                                                                   double* __restrict__ H)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= 2 * mc * mc) return;
    const int m = e / (mc * mc), r = e - m * mc * mc, i = r % mc, j = r / mc;
    if (i > j) return;
    const double* p = part + (m ? kS * kS : 0) + i + j * kS;
    double s = 0.0;
#pragma unroll 8
    for (int w = 0; w < grid; ++w) s += p[(size_t)w * kGramSlot];
    double* out = m ? H : G;
    out[i + (size_t)j * mc] = s;
    out[j + (size_t)i * mc] = s;
}

// R_c = AX_c - theta_c X_c for c < nb; the partials of R_c . R_c into part[workgroup * 8 + c]; for every c in the mask
// W[:, position of c among the mask's bits] = dinv o R_c (dinv NULL: R_c).  Pairs as the kernels of gmres_device.h.
__global__ __launch_bounds__(kThreads) void lobpcg_resid_kernel(int n, long long ld_, const double* __restrict__ X,
                                                                const double* __restrict__ AX, int nb, const double* __restrict__ theta,
                                                                const double* __restrict__ dinv, unsigned mask, long long ldw_, double* W,
                                                                double* __restrict__ part)
{
    __shared__ double th[kBlock];
    if (threadIdx.x < kBlock) th[threadIdx.x] = (int)threadIdx.x < nb ? theta[threadIdx.x] : 0.0;
    __syncthreads();
    double acc[kBlock];
#pragma unroll
    for (int c = 0; c < kBlock; ++c) acc[c] = 0.0;
    const size_t ld = (size_t)ld_, ldw = (size_t)ldw_;
    const int stride = (int)gridDim.x * kThreads;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        const bool pair = i + 1 < (size_t)n;
        double2 d = {1.0, 1.0};
        if (dinv && mask) d = pair ? load2(dinv + i) : double2{dinv[i], 1.0};
#pragma unroll
        for (int c = 0; c < kBlock; ++c) {
            if (c >= nb) break;
            double2 x, ax;
            if (pair) {
                x = load2(X + (size_t)c * ld + i);
                ax = load2(AX + (size_t)c * ld + i);
            } else {
                x = {X[(size_t)c * ld + i], 0.0};
                ax = {AX[(size_t)c * ld + i], 0.0};
            }
            double2 r;
            r.x = fma(-th[c], x.x, ax.x);
            r.y = fma(-th[c], x.y, ax.y);
            acc[c] = fma(r.y, r.y, fma(r.x, r.x, acc[c]));
            if (mask >> c & 1u) {
                double* w = W + (size_t)__popc(mask & ((1u << c) - 1u)) * ldw + i;
                if (dinv) {
                    r.x *= d.x;
                    r.y *= d.y;
                }
                if (pair)
                    store2(w, r);
                else
                    *w = r.x;
            }
        }
    }
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < kBlock; ++c) part[(size_t)blockIdx.x * kBlock + c] = acc[c];
    }
}

// out[c] = the workgroups' partials of column c added in rising order
__global__ __launch_bounds__(64) void lobpcg_resid_sum_kernel(const double* __restrict__ part, int grid, int nb, double* __restrict__ out)
{
    const int c = threadIdx.x;
    if (c >= nb) return;
    double s = 0.0;
#pragma unroll 8
    for (int w = 0; w < grid; ++w) s += part[(size_t)w * kBlock + c];
    out[c] = s;
}

void launch_gram(int n, long long ld, const double* S, const double* AS, int mc, double* G, double* H, double* part, hipStream_t st)
{
    const int grid = gram_grid(n);
    hipLaunchKernelGGL(lobpcg_gram_kernel, dim3(grid), dim3(kGramThreads), 0, st, n, ld, S, AS, mc, part);
    hipLaunchKernelGGL(lobpcg_gram_sum_kernel, dim3((2 * mc * mc + kThreads - 1) / kThreads), dim3(kThreads), 0, st, part, grid, mc, G, H);
}

void launch_resid(int grid, int n, long long ld, const double* X, const double* AX, int nb, const double* theta, const double* dinv,
                  unsigned mask, long long ldw, double* W, double* part, double* res2, hipStream_t st)
{
    hipLaunchKernelGGL(lobpcg_resid_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, X, AX, nb, theta, dinv, mask, ldw, W, part);
    hipLaunchKernelGGL(lobpcg_resid_sum_kernel, dim3(1), dim3(64), 0, st, part, grid, nb, res2);
}

// ------------------------------------------------------------------ the pencil (A, M): ehyb_lobpcg_gen
// The Gram kernel with a third image: G = S^T BS and H = S^T AS, BS = M S.  The shape is lobpcg_gram_kernel's -- twelve waves, one
// 8 x 8 block each, lane l adds rows l and l + 64 of every tile, the same tile order, shuffle tree and grid -- so that BS == S
// gives its bits.  The tile holds three groups of 24 columns x 128 rows, 73,728 B: dynamic LDS, opted in by launch_gram_b.
// LUMPED: M = diag(m).  No third stream leaves memory: a wave forms m[r] S[r, c] (one rounding) from the S pairs it fetched
// and the tile's m pair while it fills the tile.
constexpr int kGramBTile = 3 * kS * kGramRows;  // doubles of the tile: S, AS, BS
constexpr int kGramBLds = kGramBTile * (int)sizeof(double);

template <bool LUMPED>
__global__ __launch_bounds__(kGramThreads) void lobpcg_gram_b_kernel(int n, long long ld_, const double* __restrict__ S,
                                                                     const double* __restrict__ AS, const double* __restrict__ BS,
                                                                     const double* __restrict__ m, int mc, double* __restrict__ part)
{
    // column q < 24 of the tile is column q of S, 24 + q column q of AS, 48 + q column q of BS; columns >= mc stay zero
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;  // uniform: column bases in scalar registers
    for (int k = threadIdx.x; k < kGramBTile; k += kGramThreads) tile[k] = 0.0;
    const int groups = (mc + kGroup - 1) / kGroup;
    const int b = wave % 6;
    const bool is_h = wave >= 6, active = b < groups * (groups + 1) / 2;
    const int gi = kBlockI[b], gj = kBlockJ[b];
    const double* a_sh = tile + (size_t)gi * kGroup * kGramRows;
    const double* b_sh = tile + (size_t)((is_h ? kS : 2 * kS) + gj * kGroup) * kGramRows;
    const size_t ld = (size_t)ld_;
    const long long tiles = ((long long)n + kGramRows - 1) / kGramRows;

    // a wave copies columns wave and wave + 12 of every group -- number k = 2 group + (0 or 1) -- lane l the pair (2l, 2l + 1) of
    // each: k < 6 with BS in memory; LUMPED: k < 4, and its two columns of S, scaled by the pair of m, are its two of the third group
    constexpr int kFetch = LUMPED ? 4 : 6;
    double2 pre[kFetch], mp = {0.0, 0.0};
    auto fetch = [&](long long t) {
        const long long i = t * kGramRows + 2 * lane;
        if (LUMPED) {
            if (i + 1 < n)
                mp = load2(m + i);
            else
                mp = {i < n ? m[i] : 0.0, 0.0};
        }
#pragma unroll
        for (int k = 0; k < kFetch; ++k) {
            const int c = wave + kGramWaves * (k & 1);
            if (c >= mc) continue;
            const double* col = (k < 2 ? S : k < 4 ? AS : BS) + (size_t)c * ld;
            if (i + 1 < n)
                pre[k] = load2(col + i);
            else
                pre[k] = {i < n ? col[i] : 0.0, 0.0};
        }
    };
    auto put = [&]() {
#pragma unroll
        for (int k = 0; k < kFetch; ++k) {
            const int c = wave + kGramWaves * (k & 1);
            if (c >= mc) continue;
            store2(tile + (size_t)(kS * (k / 2) + c) * kGramRows + 2 * lane, pre[k]);
            if (LUMPED && k < 2) store2(tile + (size_t)(2 * kS + c) * kGramRows + 2 * lane, double2{mp.x * pre[k].x, mp.y * pre[k].y});
        }
    };

    double acc[kGroup][kGroup];
#pragma unroll
    for (int i = 0; i < kGroup; ++i) {
#pragma unroll
        for (int j = 0; j < kGroup; ++j) acc[i][j] = 0.0;
    }
    long long t = blockIdx.x;
    if (t < tiles) fetch(t);
    __syncthreads();  // the zeros are in place
    for (; t < tiles; t += gridDim.x) {
        put();
        __syncthreads();
        if (t + gridDim.x < tiles) fetch(t + gridDim.x);
        __builtin_amdgcn_sched_barrier(0);  // the loads are issued before the sums, not sunk behind them
        if (active) {
#pragma unroll 1  // as lobpcg_gram_kernel: 64 sums fill the registers of a wave that shares its SIMD with two more
            for (int r = lane; r < kGramRows; r += 64) {
                // four columns of a at a time, the halves kept apart: the registers this frees hold the next tile's third group.
                // Every sum still takes one term per row, in the order of the rows
#pragma unroll
                for (int h = 0; h < kGroup; h += 4) {
                    double a[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) a[i] = a_sh[(h + i) * kGramRows + r];
#pragma unroll
                    for (int j = 0; j < kGroup; ++j) {
                        const double bj = b_sh[j * kGramRows + r];
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[h + i][j] = fma(a[i], bj, acc[h + i][j]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __syncthreads();  // the tile is free
    }
    if (!active) return;
    double* slot = part + (size_t)blockIdx.x * kGramSlot + (is_h ? kS * kS : 0);
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
#pragma unroll
        for (int i = 0; i < kGroup; ++i) {
            double v = acc[i][j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            const int I = gi * kGroup + i, J = gj * kGroup + j;
            if (lane == 0 && I <= J && J < mc) slot[I + J * kS] = v;
        }
    }
}

// lobpcg_resid_kernel with R_c = AX_c - theta_c BX_c: BX read next to X, or LUMPED formed as m o X (one rounding)
template <bool LUMPED>
__global__ __launch_bounds__(kThreads) void lobpcg_resid_b_kernel(int n, long long ld_, const double* __restrict__ X,
                                                                  const double* __restrict__ AX, const double* __restrict__ BX,
                                                                  const double* __restrict__ m, int nb, const double* __restrict__ theta,
                                                                  const double* __restrict__ dinv, unsigned mask, long long ldw_, double* W,
                                                                  double* __restrict__ part)
{
    __shared__ double th[kBlock];
    if (threadIdx.x < kBlock) th[threadIdx.x] = (int)threadIdx.x < nb ? theta[threadIdx.x] : 0.0;
    __syncthreads();
    double acc[kBlock];
#pragma unroll
    for (int c = 0; c < kBlock; ++c) acc[c] = 0.0;
    const size_t ld = (size_t)ld_, ldw = (size_t)ldw_;
    const int stride = (int)gridDim.x * kThreads;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        const bool pair = i + 1 < (size_t)n;
        double2 d = {1.0, 1.0}, mm = {0.0, 0.0};
        if (dinv && mask) d = pair ? load2(dinv + i) : double2{dinv[i], 1.0};
        if (LUMPED) mm = pair ? load2(m + i) : double2{m[i], 0.0};
#pragma unroll
        for (int c = 0; c < kBlock; ++c) {
            if (c >= nb) break;
            const double* src = LUMPED ? X : BX;
            double2 bx, ax;
            if (pair) {
                bx = load2(src + (size_t)c * ld + i);
                ax = load2(AX + (size_t)c * ld + i);
            } else {
                bx = {src[(size_t)c * ld + i], 0.0};
                ax = {AX[(size_t)c * ld + i], 0.0};
            }
            if (LUMPED) {
                bx.x *= mm.x;
                bx.y *= mm.y;
            }
            double2 r;
            r.x = fma(-th[c], bx.x, ax.x);
            r.y = fma(-th[c], bx.y, ax.y);
            acc[c] = fma(r.y, r.y, fma(r.x, r.x, acc[c]));
            if (mask >> c & 1u) {
                double* w = W + (size_t)__popc(mask & ((1u << c) - 1u)) * ldw + i;
                if (dinv) {
                    r.x *= d.x;
                    r.y *= d.y;
                }
                if (pair)
                    store2(w, r);
                else
                    *w = r.x;
            }
        }
    }
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < kBlock; ++c) part[(size_t)blockIdx.x * kBlock + c] = acc[c];
    }
}

// exactly one of BS and m is given.  The tile is over the 64 KiB a kernel gets without asking: the opt-in comes before the launch.
hipError_t launch_gram_b(int n, long long ld, const double* S, const double* AS, const double* BS, const double* m, int mc, double* G,
                         double* H, double* part, hipStream_t st)
{
    const int grid = gram_grid(n);
    const void* fn = m ? reinterpret_cast<const void*>(lobpcg_gram_b_kernel<true>) : reinterpret_cast<const void*>(lobpcg_gram_b_kernel<false>);
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kGramBLds);
    if (e != hipSuccess) return e;
    if (m)
        hipLaunchKernelGGL(lobpcg_gram_b_kernel<true>, dim3(grid), dim3(kGramThreads), kGramBLds, st, n, ld, S, AS, BS, m, mc, part);
    else
        hipLaunchKernelGGL(lobpcg_gram_b_kernel<false>, dim3(grid), dim3(kGramThreads), kGramBLds, st, n, ld, S, AS, BS, m, mc, part);
    hipLaunchKernelGGL(lobpcg_gram_sum_kernel, dim3((2 * mc * mc + kThreads - 1) / kThreads), dim3(kThreads), 0, st, part, grid, mc, G, H);
    return hipGetLastError();
}

void launch_resid_b(int grid, int n, long long ld, const double* X, const double* AX, const double* BX, const double* m, int nb,
                    const double* theta, const double* dinv, unsigned mask, long long ldw, double* W, double* part, double* res2, hipStream_t st)
{
    if (m)
        hipLaunchKernelGGL(lobpcg_resid_b_kernel<true>, dim3(grid), dim3(kThreads), 0, st, n, ld, X, AX, BX, m, nb, theta, dinv, mask, ldw, W, part);
    else
        hipLaunchKernelGGL(lobpcg_resid_b_kernel<false>, dim3(grid), dim3(kThreads), 0, st, n, ld, X, AX, BX, m, nb, theta, dinv, mask, ldw, W, part);
    hipLaunchKernelGGL(lobpcg_resid_sum_kernel, dim3(1), dim3(64), 0, st, part, grid, nb, res2);
}

// ------------------------------------------------------------------ the driver
// the mass matrix of ehyb_lobpcg_gen: a plan, a diagonal, or neither (ehyb_lobpcg: M = I and the kernels without a third image)
struct Mass {
    ehyb_plan* plan;
    const double* diag;
    double bnorm;
    bool any() const { return plan || diag; }
};

struct Outputs {
    int nev;
    double *evals, *resid;
    int *nconv, *iters, *multiplies, *mass_multiplies;
    void counts(int c, int it, int mu, int mm) const
    {
        if (nconv) *nconv = c;
        if (iters) *iters = it;
        if (multiplies) *multiplies = mu;
        if (mass_multiplies) *mass_multiplies = mm;
    }
    void values(const double* theta, const double* res) const
    {
        for (int i = 0; i < nev; ++i) {
            if (evals) evals[i] = theta ? theta[i] : std::numeric_limits<double>::quiet_NaN();
            if (resid) resid[i] = res ? res[i] : std::numeric_limits<double>::quiet_NaN();
        }
    }
};

// the start block of the header: column j, row i
inline double start_entry(uint32_t i, uint32_t j)
{
    uint32_t h = (i + 1u) * 2654435761u + (j + 1u) * 40503u;
    h ^= h >> 15;
    h *= 2246822519u;
    h ^= h >> 13;
    return ((double)(h & 2047u) - 1023.5) / 1024.0;
}

// the small device arrays of a solve, in doubles behind one pointer
enum { D_THETA = 0, D_RES2 = D_THETA + kBlock, D_Y = D_RES2 + kBlock, D_G = D_Y + kS * 2 * kBlock, D_H = D_G + kS * kS,
       D_PART = D_H + kS * kS, D_COUNT = D_PART + (kMaxGrid / 2) * kBlock };

int lobpcg_solve(const char* who, ehyb_plan* P, const Mass& mass, ehyb_coarse* coarse, const double* dinv, const double* X0, int64_t ldx0,
                 int nev, int nb, int max_iter, double tol, double anorm, double* evecs, int64_t ldv, void* stream, const Outputs& out)
{
    const int n = P->host.n_cols;
    const size_t ld = (size_t)n + (n & 1);
    SolveLoop L(n, 0);
    double* sm;
    HIP_TRY(L.begin(stream, {}, 0, &sm, 0, D_COUNT));
    // two pairs (S, AS) of 3 nb columns: one holds [X | P | W], the other receives the rotation; they swap by pointer.  A mass
    // plan makes them triples (S, AS, BS); a lumped mass is applied where S is read
    double *S[2], *AS[2], *BS[2] = {nullptr, nullptr}, *gram_part, *Rs = nullptr;
    for (int p = 0; p < 2; ++p) {
        HIP_TRY(L.more(&S[p], ld * 3 * (size_t)nb));
        HIP_TRY(L.more(&AS[p], ld * 3 * (size_t)nb));
        if (mass.plan) HIP_TRY(L.more(&BS[p], ld * 3 * (size_t)nb));
    }
    HIP_TRY(L.more(&gram_part, (size_t)kGramGrid * kGramSlot));
    if (coarse) HIP_TRY(L.more(&Rs, ld * (size_t)nb));
    const hipStream_t st = L.st;
    int cur = 0, it = 0, mult = 0, walks = 0, mass_mult = 0, mass_walks = 0;

    std::vector<double> start;
    if (X0) {
        HIP_TRY(hipMemcpy2DAsync(S[0], ld * sizeof(double), X0, (size_t)ldx0 * sizeof(double), (size_t)n * sizeof(double), nb,
                                 hipMemcpyDeviceToDevice, st));
    } else {
        start.assign(ld * (size_t)nb, 0.0);
        for (int j = 0; j < nb; ++j)
            for (int i = 0; i < n; ++i) start[(size_t)j * ld + i] = start_entry((uint32_t)i, (uint32_t)j);
        HIP_TRY(hipMemcpyAsync(S[0], start.data(), start.size() * sizeof(double), hipMemcpyHostToDevice, st));
    }
    auto multiply = [&](int c0, int k) -> int {
        mult += k;
        const int rc = ehyb_spmm(P, S[cur] + (size_t)c0 * ld, (int64_t)ld, AS[cur] + (size_t)c0 * ld, (int64_t)ld, k, st,
                                 walks++ & 1 ? EHYB_WALK_LAST_TO_FIRST : EHYB_WALK_FIRST_TO_LAST);
        if (rc != EHYB_OK || !mass.plan) return rc;
        mass_mult += k;
        return ehyb_spmm(mass.plan, S[cur] + (size_t)c0 * ld, (int64_t)ld, BS[cur] + (size_t)c0 * ld, (int64_t)ld, k, st,
                         mass_walks++ & 1 ? EHYB_WALK_LAST_TO_FIRST : EHYB_WALK_FIRST_TO_LAST);
    };
    auto resid = [&](unsigned mask, const double* scale, double* W) {
        if (mass.any())
            launch_resid_b(L.grid, n, (long long)ld, S[cur], AS[cur], BS[cur], mass.diag, nb, sm + D_THETA, scale, mask, (long long)ld, W,
                           sm + D_PART, sm + D_RES2, st);
        else
            launch_resid(L.grid, n, (long long)ld, S[cur], AS[cur], nb, sm + D_THETA, scale, mask, (long long)ld, W, sm + D_PART, sm + D_RES2, st);
    };
    std::vector<double> GH((size_t)2 * kS * kS), theta(kBlock), Y((size_t)kS * kBlock), YY((size_t)kS * 2 * kBlock), res2(kBlock), res(kBlock);
    std::string why;
    // the Gram matrices of the first mc columns, the projected problem, the rotation by kc columns into the other pair, the swap
    auto rayleigh_ritz = [&](int mc, bool with_p, bool* broke) -> int {
        if (mass.any())
            HIP_TRY(launch_gram_b(n, (long long)ld, S[cur], AS[cur], BS[cur], mass.diag, mc, sm + D_G, sm + D_H, gram_part, st));
        else
            launch_gram(n, (long long)ld, S[cur], AS[cur], mc, sm + D_G, sm + D_H, gram_part, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(GH.data(), sm + D_G, GH.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int rank = 0;
        if (ehyb_lobpcg_rr(mc, GH.data(), GH.data() + kS * kS, nb, theta.data(), Y.data(), &rank) != EHYB_OK) {
            why = ehyb_last_error();
            *broke = true;
            return EHYB_OK;
        }
        const int kc = with_p ? 2 * nb : nb;
        std::fill(YY.begin(), YY.end(), 0.0);
        for (int c = 0; c < nb; ++c)
            for (int l = 0; l < mc; ++l) {
                YY[(size_t)c * mc + l] = Y[(size_t)c * mc + l];
                if (with_p && l >= nb) YY[(size_t)(nb + c) * mc + l] = Y[(size_t)c * mc + l];
            }
        HIP_TRY(hipMemcpyAsync(sm + D_Y, YY.data(), (size_t)mc * kc * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(sm + D_THETA, theta.data(), kBlock * sizeof(double), hipMemcpyHostToDevice, st));
        int rc = ehyb_eigsh_rotate_step(n, (int64_t)ld, S[cur], (int64_t)ld, S[cur ^ 1], sm + D_Y, mc, kc, st);
        if (rc == EHYB_OK) rc = ehyb_eigsh_rotate_step(n, (int64_t)ld, AS[cur], (int64_t)ld, AS[cur ^ 1], sm + D_Y, mc, kc, st);
        if (rc == EHYB_OK && mass.plan) rc = ehyb_eigsh_rotate_step(n, (int64_t)ld, BS[cur], (int64_t)ld, BS[cur ^ 1], sm + D_Y, mc, kc, st);
        cur ^= 1;
        return rc;
    };
    auto breakdown = [&]() -> int {
        out.values(nullptr, nullptr);
        out.counts(0, it, mult, mass_mult);
        EHYB_FAIL(EHYB_ERR_ARG, "%s: breakdown after %d iterations (%s)", who, it, why.c_str());
    };

    int rc = multiply(0, nb);
    if (rc != EHYB_OK) return rc;
    bool broke = false;
    if ((rc = rayleigh_ritz(nb, false, &broke)) != EHYB_OK) return rc;
    if (broke) return breakdown();
    const unsigned all = (1u << nb) - 1u;
    bool have_p = false;
    int nconv = 0;
    for (;; ++it) {
        const int w0 = have_p ? 2 * nb : nb;  // the first W column
        // Before the look nobody knows which columns are active, and a third look would cost more than a kernel: the launch takes
        // every column as active -- W where it belongs, or with a coarse object R into the scratch columns, which is all the
        // coarse apply needs.  Without a coarse object, once a column has converged, a second launch packs W for the active
        // ones: it reads X and AX again (2 nb + 1 vectors read, na written) and leaves the same res2.
        resid(all, coarse ? nullptr : dinv, coarse ? Rs : S[cur] + (size_t)w0 * ld);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(res2.data(), sm + D_RES2, kBlock * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));  // the first look; Y and theta are the host's again
        double nrm = anorm;
        bool finite = true;
        for (int c = 0; c < nb; ++c) {
            res[c] = std::sqrt(res2[c]);
            finite = finite && std::isfinite(res[c]) && std::isfinite(theta[c]);
            nrm = std::max(nrm, mass.bnorm * std::fabs(theta[c]));
        }
        if (!finite) {
            why = "a non-finite Ritz value or residual norm";
            return breakdown();
        }
        unsigned active = 0;
        for (int c = 0; c < nb; ++c)
            if (!(res[c] <= tol * nrm)) active |= 1u << c;
        for (nconv = 0; nconv < nev && !(active >> nconv & 1u);) ++nconv;
        if (nconv == nev || it == max_iter) break;
        const int na = __builtin_popcount(active);
        if (coarse) {
            for (int c = 0, a = 0; c < nb; ++c)
                if (active >> c & 1u) {
                    rc = ehyb_coarse_apply(coarse, dinv, Rs + (size_t)c * ld, S[cur] + (size_t)(w0 + a++) * ld, st);
                    if (rc != EHYB_OK) return rc;
                }
        } else if (active != all) {  // the active columns packed
            resid(active, dinv, S[cur] + (size_t)w0 * ld);
        }
        if ((rc = multiply(w0, na)) != EHYB_OK) return rc;
        if ((rc = rayleigh_ritz(w0 + na, true, &broke)) != EHYB_OK) return rc;  // the second look
        if (broke) return breakdown();
        have_p = true;
    }
    if (evecs) {
        HIP_TRY(hipMemcpy2DAsync(evecs, (size_t)ldv * sizeof(double), S[cur], ld * sizeof(double), (size_t)n * sizeof(double), nev,
                                 hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    out.values(theta.data(), res.data());
    out.counts(nconv, it, mult, mass_mult);
    return EHYB_OK;
}

inline double upper(const double* M, int mc, int i, int j) { return i <= j ? M[i + (size_t)j * mc] : M[j + (size_t)i * mc]; }

}  // namespace

extern "C" int ehyb_lobpcg(ehyb_plan* P, ehyb_coarse* coarse, const double* inv_diag, const double* X0, int64_t ldx0, int nev, int block,
                           int max_iter, double tol, double anorm, double* evals, double* evecs, int64_t ldv, void* stream, int* nconv,
                           int* iters_done, int* multiplies, double* resid)
{
    clear_error();
    if (!P) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg: null argument");
    const int nb = block == 0 ? nev : block;
    if (nev < 1 || nb < nev || nb > EHYB_LOBPCG_MAX_BLOCK || max_iter < 0)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg: nev %d (1 .. block), block %d (0 or nev .. %d), max_iter %d", nev, block, EHYB_LOBPCG_MAX_BLOCK,
                  max_iter);
    if (!(tol >= 0) || !(anorm >= 0) || !std::isfinite(anorm)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg: tol %g, anorm %g", tol, anorm);
    if (P->host.row_begin != 0 || P->host.row_end != P->host.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg: needs a plan over all rows");
    const int n = P->host.n_cols;
    if (nb > n) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg: a block of %d vectors for %d rows", nb, n);
    if ((evecs && (ldv < n || (ldv & 1))) || (X0 && (ldx0 < n || (ldx0 & 1))))
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg: ldv %lld and ldx0 %lld must be even and >= %d rows", (long long)ldv, (long long)ldx0, n);
    if ((((uintptr_t)evecs | (uintptr_t)inv_diag | (uintptr_t)X0) & 15) != 0)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg: evecs_dev, inv_diag_dev and X0_dev must be 16-byte aligned");
    if (coarse && coarse->n != n) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg: the coarse object has %d rows, the plan %d", coarse->n, n);
    const int rc = solve_uploaded("ehyb_lobpcg", P);
    if (rc != EHYB_OK) return rc;
    if (coarse && !coarse->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_lobpcg: coarse object not uploaded");
    const Outputs out{nev, evals, resid, nconv, iters_done, multiplies, nullptr};
    return lobpcg_solve("ehyb_lobpcg", P, Mass{nullptr, nullptr, 1.0}, coarse, inv_diag, X0, ldx0, nev, nb, max_iter, tol, anorm, evecs, ldv, stream,
                        out);
}

extern "C" int ehyb_lobpcg_gen(ehyb_plan* P, ehyb_plan* MP, const double* mass_diag, ehyb_coarse* coarse, const double* inv_diag,
                               const double* X0, int64_t ldx0, int nev, int block, int max_iter, double tol, double anorm, double bnorm,
                               double* evals, double* evecs, int64_t ldv, void* stream, int* nconv, int* iters_done, int* multiplies,
                               int* mass_multiplies, double* resid)
{
    clear_error();
    if (!P) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: null argument");
    const int nb = block == 0 ? nev : block;
    if (nev < 1 || nb < nev || nb > EHYB_LOBPCG_MAX_BLOCK || max_iter < 0)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: nev %d (1 .. block), block %d (0 or nev .. %d), max_iter %d", nev, block, EHYB_LOBPCG_MAX_BLOCK,
                  max_iter);
    if (!(tol >= 0) || !(anorm >= 0) || !std::isfinite(anorm) || !(bnorm >= 0) || !std::isfinite(bnorm))
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: tol %g, anorm %g, bnorm %g", tol, anorm, bnorm);
    if (P->host.row_begin != 0 || P->host.row_end != P->host.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: needs a plan over all rows");
    const int n = P->host.n_cols;
    if (!MP == !mass_diag) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: exactly one of mass_plan and mass_diag_dev must be given");
    if (MP && (MP->host.row_begin != 0 || MP->host.row_end != MP->host.n_cols || MP->host.n_cols != n))
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: the mass plan must cover all rows of a matrix of %d rows (it has rows %d .. %d of %d)", n,
                  MP->host.row_begin, MP->host.row_end, MP->host.n_cols);
    if (((uintptr_t)mass_diag & 15) != 0) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: mass_diag_dev must be 16-byte aligned");
    if (nb > n) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: a block of %d vectors for %d rows", nb, n);
    if ((evecs && (ldv < n || (ldv & 1))) || (X0 && (ldx0 < n || (ldx0 & 1))))
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: ldv %lld and ldx0 %lld must be even and >= %d rows", (long long)ldv, (long long)ldx0, n);
    if ((((uintptr_t)evecs | (uintptr_t)inv_diag | (uintptr_t)X0) & 15) != 0)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: evecs_dev, inv_diag_dev and X0_dev must be 16-byte aligned");
    if (coarse && coarse->n != n) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gen: the coarse object has %d rows, the plan %d", coarse->n, n);
    int rc = solve_uploaded("ehyb_lobpcg_gen", P);
    if (rc != EHYB_OK) return rc;
    if (MP && !MP->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_lobpcg_gen: mass plan not uploaded");
    if (coarse && !coarse->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_lobpcg_gen: coarse object not uploaded");
    const Outputs out{nev, evals, resid, nconv, iters_done, multiplies, mass_multiplies};
    return lobpcg_solve("ehyb_lobpcg_gen", P, Mass{MP, mass_diag, bnorm == 0 ? 1.0 : bnorm}, coarse, inv_diag, X0, ldx0, nev, nb, max_iter, tol, anorm,
                        evecs, ldv, stream, out);
}

// host only
extern "C" int ehyb_lobpcg_rr(int mc, const double* G, const double* H, int nb, double* theta, double* Y, int* rank_out)
{
    clear_error();
    if (rank_out) *rank_out = 0;
    if (!G || !H || !theta || !Y || mc < 1 || mc > kS || nb < 1 || nb > kBlock || nb > mc)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_rr: bad arguments (mc %d, 1 .. %d; nb %d, 1 .. min(%d, mc))", mc, kS, nb, kBlock);
    for (int j = 0; j < mc; ++j)
        for (int i = 0; i <= j; ++i)
            if (!std::isfinite(G[i + (size_t)j * mc]) || !std::isfinite(H[i + (size_t)j * mc]))
                EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_rr: a non-finite entry at (%d, %d)", i, j);
    int keep[kS], m = 0;
    double d[kS];
    for (int i = 0; i < mc; ++i) {
        const double g = G[i + (size_t)i * mc];
        if (g < 0) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_rr: G[%d, %d] = %g is negative", i, i, g);
        if (g == 0) continue;
        d[m] = 1.0 / std::sqrt(g);
        keep[m++] = i;
    }
    if (m < nb) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_rr: rank %d of the basis is below nb = %d", m, nb);
    // G^ = d G d with a unit diagonal, its eigenpairs, Q = D U Sigma^-1/2 over the sigma above 2^-40 sigma_max
    double Gs[kS * kS], sigma[kS], U[kS * kS];
    for (int b = 0; b < m; ++b)
        for (int a = 0; a <= b; ++a) Gs[a + b * m] = a == b ? 1.0 : d[a] * G[keep[a] + (size_t)keep[b] * mc] * d[b];
    int rc = ehyb_sym_eig(m, Gs, m, sigma, U);
    if (rc != EHYB_OK) return rc;
    int first = 0;
    while (first < m && !(sigma[first] > 0x1p-40 * sigma[m - 1])) ++first;
    const int r = m - first;
    if (rank_out) *rank_out = r;
    if (r < nb) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_rr: rank %d of the basis is below nb = %d", r, nb);
    double Q[kS * kS];  // m x r, row a is row keep[a] of the full Q
    for (int l = 0; l < r; ++l) {
        const double s = 1.0 / std::sqrt(sigma[first + l]);
        for (int a = 0; a < m; ++a) Q[a + l * m] = d[a] * U[a + (first + l) * m] * s;
    }
    // M = Q^T H Q, every sum in rising index order
    double HQ[kS * kS], M[kS * kS], th[kS], Z[kS * kS];
    for (int l = 0; l < r; ++l)
        for (int a = 0; a < m; ++a) {
            double s = 0.0;
            for (int b = 0; b < m; ++b) s += upper(H, mc, keep[a], keep[b]) * Q[b + l * m];
            HQ[a + l * m] = s;
        }
    for (int l = 0; l < r; ++l)
        for (int k = 0; k <= l; ++k) {
            double s = 0.0;
            for (int a = 0; a < m; ++a) s += Q[a + k * m] * HQ[a + l * m];
            M[k + l * r] = s;
        }
    rc = ehyb_sym_eig(r, M, r, th, Z);
    if (rc != EHYB_OK) return rc;
    std::fill(Y, Y + (size_t)mc * nb, 0.0);
    for (int c = 0; c < nb; ++c) {
        theta[c] = th[c];
        for (int a = 0; a < m; ++a) {
            double s = 0.0;
            for (int l = 0; l < r; ++l) s += Q[a + l * m] * Z[l + c * r];
            Y[keep[a] + (size_t)c * mc] = s;
        }
    }
    return EHYB_OK;
}

// ------------------------------------------------------------------ building blocks: one launch each (and its fixed-order sum)
extern "C" int ehyb_lobpcg_gram_step(int n, int64_t ld, const double* S, const double* AS, int mc, double* G, double* H, double* scratch,
                                     void* stream)
{
    clear_error();
    int rc = check_step("ehyb_lobpcg_gram_step", n, {S, AS, G, H, scratch});
    if (rc != EHYB_OK) return rc;
    if (mc < 1 || mc > kS) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gram_step: bad arguments (mc %d, 1 .. %d)", mc, kS);
    if ((rc = check_pairs("ehyb_lobpcg_gram_step", n, ld, {S, AS})) != EHYB_OK) return rc;
    launch_gram(n, (long long)ld, S, AS, mc, G, H, scratch, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_lobpcg_gram_b_step(int n, int64_t ld, const double* S, const double* AS, const double* BS, const double* mass_diag, int mc,
                                       double* G, double* H, double* scratch, void* stream)
{
    clear_error();
    int rc = check_step("ehyb_lobpcg_gram_b_step", n, {S, AS, G, H, scratch});
    if (rc != EHYB_OK) return rc;
    if (!BS == !mass_diag) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gram_b_step: exactly one of BS_dev and mass_diag_dev must be given");
    if (mc < 1 || mc > kS) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_gram_b_step: bad arguments (mc %d, 1 .. %d)", mc, kS);
    if ((rc = check_pairs("ehyb_lobpcg_gram_b_step", n, ld, {S, AS, BS, mass_diag})) != EHYB_OK) return rc;
    HIP_TRY(launch_gram_b(n, (long long)ld, S, AS, BS, mass_diag, mc, G, H, scratch, (hipStream_t)stream));
    return EHYB_OK;
}

extern "C" int ehyb_lobpcg_resid_b_step(int n, int64_t ld, const double* X, const double* AX, const double* BX, const double* mass_diag, int nb,
                                        const double* theta, const double* inv_diag, unsigned active_mask, int64_t ldw, double* W, double* res2,
                                        double* scratch, void* stream)
{
    clear_error();
    int rc = check_step("ehyb_lobpcg_resid_b_step", n, {X, AX, theta, res2, scratch});
    if (rc != EHYB_OK) return rc;
    if (!BX == !mass_diag) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_resid_b_step: exactly one of BX_dev and mass_diag_dev must be given");
    if (nb < 1 || nb > kBlock || active_mask >> nb != 0 || (active_mask && !W))
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_resid_b_step: bad arguments (nb %d, 1 .. %d; active mask 0x%x within nb bits, with its W)", nb, kBlock,
                  active_mask);
    if ((rc = check_pairs("ehyb_lobpcg_resid_b_step", n, ld, {X, AX, BX, mass_diag, inv_diag})) != EHYB_OK) return rc;
    if (active_mask && (rc = check_pairs("ehyb_lobpcg_resid_b_step", n, ldw, {W})) != EHYB_OK) return rc;
    launch_resid_b(kStepGrid, n, (long long)ld, X, AX, BX, mass_diag, nb, theta, inv_diag, active_mask, (long long)ldw, W, scratch, res2,
                   (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_lobpcg_resid_step(int n, int64_t ld, const double* X, const double* AX, int nb, const double* theta,
                                      const double* inv_diag, unsigned active_mask, int64_t ldw, double* W, double* res2, double* scratch,
                                      void* stream)
{
    clear_error();
    int rc = check_step("ehyb_lobpcg_resid_step", n, {X, AX, theta, res2, scratch});
    if (rc != EHYB_OK) return rc;
    if (nb < 1 || nb > kBlock || active_mask >> nb != 0 || (active_mask && !W))
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lobpcg_resid_step: bad arguments (nb %d, 1 .. %d; active mask 0x%x within nb bits, with its W)", nb, kBlock,
                  active_mask);
    if ((rc = check_pairs("ehyb_lobpcg_resid_step", n, ld, {X, AX, inv_diag})) != EHYB_OK) return rc;
    if (active_mask && (rc = check_pairs("ehyb_lobpcg_resid_step", n, ldw, {W})) != EHYB_OK) return rc;
    launch_resid(kStepGrid, n, (long long)ld, X, AX, nb, theta, inv_diag, active_mask, (long long)ldw, W, scratch, res2, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
