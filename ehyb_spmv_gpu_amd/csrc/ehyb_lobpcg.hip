// LOBPCG for the nev smallest eigenpairs of the plan's symmetric matrix (ehyb_lobpcg): a block of nb vectors X, their
// preconditioned residuals W and the previous directions P span the trial space S = [X | P | W] of at most 24 columns; the host
// solves the projected problem S^T A S y = theta S^T S y (ehyb_lobpcg_rr) and the device rotates S and A S into the next X and P.
// The multiplies are ehyb_spmm, the rotation is the kernel of ehyb_eigsh_rotate_step, the preconditioner is ehyb_coarse_apply,
// inv_diag or nothing.  New here: the Gram kernel, the residual kernel and their fixed-order sums.
//
// ehyb_lobpcg_gen is the same driver for the pencil K x = lambda M x: an image BS = M S beside S and AS, G = S^T BS,
// R = AX - theta BX.  Both kernels are ONE body each, instantiated for the three forms of the mass (MassForm): none (BS is S),
// stored (BS in memory, multiplied and rotated like AS for a mass plan) and lumped (M = diag(m): BS is formed as m o s inside the
// kernels, one rounding, and no third stream leaves memory).
//
// The Gram kernel.  [G | H] = S^T [BS | AS] has at most 24 x 48 entries and n terms each: it is cut into 8 x 8 blocks, of which
// the upper triangle holds at most 6 per matrix, and ONE WAVE of a workgroup of twelve owns one block for the whole launch, its
// 64 sums in registers (lane l adds rows l and l + 64 of every tile).  A workgroup walks tiles of 128 rows: all twelve waves
// copy the columns of the tile into LDS with 16-byte loads -- each column leaves HBM once -- and every wave then reads its
// 8 + 8 columns from LDS.  The loads of the next tile are in flight while the blocks of this one are summed.  At the end a wave
// adds its lanes with the shuffle tree and lane 0 writes the block's entries of the upper triangle into the workgroup's own
// slot; a second launch adds the slots in rising order and mirrors the triangle.  No atomics, no "last workgroup".  The form
// changes which columns a tile holds and where the six G waves read b, never the order of a sum: BS == S, or m == 1, gives the
// bits of the form without a mass.
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

// the mass of the pencil as the kernels see it: BS is S itself, a third image in memory, or m o S formed on the way
enum MassForm { kMassNone, kMassStored, kMassLumped };

// groups of 24 columns in a tile -- S, AS and, with a mass, BS -- and the tile's bytes: 49,152 without a mass, 73,728 with one
constexpr int gram_images(MassForm form) { return form == kMassNone ? 2 : 3; }
constexpr int gram_lds(MassForm form) { return gram_images(form) * kS * kGramRows * (int)sizeof(double); }

template <MassForm FORM>
__global__ __launch_bounds__(kGramThreads) void lobpcg_gram_kernel(int n, long long ld_, const double* __restrict__ S,
                                                                   const double* __restrict__ AS, const double* __restrict__ BS,
                                                                   const double* __restrict__ m, int mc, double* __restrict__ part)
{
    // column q < 24 of the tile is column q of S, 24 + q column q of AS and, with a mass, 48 + q column q of BS; columns >= mc stay zero
    constexpr int kImages = gram_images(FORM), kBGroup = FORM == kMassNone ? 0 : 2 * kS;  // the group whose columns are the b of G
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;  // uniform: column bases in scalar registers
    for (int k = threadIdx.x; k < kImages * kS * kGramRows; k += kGramThreads) tile[k] = 0.0;
    const int groups = (mc + kGroup - 1) / kGroup;
    const int b = wave % 6;
    const bool is_h = wave >= 6, active = b < groups * (groups + 1) / 2;
    const int gi = kBlockI[b], gj = kBlockJ[b];
    const double* a_sh = tile + (size_t)gi * kGroup * kGramRows;
    const double* b_sh = tile + (size_t)((is_h ? kS : kBGroup) + gj * kGroup) * kGramRows;
    const size_t ld = (size_t)ld_;
    const long long tiles = ((long long)n + kGramRows - 1) / kGramRows;

    // a wave copies columns wave and wave + 12 of every group -- number k = 2 group + (0 or 1) -- lane l the pair (2l, 2l + 1) of
    // each: k < 6 with BS in memory, else k < 4; lumped, its two columns of S, scaled by the pair of m, are its two of the third group
    constexpr bool kLumped = FORM == kMassLumped;
    constexpr int kFetch = FORM == kMassStored ? 6 : 4;
    double2 pre[kFetch], mp = {0.0, 0.0};
    auto fetch = [&](long long t) {
        const long long i = t * kGramRows + 2 * lane;
        if (kLumped) {
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
            if (kLumped && k < 2) store2(tile + (size_t)(2 * kS + c) * kGramRows + 2 * lane, double2{mp.x * pre[k].x, mp.y * pre[k].y});
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
#pragma unroll 1  // 64 sums fill the registers of a wave that shares its SIMD with two more
            for (int r = lane; r < kGramRows; r += 64) {
                // four columns of a at a time, the halves kept apart: the registers this frees hold the next tile's loads.
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

// R_c = AX_c - theta_c BX_c for c < nb, BX being X without a mass, read next to X when stored, formed as m o X (one rounding) when
// lumped; the partials of R_c . R_c into part[workgroup * 8 + c]; for every c in the mask
// W[:, position of c among the mask's bits] = dinv o R_c (dinv NULL: R_c).  Pairs as the kernels of gmres_device.h.
template <MassForm FORM>
__global__ __launch_bounds__(kThreads) void lobpcg_resid_kernel(int n, long long ld_, const double* __restrict__ X,
                                                                const double* __restrict__ AX, const double* __restrict__ BX,
                                                                const double* __restrict__ m, int nb, const double* __restrict__ theta,
                                                                const double* __restrict__ dinv, unsigned mask, long long ldw_, double* W,
                                                                double* __restrict__ part)
{
    constexpr bool kLumped = FORM == kMassLumped;
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
        if (kLumped) mm = pair ? load2(m + i) : double2{m[i], 0.0};
#pragma unroll
        for (int c = 0; c < kBlock; ++c) {
            if (c >= nb) break;
            const double* src = FORM == kMassStored ? BX : X;
            double2 bx, ax;
            if (pair) {
                bx = load2(src + (size_t)c * ld + i);
                ax = load2(AX + (size_t)c * ld + i);
            } else {
                bx = {src[(size_t)c * ld + i], 0.0};
                ax = {AX[(size_t)c * ld + i], 0.0};
            }
            if (kLumped) {
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

// at most one of BS and m is given; neither: no mass.  A tile with a third image is over the 64 KiB a kernel gets without asking: its
// opt-in comes before the launch, and the form without a mass makes no such call.
template <MassForm FORM>
hipError_t launch_gram_form(int grid, int n, long long ld, const double* S, const double* AS, const double* BS, const double* m, int mc,
                            double* part, hipStream_t st)
{
    if (gram_lds(FORM) > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lobpcg_gram_kernel<FORM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 gram_lds(FORM));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lobpcg_gram_kernel<FORM>, dim3(grid), dim3(kGramThreads), gram_lds(FORM), st, n, ld, S, AS, BS, m, mc, part);
    return hipSuccess;
}

hipError_t launch_gram(int n, long long ld, const double* S, const double* AS, const double* BS, const double* m, int mc, double* G, double* H,
                       double* part, hipStream_t st)
{
    const int grid = gram_grid(n);
    const hipError_t e = m    ? launch_gram_form<kMassLumped>(grid, n, ld, S, AS, BS, m, mc, part, st)
                         : BS ? launch_gram_form<kMassStored>(grid, n, ld, S, AS, BS, m, mc, part, st)
                              : launch_gram_form<kMassNone>(grid, n, ld, S, AS, BS, m, mc, part, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lobpcg_gram_sum_kernel, dim3((2 * mc * mc + kThreads - 1) / kThreads), dim3(kThreads), 0, st, part, grid, mc, G, H);
    return hipGetLastError();
}

hipError_t launch_resid(int grid, int n, long long ld, const double* X, const double* AX, const double* BX, const double* m, int nb,
                        const double* theta, const double* dinv, unsigned mask, long long ldw, double* W, double* part, double* res2,
                        hipStream_t st)
{
    auto* kernel = m ? lobpcg_resid_kernel<kMassLumped> : BX ? lobpcg_resid_kernel<kMassStored> : lobpcg_resid_kernel<kMassNone>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, X, AX, BX, m, nb, theta, dinv, mask, ldw, W, part);
    hipLaunchKernelGGL(lobpcg_resid_sum_kernel, dim3(1), dim3(64), 0, st, part, grid, nb, res2);
    return hipGetLastError();
}

// ------------------------------------------------------------------ the driver
// the mass matrix of ehyb_lobpcg_gen: a plan, a diagonal, or neither (ehyb_lobpcg: M = I and the kernels without a third image)
struct Mass {
    ehyb_plan* plan;
    const double* diag;
    double bnorm;
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
        return launch_resid(L.grid, n, (long long)ld, S[cur], AS[cur], BS[cur], mass.diag, nb, sm + D_THETA, scale, mask, (long long)ld, W,
                            sm + D_PART, sm + D_RES2, st);
    };
    std::vector<double> GH((size_t)2 * kS * kS), theta(kBlock), Y((size_t)kS * kBlock), YY((size_t)kS * 2 * kBlock), res2(kBlock), res(kBlock);
    std::string why;
    // the Gram matrices of the first mc columns, the projected problem, the rotation by kc columns into the other pair, the swap
    auto rayleigh_ritz = [&](int mc, bool with_p, bool* broke) -> int {
        HIP_TRY(launch_gram(n, (long long)ld, S[cur], AS[cur], BS[cur], mass.diag, mc, sm + D_G, sm + D_H, gram_part, st));
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
        HIP_TRY(resid(all, coarse ? nullptr : dinv, coarse ? Rs : S[cur] + (size_t)w0 * ld));
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
            HIP_TRY(resid(active, dinv, S[cur] + (size_t)w0 * ld));
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

// the checks of both solvers in the header's order, those of the mass (gen) where ehyb_lobpcg_gen makes them, then the solve
int lobpcg_checked(const char* who, bool gen, ehyb_plan* P, ehyb_plan* MP, const double* mass_diag, ehyb_coarse* coarse, const double* inv_diag,
                   const double* X0, int64_t ldx0, int nev, int block, int max_iter, double tol, double anorm, double bnorm, double* evecs,
                   int64_t ldv, void* stream, const Outputs& out)
{
    clear_error();
    if (!P) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    const int nb = block == 0 ? nev : block;
    if (nev < 1 || nb < nev || nb > EHYB_LOBPCG_MAX_BLOCK || max_iter < 0)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: nev %d (1 .. block), block %d (0 or nev .. %d), max_iter %d", who, nev, block, EHYB_LOBPCG_MAX_BLOCK, max_iter);
    if (!(tol >= 0) || !(anorm >= 0) || !std::isfinite(anorm) || !(bnorm >= 0) || !std::isfinite(bnorm)) {
        if (gen) EHYB_FAIL(EHYB_ERR_ARG, "%s: tol %g, anorm %g, bnorm %g", who, tol, anorm, bnorm);
        EHYB_FAIL(EHYB_ERR_ARG, "%s: tol %g, anorm %g", who, tol, anorm);
    }
    if (P->host.row_begin != 0 || P->host.row_end != P->host.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "%s: needs a plan over all rows", who);
    const int n = P->host.n_cols;
    if (gen) {
        if (!MP == !mass_diag) EHYB_FAIL(EHYB_ERR_ARG, "%s: exactly one of mass_plan and mass_diag_dev must be given", who);
        if (MP && (MP->host.row_begin != 0 || MP->host.row_end != MP->host.n_cols || MP->host.n_cols != n))
            EHYB_FAIL(EHYB_ERR_ARG, "%s: the mass plan must cover all rows of a matrix of %d rows (it has rows %d .. %d of %d)", who, n,
                      MP->host.row_begin, MP->host.row_end, MP->host.n_cols);
        if (((uintptr_t)mass_diag & 15) != 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: mass_diag_dev must be 16-byte aligned", who);
    }
    if (nb > n) EHYB_FAIL(EHYB_ERR_ARG, "%s: a block of %d vectors for %d rows", who, nb, n);
    if ((evecs && (ldv < n || (ldv & 1))) || (X0 && (ldx0 < n || (ldx0 & 1))))
        EHYB_FAIL(EHYB_ERR_ARG, "%s: ldv %lld and ldx0 %lld must be even and >= %d rows", who, (long long)ldv, (long long)ldx0, n);
    if ((((uintptr_t)evecs | (uintptr_t)inv_diag | (uintptr_t)X0) & 15) != 0)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: evecs_dev, inv_diag_dev and X0_dev must be 16-byte aligned", who);
    if (coarse && coarse->n != n) EHYB_FAIL(EHYB_ERR_ARG, "%s: the coarse object has %d rows, the plan %d", who, coarse->n, n);
    const int rc = solve_uploaded(who, P);
    if (rc != EHYB_OK) return rc;
    if (MP && !MP->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: mass plan not uploaded", who);
    if (coarse && !coarse->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: coarse object not uploaded", who);
    return lobpcg_solve(who, P, Mass{MP, mass_diag, bnorm == 0 ? 1.0 : bnorm}, coarse, inv_diag, X0, ldx0, nev, nb, max_iter, tol, anorm, evecs, ldv,
                        stream, out);
}

// the checks of the two Gram steps (with_mass: exactly one of BS and mass_diag), then the launch
int gram_step_checked(const char* who, bool with_mass, int n, int64_t ld, const double* S, const double* AS, const double* BS,
                      const double* mass_diag, int mc, double* G, double* H, double* scratch, void* stream)
{
    clear_error();
    int rc = check_step(who, n, {S, AS, G, H, scratch});
    if (rc != EHYB_OK) return rc;
    if (with_mass && !BS == !mass_diag) EHYB_FAIL(EHYB_ERR_ARG, "%s: exactly one of BS_dev and mass_diag_dev must be given", who);
    if (mc < 1 || mc > kS) EHYB_FAIL(EHYB_ERR_ARG, "%s: bad arguments (mc %d, 1 .. %d)", who, mc, kS);
    if ((rc = check_pairs(who, n, ld, {S, AS, BS, mass_diag})) != EHYB_OK) return rc;
    HIP_TRY(launch_gram(n, (long long)ld, S, AS, BS, mass_diag, mc, G, H, scratch, (hipStream_t)stream));
    return EHYB_OK;
}

// the checks of the two residual steps (with_mass: exactly one of BX and mass_diag), then the launch
int resid_step_checked(const char* who, bool with_mass, int n, int64_t ld, const double* X, const double* AX, const double* BX,
                       const double* mass_diag, int nb, const double* theta, const double* inv_diag, unsigned active_mask, int64_t ldw, double* W,
                       double* res2, double* scratch, void* stream)
{
    clear_error();
    int rc = check_step(who, n, {X, AX, theta, res2, scratch});
    if (rc != EHYB_OK) return rc;
    if (with_mass && !BX == !mass_diag) EHYB_FAIL(EHYB_ERR_ARG, "%s: exactly one of BX_dev and mass_diag_dev must be given", who);
    if (nb < 1 || nb > kBlock || active_mask >> nb != 0 || (active_mask && !W))
        EHYB_FAIL(EHYB_ERR_ARG, "%s: bad arguments (nb %d, 1 .. %d; active mask 0x%x within nb bits, with its W)", who, nb, kBlock, active_mask);
    if ((rc = check_pairs(who, n, ld, {X, AX, BX, mass_diag, inv_diag})) != EHYB_OK) return rc;
    if (active_mask && (rc = check_pairs(who, n, ldw, {W})) != EHYB_OK) return rc;
    HIP_TRY(launch_resid(kStepGrid, n, (long long)ld, X, AX, BX, mass_diag, nb, theta, inv_diag, active_mask, (long long)ldw, W, scratch, res2,
                         (hipStream_t)stream));
    return EHYB_OK;
}

}  // namespace

extern "C" int ehyb_lobpcg(ehyb_plan* P, ehyb_coarse* coarse, const double* inv_diag, const double* X0, int64_t ldx0, int nev, int block,
                           int max_iter, double tol, double anorm, double* evals, double* evecs, int64_t ldv, void* stream, int* nconv,
                           int* iters_done, int* multiplies, double* resid)
{
    return lobpcg_checked("ehyb_lobpcg", false, P, nullptr, nullptr, coarse, inv_diag, X0, ldx0, nev, block, max_iter, tol, anorm, 1.0, evecs, ldv,
                          stream, Outputs{nev, evals, resid, nconv, iters_done, multiplies, nullptr});
}

extern "C" int ehyb_lobpcg_gen(ehyb_plan* P, ehyb_plan* MP, const double* mass_diag, ehyb_coarse* coarse, const double* inv_diag,
                               const double* X0, int64_t ldx0, int nev, int block, int max_iter, double tol, double anorm, double bnorm,
                               double* evals, double* evecs, int64_t ldv, void* stream, int* nconv, int* iters_done, int* multiplies,
                               int* mass_multiplies, double* resid)
{
    return lobpcg_checked("ehyb_lobpcg_gen", true, P, MP, mass_diag, coarse, inv_diag, X0, ldx0, nev, block, max_iter, tol, anorm, bnorm, evecs, ldv,
                          stream, Outputs{nev, evals, resid, nconv, iters_done, multiplies, mass_multiplies});
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
    return gram_step_checked("ehyb_lobpcg_gram_step", false, n, ld, S, AS, nullptr, nullptr, mc, G, H, scratch, stream);
}

extern "C" int ehyb_lobpcg_gram_b_step(int n, int64_t ld, const double* S, const double* AS, const double* BS, const double* mass_diag, int mc,
                                       double* G, double* H, double* scratch, void* stream)
{
    return gram_step_checked("ehyb_lobpcg_gram_b_step", true, n, ld, S, AS, BS, mass_diag, mc, G, H, scratch, stream);
}

extern "C" int ehyb_lobpcg_resid_step(int n, int64_t ld, const double* X, const double* AX, int nb, const double* theta,
                                      const double* inv_diag, unsigned active_mask, int64_t ldw, double* W, double* res2, double* scratch,
                                      void* stream)
{
    return resid_step_checked("ehyb_lobpcg_resid_step", false, n, ld, X, AX, nullptr, nullptr, nb, theta, inv_diag, active_mask, ldw, W, res2, scratch,
                              stream);
}

extern "C" int ehyb_lobpcg_resid_b_step(int n, int64_t ld, const double* X, const double* AX, const double* BX, const double* mass_diag, int nb,
                                        const double* theta, const double* inv_diag, unsigned active_mask, int64_t ldw, double* W, double* res2,
                                        double* scratch, void* stream)
{
    return resid_step_checked("ehyb_lobpcg_resid_b_step", true, n, ld, X, AX, BX, mass_diag, nb, theta, inv_diag, active_mask, ldw, W, res2, scratch,
                              stream);
}
