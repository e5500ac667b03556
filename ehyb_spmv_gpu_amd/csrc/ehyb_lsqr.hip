// Device-resident LSQR (Paige-Saunders) for min ||b - A x||_2 -- over- and under-determined (padded square), inconsistent,
// singular and Tikhonov-damped systems -- on top of the EHYB plan (ehyb_lsqr): the Golub-Kahan bidiagonalisation of A, which
// needs A and A^T.  A^T is a second plan in A's numbering (plan_t: ehyb_matrix_reorder_like of the transpose) or, without one,
// ehyb_spmv_t on the plan of A.  Per column five vectors are stored: x, the two Lanczos vectors UNNORMALISED, as ehyb_minres.hip
// stores its residuals -- U = beta u, V = alpha v --, the direction w and one product vector t (A V, then A^T U).
//
// Per iteration of parity cur two multiplies and three vector kernels, each one grid-stride pass:
//   1. t = A V                                                  (ehyb_spmm on plan, walks alternating)
//   2. ustep    the stop tests on state copy cur;  U = t / alpha - (alpha / beta) U;  partials of beta'^2 = U.U
//   3. t = A^T U                                                (ehyb_spmm on plan_t, or ehyb_spmv_t per column)
//   4. vstep    V = t / beta' - (beta' / alpha) V;  partials of alpha'^2 = V.V;  skipped by rule when beta' = 0
//   5. update   the two rotations and the ||x|| recurrence;  x += (phi / rho) w;  w = V / alpha' - (theta / rho) w (alpha' > 0);
//               state copy cur ^ 1, the counter
// alpha^2 and beta^2 of iterations of parity c live in slots L_ALPHA0 + c and L_BETA0 + c, so a kernel never writes the slot it
// reads its own scalars from, and an even and an odd iteration differ in kernel arguments only: one hipGraph holds the pair.
//
// What no sum gives back is CARRIED in two state copies per column, one per parity, exactly as in ehyb_minres.hip: an iteration
// of parity cur reads copy cur -- every workgroup for itself --, workgroup 0 of its update kernel writes copy cur ^ 1.  The
// copy also holds the four numbers of the stop tests (rnorm, arnorm, xnorm, bnorm), so the tests are a function of one copy:
// the ustep kernel of the next iteration makes them on the device, the host makes the same ones (lsqr_stop, one body for
// both) on what it read.  A kernel that sets the status writes nothing else; once it is set every vector kernel returns at
// once.  No atomics; no launch reads a word that it writes (but the counter, which one workgroup owns).
//
// k right-hand sides (ehyb_lsqr_multi) are k such solves that share the multiplies; the kernels are templated on K columns per
// launch, every column with its own slots, state copies, status word and counter; ehyb_lsqr is the driver at k = 1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ehyb_internal.h"
#include "solve_loop.h"
#include "transpose_pair.h"
#include "vec_walk.h"

using namespace ehyb;

namespace {

// partial slots, kMaxGrid doubles each; column j's set starts at s + j * L_COUNT * kMaxGrid.  Behind the last set column j has
// T_COUNT doubles (its tail): the state of parity 0, the state of parity 1, and one double whose two ints are the status word
// and the iteration counter.  One column is the layout of ehyb_lsqr_layout.
enum { L_BB = 0, L_BETA0 = 1, L_ALPHA0 = 3, L_COUNT = 5 };
enum { S_RHOBAR = 0, S_PHIBAR, S_CS2, S_SN2, S_Z, S_XXNORM, S_RES2, S_ANORM2, S_RNORM, S_ARNORM, S_XNORM, S_BNORM, S_COUNT };
enum { T_FLAGS = 2 * S_COUNT, T_COUNT = T_FLAGS + 1 };

__host__ __device__ __forceinline__ double* tail_of(double* tail, int col) { return tail + (size_t)col * T_COUNT; }
__device__ __forceinline__ auto column_flags(double* tail)
{
    return [=](int col) { return (int*)(tail_of(tail, col) + T_FLAGS); };
}

// The stop tests on one state copy: 1 = rnorm <= btol bnorm + atol anorm xnorm, 2 = arnorm <= atol anorm rnorm, 0 = neither.
// Every product and the one sum are spelled out so that the device and the host round alike.
__host__ __device__ inline int lsqr_stop(const double* st, double atol, double btol)
{
    const double t = atol * sqrt(st[S_ANORM2]);
    if (st[S_RNORM] <= fma(t, st[S_XNORM], btol * st[S_BNORM])) return 1;
    if (st[S_ARNORM] <= t * st[S_RNORM]) return 2;
    return 0;
}

__device__ __forceinline__ bool square_ok(double v2) { return isfinite(v2) && v2 >= 0; }

// ------------------------------------------------------------------ the vector kernels, K columns per launch
// Columns c0 .. c0 + K - 1 of vectors with leading dimension n (B: ldb, X: ldx); K <= 4 per launch.  The walk is vec_walk.h's, so
// a column's partials and scalars are the one-vector solve's bits.  A column whose status is set is skipped.

// U = b - t (t = A x0); partials of beta_1^2 = U.U (slot L_BETA0) and of b.b.  Takes no tail.
template <int K>
__global__ __launch_bounds__(kThreads) void lsqr_init_kernel(int n, const double* __restrict__ B, long long ldb,
                                                             const double* __restrict__ T, double* __restrict__ Uv,
                                                             double* __restrict__ s, int c0)
{
    double sums[2 * K];
#pragma unroll
    for (int c = 0; c < 2 * K; ++c) sums[c] = 0.0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const size_t o = (size_t)(c0 + c) * n + i;
            const double bi = B[(size_t)(c0 + c) * ldb + i], ui = bi - T[o];
            Uv[o] = ui;
            sums[c] = fma(ui, ui, sums[c]);
            sums[K + c] = fma(bi, bi, sums[K + c]);
        }
    }
    block_sum_n(sums);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            slot<L_COUNT>(s, c0 + c, L_BETA0)[blockIdx.x] = sums[c];
            slot<L_COUNT>(s, c0 + c, L_BB)[blockIdx.x] = sums[K + c];
        }
    }
}

// V = t / beta_1 (t = A^T U); partials of alpha_1^2 = V.V (slot L_ALPHA0).  Takes no tail: the caller reads both sums, decides
// and plants the first state and the flags.  A column whose beta_1^2 is zero or not finite is left alone.
template <int K>
__global__ __launch_bounds__(kThreads) void lsqr_start_kernel(int n, const double* __restrict__ T, double* __restrict__ V,
                                                              double* __restrict__ s, int c0)
{
    double b2[K], sums[K];
#pragma unroll
    for (int c = 0; c < K; ++c) b2[c] = partials_of(slot<L_COUNT>(s, c0 + c, L_BETA0));
    block_sum_n(b2);
    bool on[K], any = false;
    double beta[K];
    const double* t[K];
    double* v[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = uniform(isfinite(b2[c]) && b2[c] > 0);
        any = any || on[c];
        beta[c] = sqrt(b2[c]);
        t[c] = T + (size_t)(c0 + c) * n;
        v[c] = V + (size_t)(c0 + c) * n;
        sums[c] = 0.0;
    }
    if (!any) return;
    walk<K, kWalkU, 1>(
        n, on, NoShared{}, [&](int c, int i, double(&in)[1], int) { in[0] = t[c][i]; },
        [&](int c, int i, const double(&in)[1], int) {
            const double vi = in[0] / beta[c];
            v[c][i] = vi;
            sums[c] = fma(vi, vi, sums[c]);
        });
    block_sum_n(sums);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<L_COUNT>(s, c0 + c, L_ALPHA0)[blockIdx.x] = sums[c];
    }
}

// w = V / alpha_1, alpha_1^2 from slot L_ALPHA0; a sum that is zero or not finite (the caller should have stopped): breakdown
template <int K>
__global__ __launch_bounds__(kThreads) void lsqr_wstart_kernel(int n, const double* __restrict__ V, double* __restrict__ W,
                                                               const double* __restrict__ s, double* tail, int c0)
{
    bool on[K];
    if (!running<K>(column_flags(tail), c0, on)) return;
    double a2[K];
#pragma unroll
    for (int c = 0; c < K; ++c) a2[c] = on[c] ? partials_of(slot<L_COUNT>(s, c0 + c, L_ALPHA0)) : 0.0;
    block_sum_n(a2);
    bool any = false;
    double alpha[K];
    const double* v[K];
    double* w[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        alpha[c] = sqrt(a2[c]);
        v[c] = V + (size_t)(c0 + c) * n;
        w[c] = W + (size_t)(c0 + c) * n;
        if (on[c] && uniform(!isfinite(a2[c]) || !(a2[c] > 0))) {
            set_status(column_flags(tail), c0 + c, ST_BREAKDOWN);
            on[c] = false;
        }
        any = any || on[c];
    }
    if (!any) return;
    walk<K, kWalkU, 1>(
        n, on, NoShared{}, [&](int c, int i, double(&in)[1], int) { in[0] = v[c][i]; },
        [&](int c, int i, const double(&in)[1], int) { w[c][i] = in[0] / alpha[c]; });
}

// step 2: the stop tests on state copy cur (converged: the status, nothing else), then U = t / alpha - (alpha / beta) U with
// alpha^2, beta^2 from the slots of parity cur; partials of beta'^2 = U.U into the beta^2 slot of the other parity
template <int K, int U>
__global__ __launch_bounds__(kThreads) void lsqr_ustep_kernel(int n, const double* __restrict__ T, double* __restrict__ Uv,
                                                              double* __restrict__ s, double* tail, int c0, int cur, double atol,
                                                              double btol)
{
    bool on[K];
    if (!running<K>(column_flags(tail), c0, on)) return;
    bool any = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        if (on[c] && uniform(lsqr_stop(tail_of(tail, c0 + c) + cur * S_COUNT, atol, btol) != 0)) {
            set_status(column_flags(tail), c0 + c, ST_CONVERGED);
            on[c] = false;
        }
        any = any || on[c];
    }
    if (!any) return;
    double sums[2 * K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        sums[c] = on[c] ? partials_of(slot<L_COUNT>(s, c0 + c, L_ALPHA0 + cur)) : 0.0;
        sums[K + c] = on[c] ? partials_of(slot<L_COUNT>(s, c0 + c, L_BETA0 + cur)) : 0.0;
    }
    block_sum_n(sums);
    const double* t[K];
    double* u[K];
    double alpha[K], ab[K], b2n[K];
    any = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        t[c] = T + (size_t)(c0 + c) * n;
        u[c] = Uv + (size_t)(c0 + c) * n;
        b2n[c] = 0.0;
        const double a2 = sums[c], b2 = sums[K + c];
        alpha[c] = sqrt(a2);
        ab[c] = alpha[c] / sqrt(b2);
        if (on[c] && uniform(!isfinite(a2) || !(a2 > 0) || !isfinite(b2) || !(b2 > 0) || !isfinite(ab[c]))) {
            set_status(column_flags(tail), c0 + c, ST_BREAKDOWN);
            on[c] = false;
        }
        any = any || on[c];
    }
    if (!any) return;
    walk<K, U, 2>(
        n, on, NoShared{},
        [&](int c, int i, double(&in)[2], int) {
            in[0] = t[c][i];
            in[1] = u[c][i];
        },
        [&](int c, int i, const double(&in)[2], int) {
            const double un = fma(-ab[c], in[1], in[0] / alpha[c]);
            u[c][i] = un;
            b2n[c] = fma(un, un, b2n[c]);
        });
    block_sum_n(b2n);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<L_COUNT>(s, c0 + c, L_BETA0 + (cur ^ 1))[blockIdx.x] = b2n[c];
    }
}

// step 4: V = t / beta' - (beta' / alpha) V with beta'^2 from the beta^2 slot of parity cur ^ 1 and alpha^2 from the alpha^2 slot
// of parity cur; partials of alpha'^2 = V.V into the alpha^2 slot of parity cur ^ 1.  beta' = 0 (the lucky end): nothing is
// written, the update kernel takes alpha' = 0.
template <int K, int U>
__global__ __launch_bounds__(kThreads) void lsqr_vstep_kernel(int n, const double* __restrict__ T, double* __restrict__ V,
                                                              double* __restrict__ s, double* tail, int c0, int cur)
{
    bool on[K];
    if (!running<K>(column_flags(tail), c0, on)) return;
    double sums[2 * K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        sums[c] = on[c] ? partials_of(slot<L_COUNT>(s, c0 + c, L_ALPHA0 + cur)) : 0.0;
        sums[K + c] = on[c] ? partials_of(slot<L_COUNT>(s, c0 + c, L_BETA0 + (cur ^ 1))) : 0.0;
    }
    block_sum_n(sums);
    const double* t[K];
    double* v[K];
    double beta_n[K], ba[K], a2n[K];
    bool any = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        t[c] = T + (size_t)(c0 + c) * n;
        v[c] = V + (size_t)(c0 + c) * n;
        a2n[c] = 0.0;
        const double a2 = sums[c], b2n = sums[K + c];
        beta_n[c] = sqrt(b2n);
        ba[c] = beta_n[c] / sqrt(a2);
        if (on[c] && uniform(!isfinite(a2) || !(a2 > 0) || !square_ok(b2n) || !isfinite(ba[c]))) {
            set_status(column_flags(tail), c0 + c, ST_BREAKDOWN);
            on[c] = false;
        }
        if (on[c] && uniform(b2n == 0.0)) on[c] = false;  // skipped by rule
        any = any || on[c];
    }
    if (!any) return;
    walk<K, U, 2>(
        n, on, NoShared{},
        [&](int c, int i, double(&in)[2], int) {
            in[0] = t[c][i];
            in[1] = v[c][i];
        },
        [&](int c, int i, const double(&in)[2], int) {
            const double vn = fma(-ba[c], in[1], in[0] / beta_n[c]);
            v[c][i] = vn;
            a2n[c] = fma(vn, vn, a2n[c]);
        });
    block_sum_n(a2n);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<L_COUNT>(s, c0 + c, L_ALPHA0 + (cur ^ 1))[blockIdx.x] = a2n[c];
    }
}

// step 5: from state copy cur, alpha^2 (parity cur), beta'^2 and alpha'^2 (parity cur ^ 1; alpha' = 0 when beta' = 0):
//   anorm^2 += alpha^2 + beta'^2 + damp^2
//   rhobar1 = hypot(rhobar, damp);  cs1 = rhobar / rhobar1;  sn1 = damp / rhobar1;  psi = sn1 phibar;  phibar1 = cs1 phibar
//   rho = hypot(rhobar1, beta');  cs = rhobar1 / rho;  sn = beta' / rho;  theta = sn alpha';  rhobar' = -cs alpha'
//   phi = cs phibar1;  phibar' = sn phibar1;  tau = sn phi
//   x += (phi / rho) w;  alpha' > 0:  w = V / alpha' - (theta / rho) w
//   delta = sn2 rho;  gbar = -cs2 rho;  rhs = phi - delta z;  zbar = rhs / gbar;  xnorm = sqrt(xxnorm + zbar^2)
//   gamma = hypot(gbar, theta);  cs2' = gbar / gamma;  sn2' = theta / gamma;  z' = rhs / gamma;  xxnorm' = xxnorm + z'^2
//   res2' = res2 + psi^2;  rnorm = sqrt(phibar'^2 + res2');  arnorm = alpha' |tau|
// Workgroup 0 writes the new state to copy cur ^ 1 and advances the counter, before it walks.
template <int K, int U>
__global__ __launch_bounds__(kThreads) void lsqr_update_kernel(int n, const double* __restrict__ V, double* __restrict__ W,
                                                               double* __restrict__ X, long long ldx, const double* __restrict__ s,
                                                               double* tail, int c0, int cur, double damp)
{
    bool on[K];
    if (!running<K>(column_flags(tail), c0, on)) return;
    double sums[3 * K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        sums[c] = on[c] ? partials_of(slot<L_COUNT>(s, c0 + c, L_ALPHA0 + cur)) : 0.0;
        sums[K + c] = on[c] ? partials_of(slot<L_COUNT>(s, c0 + c, L_BETA0 + (cur ^ 1))) : 0.0;
        sums[2 * K + c] = on[c] ? partials_of(slot<L_COUNT>(s, c0 + c, L_ALPHA0 + (cur ^ 1))) : 0.0;
    }
    block_sum_n(sums);
    const double* v[K];
    double* w[K];
    double* x[K];
    double alpha_n[K], t1[K], t2[K], next[K][S_COUNT];
    bool both[K], last[K], any = false, any_both = false, any_last = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        v[c] = V + (size_t)(c0 + c) * n;
        w[c] = W + (size_t)(c0 + c) * n;
        x[c] = X + (size_t)(c0 + c) * ldx;
        const double* st = tail_of(tail, c0 + c) + cur * S_COUNT;
        double in[S_COUNT];
#pragma unroll
        for (int q = 0; q < S_COUNT; ++q) in[q] = on[c] ? st[q] : 0.0;
        const double a2 = sums[c], b2n = sums[K + c];
        const bool lucky = uniform(b2n == 0.0);  // beta' = 0: the vstep kernel wrote no alpha'^2
        const double a2n = lucky ? 0.0 : sums[2 * K + c];
        const double beta_n = sqrt(b2n);
        alpha_n[c] = sqrt(a2n);
        const double rhobar1 = hypot(in[S_RHOBAR], damp), cs1 = in[S_RHOBAR] / rhobar1, sn1 = damp / rhobar1;
        const double psi = sn1 * in[S_PHIBAR], phibar1 = cs1 * in[S_PHIBAR];
        const double rho = hypot(rhobar1, beta_n), cs = rhobar1 / rho, sn = beta_n / rho;
        const double theta = sn * alpha_n[c], phi = cs * phibar1, phibar_n = sn * phibar1, tau = sn * phi;
        t1[c] = phi / rho;
        t2[c] = theta / rho;
        const double delta = in[S_SN2] * rho, gbar = -in[S_CS2] * rho, rhs = fma(-delta, in[S_Z], phi), zbar = rhs / gbar;
        const double gamma = hypot(gbar, theta), zn = rhs / gamma;
        const double res2n = fma(psi, psi, in[S_RES2]);
        next[c][S_RHOBAR] = -cs * alpha_n[c];
        next[c][S_PHIBAR] = phibar_n;
        next[c][S_CS2] = gbar / gamma;
        next[c][S_SN2] = theta / gamma;
        next[c][S_Z] = zn;
        next[c][S_XXNORM] = fma(zn, zn, in[S_XXNORM]);
        next[c][S_RES2] = res2n;
        next[c][S_ANORM2] = fma(damp, damp, (in[S_ANORM2] + a2) + b2n);
        next[c][S_RNORM] = sqrt(fma(phibar_n, phibar_n, res2n));
        next[c][S_ARNORM] = alpha_n[c] * fabs(tau);
        next[c][S_XNORM] = sqrt(fma(zbar, zbar, in[S_XXNORM]));
        next[c][S_BNORM] = in[S_BNORM];
        if (on[c] && uniform(!square_ok(b2n) || !square_ok(a2n) || !isfinite(rho) || !(rho > 0) || !isfinite(t1[c]) || !isfinite(t2[c]))) {
            set_status(column_flags(tail), c0 + c, ST_BREAKDOWN);
            on[c] = false;
        }
        both[c] = on[c] && uniform(a2n > 0);
        last[c] = on[c] && !both[c];
        any = any || on[c];
        any_both = any_both || both[c];
        any_last = any_last || last[c];
    }
    if (!any) return;
    // Before the walk, so that the new state is not held in registers across it: no workgroup of this launch reads copy cur ^ 1
    // or the counter.
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!on[c]) continue;
            double* out = tail_of(tail, c0 + c) + (cur ^ 1) * S_COUNT;
#pragma unroll
            for (int q = 0; q < S_COUNT; ++q) out[q] = next[c][q];
            column_flags(tail)(c0 + c)[F_ITERS] += 1;
        }
    }
    if (any_both) {
        walk<K, U, 3>(
            n, both, NoShared{},
            [&](int c, int i, double(&in)[3], int) {
                in[0] = v[c][i];
                in[1] = w[c][i];
                in[2] = x[c][i];
            },
            [&](int c, int i, const double(&in)[3], int) {
                x[c][i] = fma(t1[c], in[1], in[2]);
                w[c][i] = fma(-t2[c], in[1], in[0] / alpha_n[c]);
            });
    }
    if (any_last) {  // alpha' = 0, the lucky end (once per solve): w is not needed again
        walk<K, 1, 2>(
            n, last, NoShared{},
            [&](int c, int i, double(&in)[2], int) {
                in[0] = w[c][i];
                in[1] = x[c][i];
            },
            [&](int c, int i, const double(&in)[2], int) { x[c][i] = fma(t1[c], in[0], in[1]); });
    }
}

// grid strides per trip: four wherever the loads of a trip fit the registers, two for the wider launches
constexpr int pair_depth(int K) { return K <= 2 ? 4 : 2; }     // ustep, vstep: two vectors per column
constexpr int update_depth(int K) { return K == 1 ? 4 : 2; }   // update: three

template <int K>
void launch_ustep(int grid, hipStream_t st, int n, const double* t, double* u, double* s, double* tail, int c0, int cur, double atol,
                  double btol)
{
    hipLaunchKernelGGL((lsqr_ustep_kernel<K, pair_depth(K)>), dim3(grid), dim3(kThreads), 0, st, n, t, u, s, tail, c0, cur, atol, btol);
}
template <int K>
void launch_vstep(int grid, hipStream_t st, int n, const double* t, double* v, double* s, double* tail, int c0, int cur)
{
    hipLaunchKernelGGL((lsqr_vstep_kernel<K, pair_depth(K)>), dim3(grid), dim3(kThreads), 0, st, n, t, v, s, tail, c0, cur);
}
template <int K>
void launch_update(int grid, hipStream_t st, int n, const double* v, double* w, double* x, long long ldx, const double* s, double* tail,
                   int c0, int cur, double damp)
{
    hipLaunchKernelGGL((lsqr_update_kernel<K, update_depth(K)>), dim3(grid), dim3(kThreads), 0, st, n, v, w, x, ldx, s, tail, c0, cur,
                       damp);
}

// The first `grid` partials of a slot added up as a workgroup does it (partials_of, then block_sum_n): the host plants the
// first state from these bits, so that its stop tests are the device's.
double device_order_sum(const double* part, int grid)
{
    double v[kThreads];
    for (int t = 0; t < kThreads; ++t) {
        v[t] = 0.0;
        for (int i = t; i < grid; i += kThreads) v[t] += part[i];
    }
    double total = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) {
        double* lane = v + w * 64;
        for (int off = 32; off > 0; off >>= 1) {
            double next[64];
            for (int l = 0; l < 64; ++l) next[l] = lane[l] + lane[l ^ off];
            std::memcpy(lane, next, sizeof(next));
        }
        total += lane[0];
    }
    return total;
}

// The checks of both entry points, in the order of include/ehyb.h; all before any device work.  Those of the pair (plan, plan_t)
// are transpose_pair.h's, shared with ehyb_svds.hip.
int lsqr_checks(const char* who, const ehyb_plan* P, const ehyb_plan* PT, bool args_ok, double damp, double atol, double btol, int max_iter)
{
    if (!P || !args_ok) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    if (max_iter < 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: max_iter %d", who, max_iter);
    if (!(damp >= 0) || !(atol >= 0) || !(btol >= 0)) EHYB_FAIL(EHYB_ERR_ARG, "%s: damp %g, atol %g, btol %g", who, damp, atol, btol);
    const int rc = pair_args(who, P, PT);
    return rc != EHYB_OK ? rc : pair_uploaded(who, P, PT);
}

// The one driver: k solves that share both multiplies.  Every column has its own slots, state, status word and counter and is
// decided on the device; the host plants the first state and the flags from the sums of the init and start kernels, reads all
// of them at a check point and goes on while any column is running.
int lsqr_solve(const char* who, bool name_column, ehyb_plan* P, ehyb_plan* PT, const double* B, int64_t ldb, double* X, int64_t ldx, int k,
               double damp, double atol, double btol, int max_iter, int check_every, void* stream, ehyb_lsqr_info* info)
{
    const int n = P->host.n_cols;
    SolveLoop L(n, check_every);
    const int grid = L.grid;
    double *u, *v, *w, *t, *s;
    HIP_TRY(L.begin(stream, {&u, &v, &w, &t}, (size_t)n * k, &s, (size_t)k * L_COUNT, (size_t)k * T_COUNT));
    const size_t tail_at = (size_t)k * L_COUNT * kMaxGrid;
    double* tail = s + tail_at;
    const hipStream_t st = L.st;
    // T = A^T U: one ehyb_spmm on the plan of A^T, or column by column on the plan of A (transpose_pair.h)
    const auto multiply_t = [&](const double* in, double* out, int walk) -> int { return ::multiply_t(P, PT, in, out, n, k, st, walk); };

    int rc = ehyb_spmm(P, X, ldx, t, n, k, st, EHYB_WALK_LAST_TO_FIRST);
    if (rc != EHYB_OK) return rc;
    for_each_group(k, [&](auto K, int c0) {
        hipLaunchKernelGGL(lsqr_init_kernel<decltype(K)::value>, dim3(grid), dim3(kThreads), 0, st, n, B, (long long)ldb, t, u, s, c0);
    });
    if ((rc = multiply_t(u, t, EHYB_WALK_FIRST_TO_LAST)) != EHYB_OK) return rc;
    for_each_group(k, [&](auto K, int c0) {
        hipLaunchKernelGGL(lsqr_start_kernel<decltype(K)::value>, dim3(grid), dim3(kThreads), 0, st, n, t, v, s, c0);
    });
    HIP_TRY(L.read());
    std::vector<int> f((size_t)k * F_COUNT, 0);  // {status, iterations} per column, as on the device
    std::vector<double> state((size_t)k * S_COUNT, 0.0);  // the copy the last update wrote
    std::vector<char> at_start(k, 0);                      // beta_1 = 0 or alpha_1 = 0
    int n_running = 0;
    for (int j = 0; j < k; ++j) {
        const double bb = device_order_sum(&L.h[(size_t)(j * L_COUNT + L_BB) * kMaxGrid], grid);
        const double b2 = device_order_sum(&L.h[(size_t)(j * L_COUNT + L_BETA0) * kMaxGrid], grid);
        const bool b_ok = std::isfinite(bb) && std::isfinite(b2) && b2 >= 0;
        const double a2 = b_ok && b2 > 0 ? device_order_sum(&L.h[(size_t)(j * L_COUNT + L_ALPHA0) * kMaxGrid], grid) : 0.0;
        const bool ok = b_ok && std::isfinite(a2) && a2 >= 0;
        double* S = &state[(size_t)j * S_COUNT];
        const double beta = ok ? std::sqrt(b2) : NAN, alpha = ok ? std::sqrt(a2) : NAN;
        S[S_RHOBAR] = alpha;
        S[S_PHIBAR] = S[S_RNORM] = S[S_BNORM] = beta;
        S[S_CS2] = -1.0;
        S[S_ARNORM] = alpha * beta;
        at_start[j] = ok && (b2 == 0 || a2 == 0);
        const int status = !ok ? ST_BREAKDOWN : at_start[j] || lsqr_stop(S, atol, btol) ? ST_CONVERGED : ST_RUNNING;
        double* tl = &L.h[tail_at + (size_t)j * T_COUNT];
        std::memset(tl, 0, T_COUNT * sizeof(double));
        std::memcpy(tl, S, S_COUNT * sizeof(double));
        f[j * F_COUNT + F_STATUS] = status;
        std::memcpy(tl + T_FLAGS, &f[j * F_COUNT], F_COUNT * sizeof(int));
        n_running += status == ST_RUNNING;
    }
    HIP_TRY(hipMemcpyAsync(tail, &L.h[tail_at], (size_t)k * T_COUNT * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    for_each_group(k, [&](auto K, int c0) {
        hipLaunchKernelGGL(lsqr_wstart_kernel<decltype(K)::value>, dim3(grid), dim3(kThreads), 0, st, n, v, w, s, tail, c0);
    });

    // An even and an odd iteration are one graph; A walks first to last, then last to first, A^T the other way round.
    int it = 0;
    rc = L.run(
        P, max_iter, it, [&] { return n_running > 0; },
        [&](int cur, bool) -> int {
            const int fwd = cur == 0 ? EHYB_WALK_FIRST_TO_LAST : EHYB_WALK_LAST_TO_FIRST, back = cur == 0 ? EHYB_WALK_LAST_TO_FIRST : EHYB_WALK_FIRST_TO_LAST;
            int e = ehyb_spmm(P, v, n, t, n, k, st, fwd);  // stopped columns included
            if (e != EHYB_OK) return e;
            for_each_group(k, [&](auto K, int c0) { launch_ustep<decltype(K)::value>(grid, st, n, t, u, s, tail, c0, cur, atol, btol); });
            if ((e = multiply_t(u, t, back)) != EHYB_OK) return e;
            for_each_group(k, [&](auto K, int c0) {
                launch_vstep<decltype(K)::value>(grid, st, n, t, v, s, tail, c0, cur);
                launch_update<decltype(K)::value>(grid, st, n, v, w, X, (long long)ldx, s, tail, c0, cur, damp);
            });
            return EHYB_OK;
        },
        [&](int) -> int {
            n_running = 0;
            for (int j = 0; j < k; ++j) {
                const double* tl = &L.h[tail_at + (size_t)j * T_COUNT];
                std::memcpy(&f[j * F_COUNT], tl + T_FLAGS, F_COUNT * sizeof(int));
                std::memcpy(&state[(size_t)j * S_COUNT], tl + (f[j * F_COUNT + F_ITERS] & 1) * S_COUNT, S_COUNT * sizeof(double));
                // the test the next ustep kernel would make
                n_running += f[j * F_COUNT + F_STATUS] == ST_RUNNING && !lsqr_stop(&state[(size_t)j * S_COUNT], atol, btol);
            }
            return EHYB_OK;
        });
    if (rc != EHYB_OK) return rc;
    int broke = -1;
    for (int j = k - 1; j >= 0; --j) {
        const double* S = &state[(size_t)j * S_COUNT];
        const int status = f[j * F_COUNT + F_STATUS], stop = lsqr_stop(S, atol, btol);
        if (status == ST_BREAKDOWN) broke = j;
        if (!info) continue;
        info[j].istop = status == ST_BREAKDOWN ? -1 : at_start[j] ? 0 : stop ? stop : 7;
        info[j].iters = f[j * F_COUNT + F_ITERS];
        info[j].rnorm = S[S_RNORM];
        info[j].arnorm = S[S_ARNORM];
        info[j].anorm = std::sqrt(S[S_ANORM2]);
        info[j].xnorm = S[S_XNORM];
    }
    if (broke < 0) return EHYB_OK;
    const int done = f[broke * F_COUNT + F_ITERS];
    const char* what = "a non-finite b.b, beta^2, alpha^2, rho or phi / rho, or a zero rho";
    if (name_column) EHYB_FAIL(EHYB_ERR_ARG, "%s: breakdown in column %d after %d iterations (%s)", who, broke, done, what);
    EHYB_FAIL(EHYB_ERR_ARG, "%s: breakdown after %d iterations (%s)", who, done, what);
}

}  // namespace

extern "C" int ehyb_lsqr(ehyb_plan* P, ehyb_plan* PT, const double* b, double* x, double damp, double atol, double btol, int max_iter,
                         int check_every, void* stream, ehyb_lsqr_info* info)
{
    clear_error();
    const int rc = lsqr_checks("ehyb_lsqr", P, PT, b && x, damp, atol, btol, max_iter);
    if (rc != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    return lsqr_solve("ehyb_lsqr", false, P, PT, b, n, x, n, 1, damp, atol, btol, max_iter, check_every, stream, info);
}

// k right-hand sides, two multiplies per iteration
extern "C" int ehyb_lsqr_multi(ehyb_plan* P, ehyb_plan* PT, const double* B, int64_t ldb, double* X, int64_t ldx, int k, double damp,
                               double atol, double btol, int max_iter, int check_every, void* stream, ehyb_lsqr_info* info)
{
    clear_error();
    int rc = multi_args("ehyb_lsqr_multi", P, ldb, ldx, k);
    if (rc == EHYB_OK) rc = lsqr_checks("ehyb_lsqr_multi", P, PT, B && X, damp, atol, btol, max_iter);
    if (rc != EHYB_OK) return rc;
    return lsqr_solve("ehyb_lsqr_multi", true, P, PT, B, ldb, X, ldx, k, damp, atol, btol, max_iter, check_every, stream, info);
}

// ------------------------------------------------------------------ building blocks for a caller that owns the loop
// The six vector kernels above, one launch each on k = 1 .. 4 columns of leading dimension n, for a caller that issues the
// multiplies itself (and for tests that look at one kernel at a time).  s: k sets of `slots` slots of `slot_doubles` doubles and k
// tails of tail_doubles behind them (ehyb_lsqr_layout); every launch uses slot_doubles / 2 workgroups.  Asynchronous on `stream`.
extern "C" int ehyb_lsqr_layout(ehyb_lsqr_slots* out)
{
    if (!out) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lsqr_layout: null argument");
    out->slots = L_COUNT;
    out->slot_doubles = kMaxGrid;
    out->slot_bb = L_BB;
    out->slot_beta0 = L_BETA0;
    out->slot_alpha0 = L_ALPHA0;
    out->tail_doubles = T_COUNT;
    out->state_doubles = S_COUNT;
    out->state_rhobar = S_RHOBAR;
    out->state_phibar = S_PHIBAR;
    out->state_cs2 = S_CS2;
    out->state_sn2 = S_SN2;
    out->state_z = S_Z;
    out->state_xxnorm = S_XXNORM;
    out->state_res2 = S_RES2;
    out->state_anorm2 = S_ANORM2;
    out->state_rnorm = S_RNORM;
    out->state_arnorm = S_ARNORM;
    out->state_xnorm = S_XNORM;
    out->state_bnorm = S_BNORM;
    out->flags_at = T_FLAGS;
    out->flag_status = F_STATUS;
    out->flag_iters = F_ITERS;
    out->flag_count = F_COUNT;
    out->status_running = ST_RUNNING;
    out->status_converged = ST_CONVERGED;
    out->status_breakdown = ST_BREAKDOWN;
    return EHYB_OK;
}

namespace {

constexpr int kStepGrid = kMaxGrid / 2;

inline double* step_tail(double* s, int k) { return s + (size_t)k * L_COUNT * kMaxGrid; }

// f(K as an integral constant) for a step call on k columns
template <typename F>
int step_columns(const char* who, int n, int k, std::initializer_list<const void*> required, F&& f)
{
    const int rc = check_step(who, n, required);
    if (rc != EHYB_OK) return rc;
    switch (k) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: EHYB_FAIL(EHYB_ERR_ARG, "%s: k = %d columns (1 .. %d)", who, k, kMultiMaxK);
    }
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

}  // namespace

extern "C" int ehyb_lsqr_init_step(int n, int k, const double* b, const double* t, double* u, double* s, void* stream)
{
    return step_columns("ehyb_lsqr_init_step", n, k, {b, t, u, s}, [&](auto K) {
        hipLaunchKernelGGL(lsqr_init_kernel<decltype(K)::value>, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, b, (long long)n, t,
                           u, s, 0);
    });
}

extern "C" int ehyb_lsqr_start_step(int n, int k, const double* t, double* v, double* s, void* stream)
{
    return step_columns("ehyb_lsqr_start_step", n, k, {t, v, s}, [&](auto K) {
        hipLaunchKernelGGL(lsqr_start_kernel<decltype(K)::value>, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, t, v, s, 0);
    });
}

extern "C" int ehyb_lsqr_wstart_step(int n, int k, const double* v, double* w, double* s, void* stream)
{
    return step_columns("ehyb_lsqr_wstart_step", n, k, {v, w, s}, [&](auto K) {
        hipLaunchKernelGGL(lsqr_wstart_kernel<decltype(K)::value>, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, v, w, s,
                           step_tail(s, k), 0);
    });
}

extern "C" int ehyb_lsqr_ustep_step(int n, int k, const double* t, double* u, double* s, int cur, double atol, double btol, void* stream)
{
    return step_columns("ehyb_lsqr_ustep_step", n, k, {t, u, s}, [&](auto K) {
        launch_ustep<decltype(K)::value>(kStepGrid, (hipStream_t)stream, n, t, u, s, step_tail(s, k), 0, cur & 1, atol, btol);
    });
}

extern "C" int ehyb_lsqr_vstep_step(int n, int k, const double* t, double* v, double* s, int cur, void* stream)
{
    return step_columns("ehyb_lsqr_vstep_step", n, k, {t, v, s}, [&](auto K) {
        launch_vstep<decltype(K)::value>(kStepGrid, (hipStream_t)stream, n, t, v, s, step_tail(s, k), 0, cur & 1);
    });
}

extern "C" int ehyb_lsqr_update_step(int n, int k, const double* v, double* w, double* x, double* s, int cur, double damp, void* stream)
{
    return step_columns("ehyb_lsqr_update_step", n, k, {v, w, x, s}, [&](auto K) {
        launch_update<decltype(K)::value>(kStepGrid, (hipStream_t)stream, n, v, w, x, (long long)n, s, step_tail(s, k), 0, cur & 1, damp);
    });
}
