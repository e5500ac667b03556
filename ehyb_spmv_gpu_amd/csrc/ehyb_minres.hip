// Device-resident MINRES (Paige-Saunders) for symmetric indefinite systems on top of the EHYB plan (ehyb_minres), with an
// optional positive diagonal preconditioner M^-1 = diag(inv_diag) applied on the fly.  Per column seven vectors are stored:
// x, two Lanczos residuals r, two directions w, z = M^-1 r and q = A z.
//
// Per iteration of parity cur one multiply and three vector kernels, each one grid-stride pass:
//   1. q = A z                                                   (ehyb_spmv_walk / ehyb_spmm, walks alternating)
//   2. dot      the stop test on phibar; partials of z.q
//   3. lanczos  alpha = (z.q) / beta^2;  r_new = q / beta - (alpha / beta) ra - (beta / beta_old) rb  over rb;
//               z = M^-1 r_new;  partials of r_new.z = beta_new^2 into the other beta^2 slot
//   4. update   the Givens rotation;  v = M^-1 ra / beta;  w_new = (v - eps wb - delta wa) / gamma  over wb;
//               x += phi w_new;  the counter advances
// ra is the current Lanczos residual (beta v in M's geometry), rb the one before; after an iteration (ra, rb) and (wa, wb)
// have swapped roles, so an even and an odd iteration differ in kernel arguments only and are captured into one hipGraph.
//
// Sums come from partials still in their slots (vec_reduce.h: the same fixed order in every workgroup).  What no sum can
// give back is CARRIED: the rotation (dbar, eps, phibar, cs, sn) and the previous beta.  Behind the partial slots every
// column has two copies of that state, one per parity.  An iteration of parity cur reads copy cur -- every workgroup for
// itself -- and workgroup 0 of its update kernel writes copy cur ^ 1: no launch reads a word that it writes.  The previous
// beta is carried for the same reason: beta_new^2 goes to the slot that held beta_old^2, so the lanczos kernel, which
// needs beta / beta_old, must not read that slot.  A carried beta_old of 0 marks the first iteration (no rb term).
//
// Stopping and breakdown are decided on the device, by the rules of ehyb_bicgstab.hip: a status word and an iteration
// counter per column sit behind the state copies.  A kernel that sets the status writes nothing else, so the update kernel
// never sets "converged": the dot kernel of the next iteration sees the same phibar and does.  Once the status is set every
// vector kernel returns at once.
//
// k right-hand sides (ehyb_minres_multi) are k such solves that share the multiply (ehyb_spmm): the kernels are templated on
// K columns per launch, every column with its own slots, state copies, status word and counter; ehyb_minres is the driver at
// k = 1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "ehyb_internal.h"
#include "solve_loop.h"
#include "vec_walk.h"

using namespace ehyb;

namespace {

// partial slots, kMaxGrid doubles each; beta^2 = r.z of iterations of parity c lives in slot M_BETA0 + c.  Column j's set of
// slots starts at s + j * M_COUNT * kMaxGrid.  Behind the last set column j has T_COUNT doubles (its tail): the state of
// parity 0, the state of parity 1, and one double whose two ints are the status word and the iteration counter.  One column
// is the layout of ehyb_minres_layout.
enum { M_BB = 0, M_ZQ = 1, M_BETA0 = 2, M_COUNT = 4 };
enum { S_DBAR = 0, S_EPS = 1, S_PHIBAR = 2, S_CS = 3, S_SN = 4, S_BETA_OLD = 5, S_COUNT = 6 };
enum { T_FLAGS = 2 * S_COUNT, T_COUNT = T_FLAGS + 1 };

__device__ __forceinline__ double* tail_of(double* tail, int col) { return tail + (size_t)col * T_COUNT; }
// column col's status word and counter, for running and set_status (vec_reduce.h)
__device__ __forceinline__ auto column_flags(double* tail)
{
    return [=](int col) { return (int*)(tail_of(tail, col) + T_FLAGS); };
}

__device__ __forceinline__ bool converged(double phibar, double bb_sum, double thr)
{
    const double bb = bb_sum > 0 ? bb_sum : 1.0;
    return phibar * phibar <= thr * bb;
}

// ------------------------------------------------------------------ the vector kernels, K columns per launch
// Columns c0 .. c0 + K - 1 of vectors with leading dimension n (B: ldb, X: ldx); K <= 4 per launch (kMultiMaxK, for_each_group
// of solve_loop.h), K = 1 for the one-vector solve and the ehyb_minres_*_step building blocks.  The walk is vec_walk.h's, U grid
// strides per trip, so a column's partials and scalars are the one-vector solve's bits.  A column whose status is set is skipped.

// ra = b - q (q = A x0), z = M^-1 ra; partials of beta_1^2 = ra.z (slot M_BETA0) and of b.M^-1 b.  Takes no tail: the caller
// plants the first state and the flags once it has read the sums.
template <int K>
__global__ __launch_bounds__(kThreads) void minres_init_kernel(int n, const double* __restrict__ B, long long ldb,
                                                               const double* __restrict__ Q, const double* __restrict__ dinv,
                                                               double* __restrict__ R, double* __restrict__ Z, double* __restrict__ s,
                                                               int c0)
{
    double sums[2 * K];
#pragma unroll
    for (int c = 0; c < 2 * K; ++c) sums[c] = 0.0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const double di = dinv ? dinv[i] : 1.0;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const size_t o = (size_t)(c0 + c) * n + i;
            const double bi = B[(size_t)(c0 + c) * ldb + i], ri = bi - Q[o];
            const double zi = dinv ? ri * di : ri, mb = dinv ? bi * di : bi;
            R[o] = ri;
            Z[o] = zi;
            sums[c] = fma(ri, zi, sums[c]);
            sums[K + c] = fma(bi, mb, sums[K + c]);
        }
    }
    block_sum_n(sums);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            slot<M_COUNT>(s, c0 + c, M_BETA0)[blockIdx.x] = sums[c];
            slot<M_COUNT>(s, c0 + c, M_BB)[blockIdx.x] = sums[K + c];
        }
    }
}

// step 2: the stop test (phibar of state copy cur against b.M^-1 b), then partials of z.q
template <int K, int U>
__global__ __launch_bounds__(kThreads) void minres_dot_kernel(int n, const double* __restrict__ Z, const double* __restrict__ Q,
                                                              double* __restrict__ s, double* tail, int c0, int cur, double thr)
{
    bool on[K];
    if (!running<K>(column_flags(tail), c0, on)) return;
    double bb[K];
#pragma unroll
    for (int c = 0; c < K; ++c) bb[c] = on[c] ? partials_of(slot<M_COUNT>(s, c0 + c, M_BB)) : 0.0;
    block_sum_n(bb);
    const double* z[K];
    const double* q[K];
    double acc[K];
    bool any = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        z[c] = Z + (size_t)(c0 + c) * n;
        q[c] = Q + (size_t)(c0 + c) * n;
        acc[c] = 0.0;
        if (on[c] && uniform(converged(tail_of(tail, c0 + c)[cur * S_COUNT + S_PHIBAR], bb[c], thr))) {
            set_status(column_flags(tail), c0 + c, ST_CONVERGED);
            on[c] = false;
        }
        any = any || on[c];
    }
    if (!any) return;
    walk<K, U, 2>(
        n, on, NoShared{},
        [&](int c, int i, double(&in)[2], int) {
            in[0] = z[c][i];
            in[1] = q[c][i];
        },
        [&](int c, int, const double(&in)[2], int) { acc[c] = fma(in[0], in[1], acc[c]); });
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<M_COUNT>(s, c0 + c, M_ZQ)[blockIdx.x] = acc[c];
    }
}

// step 3: alpha = (z.q) / beta^2;  r_new = q / beta - (alpha / beta) ra - (beta / beta_old) rb, over rb (beta_old = 0, the first
// iteration: no rb term, rb is not read);  z = M^-1 r_new;  partials of r_new.z into the beta^2 slot of the other parity
template <int K, int U>
__global__ __launch_bounds__(kThreads) void minres_lanczos_kernel(int n, const double* __restrict__ Q, const double* __restrict__ RA,
                                                                  double* __restrict__ RB, const double* __restrict__ dinv,
                                                                  double* __restrict__ Z, double* __restrict__ s, double* tail, int c0,
                                                                  int cur)
{
    bool on[K];
    if (!running<K>(column_flags(tail), c0, on)) return;
    double sums[2 * K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        sums[c] = on[c] ? partials_of(slot<M_COUNT>(s, c0 + c, M_BETA0 + cur)) : 0.0;
        sums[K + c] = on[c] ? partials_of(slot<M_COUNT>(s, c0 + c, M_ZQ)) : 0.0;
    }
    block_sum_n(sums);
    const double* q[K];
    const double* ra[K];
    double* rb[K];
    double* z[K];
    double beta[K], ab[K], bo[K], b2n[K];
    bool first[K], later[K], any = false, any_first = false, any_later = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        q[c] = Q + (size_t)(c0 + c) * n;
        ra[c] = RA + (size_t)(c0 + c) * n;
        rb[c] = RB + (size_t)(c0 + c) * n;
        z[c] = Z + (size_t)(c0 + c) * n;
        b2n[c] = 0.0;
        const double b2 = sums[c], zq = sums[K + c], alpha = zq / b2;
        const double beta_old = on[c] ? tail_of(tail, c0 + c)[cur * S_COUNT + S_BETA_OLD] : 0.0;
        beta[c] = sqrt(b2);
        ab[c] = alpha / beta[c];
        bo[c] = beta[c] / beta_old;
        first[c] = uniform(beta_old == 0.0);
        if (on[c] && uniform(!isfinite(zq) || !(b2 > 0) || !isfinite(b2) || !isfinite(ab[c]) || (!first[c] && !isfinite(bo[c])))) {
            set_status(column_flags(tail), c0 + c, ST_BREAKDOWN);
            on[c] = false;
        }
        later[c] = on[c] && !first[c];
        first[c] = on[c] && first[c];
        any = any || on[c];
        any_first = any_first || first[c];
        any_later = any_later || later[c];
    }
    if (!any) return;
    // what both formulas do with the new residual rn
    const auto put = [&](int c, int i, double rn, double di) {
        const double zi = dinv ? rn * di : rn;
        rb[c][i] = rn;
        z[c][i] = zi;
        b2n[c] = fma(rn, zi, b2n[c]);
    };
    if (any_first) {  // the columns in their first iteration (once per solve): one plain pass, rb is not read
        walk<K, 1, 2>(
            n, first, InvDiag{dinv},
            [&](int c, int i, double(&in)[2], double) {
                in[0] = q[c][i];
                in[1] = ra[c][i];
            },
            [&](int c, int i, const double(&in)[2], double di) { put(c, i, fma(-ab[c], in[1], in[0] / beta[c]), di); });
    }
    if (any_later) {
        walk<K, U, 3>(
            n, later, InvDiag{dinv},
            [&](int c, int i, double(&in)[3], double) {
                in[0] = q[c][i];
                in[1] = ra[c][i];
                in[2] = rb[c][i];
            },
            [&](int c, int i, const double(&in)[3], double di) {
                put(c, i, fma(-bo[c], in[2], fma(-ab[c], in[1], in[0] / beta[c])), di);
            });
    }
    block_sum_n(b2n);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<M_COUNT>(s, c0 + c, M_BETA0 + (cur ^ 1))[blockIdx.x] = b2n[c];
    }
}

// step 4: from state copy cur, alpha, beta and beta_new: delta = cs dbar + sn alpha;  gbar = sn dbar - cs alpha;
// eps' = sn beta_new;  dbar' = -cs beta_new;  gamma = sqrt(gbar^2 + beta_new^2);  cs' = gbar / gamma;  sn' = beta_new / gamma;
// phi = cs' phibar;  phibar' = sn' phibar.  v = M^-1 ra / beta;  w_new = (v - eps wb - delta wa) / gamma, over wb;  x += phi w_new.
// Workgroup 0 writes the new state to copy cur ^ 1 and advances the counter.
template <int K, int U>
__global__ __launch_bounds__(kThreads) void minres_update_kernel(int n, const double* __restrict__ RA, const double* __restrict__ dinv,
                                                                 const double* __restrict__ WA, double* __restrict__ WB,
                                                                 double* __restrict__ X, long long ldx, const double* __restrict__ s,
                                                                 double* tail, int c0, int cur)
{
    bool on[K];
    if (!running<K>(column_flags(tail), c0, on)) return;
    double sums[3 * K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        sums[c] = on[c] ? partials_of(slot<M_COUNT>(s, c0 + c, M_BETA0 + cur)) : 0.0;
        sums[K + c] = on[c] ? partials_of(slot<M_COUNT>(s, c0 + c, M_ZQ)) : 0.0;
        sums[2 * K + c] = on[c] ? partials_of(slot<M_COUNT>(s, c0 + c, M_BETA0 + (cur ^ 1))) : 0.0;
    }
    block_sum_n(sums);
    const double* ra[K];
    const double* wa[K];
    double* wb[K];
    double* x[K];
    double beta[K], eps[K], delta[K], gamma[K], phi[K], next[K][S_COUNT];
    bool any = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        ra[c] = RA + (size_t)(c0 + c) * n;
        wa[c] = WA + (size_t)(c0 + c) * n;
        wb[c] = WB + (size_t)(c0 + c) * n;
        x[c] = X + (size_t)(c0 + c) * ldx;
        const double* st = tail_of(tail, c0 + c) + cur * S_COUNT;
        const double dbar = on[c] ? st[S_DBAR] : 0.0, phibar = on[c] ? st[S_PHIBAR] : 0.0, cs = on[c] ? st[S_CS] : 0.0,
                     sn = on[c] ? st[S_SN] : 0.0;
        eps[c] = on[c] ? st[S_EPS] : 0.0;
        const double b2 = sums[c], zq = sums[K + c], b2n = sums[2 * K + c], alpha = zq / b2;
        beta[c] = sqrt(b2);
        const double beta_new = sqrt(b2n);
        delta[c] = fma(cs, dbar, sn * alpha);
        const double gbar = fma(sn, dbar, -(cs * alpha));
        gamma[c] = sqrt(fma(gbar, gbar, beta_new * beta_new));
        const double cs_new = gbar / gamma[c], sn_new = beta_new / gamma[c];
        phi[c] = cs_new * phibar;
        next[c][S_DBAR] = -cs * beta_new;
        next[c][S_EPS] = sn * beta_new;
        next[c][S_PHIBAR] = sn_new * phibar;
        next[c][S_CS] = cs_new;
        next[c][S_SN] = sn_new;
        next[c][S_BETA_OLD] = beta[c];
        if (on[c] && uniform(!isfinite(zq) || !(b2 > 0) || !isfinite(b2) || !isfinite(alpha) || !(b2n >= 0) || !isfinite(b2n) ||
                             !(gamma[c] > 0) || !isfinite(gamma[c]) || !isfinite(delta[c]) || !isfinite(phi[c]))) {
            set_status(column_flags(tail), c0 + c, ST_BREAKDOWN);
            on[c] = false;
        }
        any = any || on[c];
    }
    if (!any) return;
    walk<K, U, 4>(
        n, on, InvDiag{dinv},
        [&](int c, int i, double(&in)[4], double) {
            in[0] = ra[c][i];
            in[1] = wa[c][i];
            in[2] = wb[c][i];
            in[3] = x[c][i];
        },
        [&](int c, int i, const double(&in)[4], double di) {
            const double vi = (dinv ? in[0] * di : in[0]) / beta[c];
            const double wn = fma(-delta[c], in[1], fma(-eps[c], in[2], vi)) / gamma[c];
            wb[c][i] = wn;
            x[c][i] = fma(phi[c], wn, in[3]);
        });
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!on[c]) continue;
            double* out = tail_of(tail, c0 + c) + (cur ^ 1) * S_COUNT;
#pragma unroll
            for (int w = 0; w < S_COUNT; ++w) out[w] = next[c][w];
            column_flags(tail)(c0 + c)[F_ITERS] += 1;
        }
    }
}

// grid strides per trip: four wherever the loads of a trip fit the registers, two for the wide lanczos and update kernels
// (update: four vectors per column)
constexpr int kDotU = 4;
constexpr int lanczos_depth(int K) { return K <= 2 ? 4 : 2; }
constexpr int update_depth(int K) { return K == 1 ? 4 : 2; }

// what one iteration of parity cur launches for columns c0 .. c0 + K - 1 after q = A z
template <int K>
void launch_iteration(int grid, hipStream_t st, int n, const double* q, const double* ra, double* rb, const double* dinv, double* z,
                      const double* wa, double* wb, double* x, long long ldx, double* s, double* tail, int c0, int cur, double thr)
{
    hipLaunchKernelGGL((minres_dot_kernel<K, kDotU>), dim3(grid), dim3(kThreads), 0, st, n, z, q, s, tail, c0, cur, thr);
    hipLaunchKernelGGL((minres_lanczos_kernel<K, lanczos_depth(K)>), dim3(grid), dim3(kThreads), 0, st, n, q, ra, rb, dinv, z, s, tail, c0,
                       cur);
    hipLaunchKernelGGL((minres_update_kernel<K, update_depth(K)>), dim3(grid), dim3(kThreads), 0, st, n, ra, dinv, wa, wb, x, ldx, s, tail,
                       c0, cur);
}

// The first `grid` partials of a slot added up as a workgroup does it (partials_of, then block_sum_n): per thread its entries
// in rising order, the xor tree within a wave, the waves in order.  The host needs these bits, not just this value: phibar
// starts as sqrt of this sum of beta_1^2, and the host's stop test must be the device's, or the check points would matter.
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

// The one driver: k solves that share q = A z (ehyb_spmm with explicit walks; its pass of width 1 is ehyb_spmv_walk, so k = 1
// launches the one-vector sequence).  Every column has its own slots, state, status word and counter and is decided on the
// device; the host plants the first state and the flags from the sums of the init kernel, reads all of them at a check point
// and goes on while any column is running.  The entry points have made their checks (solve_loop.h); who: the entry point,
// name_column: whether the breakdown text says which column.
int minres_solve(const char* who, bool name_column, ehyb_plan* P, const double* dinv, const double* B, int64_t ldb, double* X, int64_t ldx,
                 int k, int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const int n = P->host.n_cols;
    SolveLoop L(n, check_every);
    const int grid = L.grid;
    double *r[2], *w[2], *z, *q, *s;
    HIP_TRY(L.begin(stream, {&r[0], &r[1], &w[0], &w[1], &z, &q}, (size_t)n * k, &s, (size_t)k * M_COUNT, (size_t)k * T_COUNT));
    const size_t tail_at = (size_t)k * M_COUNT * kMaxGrid;
    double* tail = s + tail_at;
    const hipStream_t st = L.st;
    const double thr = rtol * rtol;

    // the directions start at zero: the first two updates multiply them by eps = 0 and delta = 0
    HIP_TRY(hipMemsetAsync(w[0], 0, (size_t)n * k * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(w[1], 0, (size_t)n * k * sizeof(double), st));
    // Q = A X0, walked last to first so that the first iteration's first-to-last walk starts on what it left in the cache
    int rc = ehyb_spmm(P, X, ldx, q, n, k, st, EHYB_WALK_LAST_TO_FIRST);
    if (rc != EHYB_OK) return rc;
    for_each_group(k, [&](auto K, int c0) {
        hipLaunchKernelGGL(minres_init_kernel<decltype(K)::value>, dim3(grid), dim3(kThreads), 0, st, n, B, (long long)ldb, q, dinv, r[0],
                           z, s, c0);
    });
    HIP_TRY(L.read());
    std::vector<double> bb(k), phibar(k);
    std::vector<int> f((size_t)k * F_COUNT, 0);  // {status, iterations} per column, as on the device
    auto is_converged = [&](int j) { return phibar[j] * phibar[j] <= thr * bb[j]; };
    int n_running = 0;
    for (int j = 0; j < k; ++j) {
        const double bb0 = device_order_sum(&L.h[(size_t)(j * M_COUNT + M_BB) * kMaxGrid], grid);
        const double b2 = device_order_sum(&L.h[(size_t)(j * M_COUNT + M_BETA0) * kMaxGrid], grid);
        bb[j] = bb0 > 0 ? bb0 : 1.0;
        phibar[j] = std::sqrt(b2);
        const bool finite = std::isfinite(bb0) && std::isfinite(b2);
        const int status = !finite ? ST_BREAKDOWN : is_converged(j) ? ST_CONVERGED : !(b2 > 0) ? ST_BREAKDOWN : ST_RUNNING;
        double* t = &L.h[tail_at + (size_t)j * T_COUNT];
        std::memset(t, 0, T_COUNT * sizeof(double));
        t[S_PHIBAR] = phibar[j];
        t[S_CS] = -1.0;
        f[j * F_COUNT + F_STATUS] = status;
        std::memcpy(t + T_FLAGS, &f[j * F_COUNT], F_COUNT * sizeof(int));
        n_running += status == ST_RUNNING;
    }
    HIP_TRY(hipMemcpyAsync(tail, &L.h[tail_at], (size_t)k * T_COUNT * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));

    // An even and an odd iteration -- two multiplies walking first to last, then last to first -- are one graph; the plain
    // launches use the same walks.
    int it = 0;
    rc = L.run(
        P, max_iter, it, [&] { return n_running > 0; },
        [&](int cur, bool) -> int {
            const int e = ehyb_spmm(P, z, n, q, n, k, st, cur == 0 ? EHYB_WALK_FIRST_TO_LAST : EHYB_WALK_LAST_TO_FIRST);  // stopped columns included
            if (e != EHYB_OK) return e;
            for_each_group(k, [&](auto K, int c0) {
                launch_iteration<decltype(K)::value>(grid, st, n, q, r[cur], r[cur ^ 1], dinv, z, w[cur ^ 1], w[cur], X, (long long)ldx, s,
                                                     tail, c0, cur, thr);
            });
            return EHYB_OK;
        },
        [&](int) -> int {
            n_running = 0;
            for (int j = 0; j < k; ++j) {
                const double* t = &L.h[tail_at + (size_t)j * T_COUNT];
                std::memcpy(&f[j * F_COUNT], t + T_FLAGS, F_COUNT * sizeof(int));
                phibar[j] = t[(f[j * F_COUNT + F_ITERS] & 1) * S_COUNT + S_PHIBAR];  // the copy the last update wrote
                n_running += f[j * F_COUNT + F_STATUS] == ST_RUNNING && !is_converged(j);  // the test the next dot kernel would make
            }
            return EHYB_OK;
        });
    if (rc != EHYB_OK) return rc;
    int broke = -1;
    for (int j = k - 1; j >= 0; --j) {
        if (iters_done) iters_done[j] = f[j * F_COUNT + F_ITERS];
        if (rel_residual) rel_residual[j] = phibar[j] / std::sqrt(bb[j]);
        if (f[j * F_COUNT + F_STATUS] == ST_BREAKDOWN) broke = j;
    }
    if (broke < 0) return EHYB_OK;
    const int done = f[broke * F_COUNT + F_ITERS];
    const char* what = "a non-finite b.b, z.q, beta^2 or gamma, a negative beta^2 or a zero gamma";
    if (name_column) EHYB_FAIL(EHYB_ERR_ARG, "%s: breakdown in column %d after %d iterations (%s)", who, broke, done, what);
    EHYB_FAIL(EHYB_ERR_ARG, "%s: breakdown after %d iterations (%s)", who, done, what);
}

}  // namespace

extern "C" int ehyb_minres(ehyb_plan* P, const double* dinv, const double* b, double* x, int max_iter, double rtol, int check_every,
                           void* stream, int* iters_done, double* rel_residual)
{
    const int rc = solve_prologue("ehyb_minres", P, b && x, max_iter, rtol);
    if (rc != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    return minres_solve("ehyb_minres", false, P, dinv, b, n, x, n, 1, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

// k right-hand sides, one multiply per iteration
extern "C" int ehyb_minres_multi(ehyb_plan* P, const double* dinv, const double* B, int64_t ldb, double* X, int64_t ldx, int k,
                                 int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const int rc = multi_prologue("ehyb_minres_multi", P, B && X, ldb, ldx, k, max_iter, rtol);
    if (rc != EHYB_OK) return rc;
    return minres_solve("ehyb_minres_multi", true, P, dinv, B, ldb, X, ldx, k, max_iter, rtol, check_every, stream, iters_done,
                        rel_residual);
}

// ------------------------------------------------------------------ building blocks for a caller that owns the loop
// The four vector kernels above at K = 1, one launch each, for a caller that issues the multiplies itself (and for tests that
// look at one kernel at a time) -- the analogue of ehyb_bicgstab_*_step.  s: `slots` slots of `slot_doubles` doubles and
// tail_doubles more behind them (ehyb_minres_layout); every launch uses slot_doubles / 2 workgroups.  Asynchronous on `stream`.
extern "C" int ehyb_minres_layout(ehyb_minres_slots* out)
{
    if (!out) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_minres_layout: null argument");
    out->slots = M_COUNT;
    out->slot_doubles = kMaxGrid;
    out->slot_bb = M_BB;
    out->slot_zq = M_ZQ;
    out->slot_beta0 = M_BETA0;
    out->tail_doubles = T_COUNT;
    out->state_doubles = S_COUNT;
    out->state_dbar = S_DBAR;
    out->state_eps = S_EPS;
    out->state_phibar = S_PHIBAR;
    out->state_cs = S_CS;
    out->state_sn = S_SN;
    out->state_beta_old = S_BETA_OLD;
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

inline double* step_tail(double* s) { return s + (size_t)M_COUNT * kMaxGrid; }

}  // namespace

extern "C" int ehyb_minres_init_step(int n, const double* b, const double* q, const double* dinv, double* r, double* z, double* s,
                                     void* stream)
{
    int rc = check_step("ehyb_minres_init_step", n, {b, q, r, z, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(minres_init_kernel<1>, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, b, (long long)n, q, dinv, r, z,
                       s, 0);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_minres_dot_step(int n, const double* z, const double* q, double* s, int cur, double thr, void* stream)
{
    int rc = check_step("ehyb_minres_dot_step", n, {z, q, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL((minres_dot_kernel<1, kDotU>), dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, z, q, s, step_tail(s), 0,
                       cur & 1, thr);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_minres_lanczos_step(int n, const double* q, const double* ra, double* rb, const double* dinv, double* z, double* s,
                                        int cur, void* stream)
{
    int rc = check_step("ehyb_minres_lanczos_step", n, {q, ra, rb, z, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL((minres_lanczos_kernel<1, lanczos_depth(1)>), dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, q, ra, rb,
                       dinv, z, s, step_tail(s), 0, cur & 1);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_minres_update_step(int n, const double* ra, const double* dinv, const double* wa, double* wb, double* x, double* s,
                                       int cur, void* stream)
{
    int rc = check_step("ehyb_minres_update_step", n, {ra, wa, wb, x, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL((minres_update_kernel<1, update_depth(1)>), dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, ra, dinv, wa,
                       wb, x, (long long)n, s, step_tail(s), 0, cur & 1);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
