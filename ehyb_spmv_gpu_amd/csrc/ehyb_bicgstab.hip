// Device-resident BiCGSTAB for unsymmetric systems on top of the EHYB plan (ehyb_bicgstab), right-preconditioned with
// M = diag(A) applied on the fly from 1/diag.  Only the preconditioned directions p^ = M^-1 p and s^ = M^-1 s are stored.
//
// Per iteration two multiplies and five vector kernels, each one grid-stride pass writing one partial sum per workgroup:
//   1. v = A p^                                                  (ehyb_spmv_walk, first to last)
//   2. partials of rh.v                                          (rh: the shadow residual r0)
//   3. alpha = rho / rh.v;  s = r - alpha v;  s^ = M^-1 s;       partials of s.s
//   4. t = A s^                                                  (ehyb_spmv_walk, last to first)
//   5. partials of t.s and t.t
//   6. omega = t.s / t.t;  x += alpha p^ + omega s^;  r = s - omega t;  partials of rho_new = rh.r and r.r
//      (half step: s.s <= rtol^2 b.b -> x += alpha p^, r = s)
//   7. beta = (rho_new / rho) (alpha / omega);  p^ = M^-1 r + beta (p^ - omega M^-1 v);  the stop test
// Every kernel recomputes the scalars it needs from partials still in their slots (vec_reduce.h: the same fixed order in
// every workgroup, so every workgroup takes the same decision); no scalar is carried from kernel to kernel.  rho alternates
// between two slots, so an even and an odd iteration differ in one kernel argument and are captured together into one hipGraph.
//
// Stopping and breakdown are decided on the device: a status word and an iteration counter sit behind the partial slots.
// Once the status is set every vector kernel returns at once; the multiplies of the rest of the burst run on vectors that no
// longer change.  A kernel that sets the status writes nothing else, so a workgroup that already sees the status its own
// launch set does what it would have done anyway.  The half step is the exception -- it updates x and r -- so step 6 does
// not set the status for it; step 7 sees the same s.s and sets it.  The host reads partials, status and counter at check
// points only.
//
// k right-hand sides (ehyb_bicgstab_multi) are k such solves that share the two multiplies (ehyb_spmm): the vector kernels are
// templated on K columns per launch, every column with its own slots, status word and counter, and K = 1 is the one-vector solve.
// The host side is written once too: bicgstab_solve drives k columns, ehyb_bicgstab is its own argument check and that driver at
// k = 1, ehyb_bicgstab_multi the k and leading-dimension checks and the driver.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "bilu.h"
#include "ehyb_internal.h"
#include "solve_loop.h"
#include "vec_walk.h"

using namespace ehyb;

namespace {

// partial slots, kMaxGrid doubles each; rho number c = r^.r of iterations of parity c lives in slot B_RHO0 + 2 c.  Column j's
// set of slots starts at s + j * B_COUNT * kMaxGrid; behind the last set two ints per column: the status word and the device's
// iteration counter.  One column is the layout of ehyb_bicgstab_layout.
enum { B_BB = 0, B_RV = 1, B_SS = 2, B_TS = 3, B_TT = 4, B_RHO0 = 5, B_RR = 6, B_RHO1 = 7, B_COUNT = 8 };

// column col's status word and counter, for running and set_status (vec_reduce.h)
template <class I>
__device__ __forceinline__ auto column_flags(I* __restrict__ flags)
{
    return [=](int col) { return flags + col * F_COUNT; };
}

// ------------------------------------------------------------------ the vector kernels, K columns per launch
// Columns c0 .. c0 + K - 1 of vectors with leading dimension n (B: ldb, X: ldx); K <= 4 per launch (kMultiMaxK, for_each_group
// of solve_loop.h), K = 1 for the one-vector solve and the ehyb_bicgstab_*_step building blocks.  The walk is vec_walk.h's, U grid
// strides per trip, so a column's partials and scalars are the one-vector solve's bits.  A column whose status is set is
// skipped: its vectors and partials stay as they are.

// r = b - q (q = A x0), r^ = r, p^ = M^-1 r; partials of rho = r^.r, r.r, b.b.  Takes no flags: they are zero at the start.
template <int K>
__global__ __launch_bounds__(kThreads) void bicg_init_kernel(int n, const double* __restrict__ B, long long ldb,
                                                             const double* __restrict__ Q, const double* __restrict__ dinv,
                                                             double* __restrict__ R, double* __restrict__ RH, double* __restrict__ P,
                                                             double* __restrict__ s, int c0)
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
            R[o] = ri;
            RH[o] = ri;
            P[o] = dinv ? ri * di : ri;
            sums[c] = fma(ri, ri, sums[c]);
            sums[K + c] = fma(bi, bi, sums[K + c]);
        }
    }
    block_sum_n(sums);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            slot<B_COUNT>(s, c0 + c, B_RHO0)[blockIdx.x] = sums[c];
            slot<B_COUNT>(s, c0 + c, B_RR)[blockIdx.x] = sums[c];
            slot<B_COUNT>(s, c0 + c, B_BB)[blockIdx.x] = sums[K + c];
        }
    }
}

// step 2: partials of r^.v
template <int K, int U>
__global__ __launch_bounds__(kThreads) void bicg_dot_kernel(int n, const double* __restrict__ RH, const double* __restrict__ V,
                                                            double* __restrict__ s, const int* __restrict__ flags, int c0)
{
    bool on[K];
    if (!running<K>(column_flags(flags), c0, on)) return;
    const double* rh[K];
    const double* v[K];
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        rh[c] = RH + (size_t)(c0 + c) * n;
        v[c] = V + (size_t)(c0 + c) * n;
        acc[c] = 0.0;
    }
    walk<K, U, 2>(
        n, on, NoShared{},
        [&](int c, int i, double(&in)[2], int) {
            in[0] = rh[c][i];
            in[1] = v[c][i];
        },
        [&](int c, int, const double(&in)[2], int) { acc[c] = fma(in[0], in[1], acc[c]); });
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<B_COUNT>(s, c0 + c, B_RV)[blockIdx.x] = acc[c];
    }
}

// step 3: alpha = rho / r^.v;  s = r - alpha v;  s^ = M^-1 s;  partials of s.s
template <int K, int U>
__global__ __launch_bounds__(kThreads) void bicg_s_kernel(int n, const double* __restrict__ R, const double* __restrict__ V,
                                                          const double* __restrict__ dinv, double* __restrict__ SV,
                                                          double* __restrict__ SH, double* __restrict__ s, int* __restrict__ flags,
                                                          int c0, int cur)
{
    bool on[K];
    if (!running<K>(column_flags(flags), c0, on)) return;
    double sums[2 * K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        sums[c] = on[c] ? partials_of(slot<B_COUNT>(s, c0 + c, B_RHO0 + 2 * cur)) : 0.0;
        sums[K + c] = on[c] ? partials_of(slot<B_COUNT>(s, c0 + c, B_RV)) : 0.0;
    }
    block_sum_n(sums);
    double alpha[K], ss[K];
    const double* r[K];
    const double* v[K];
    double* sv[K];
    double* sh[K];
    bool any = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        r[c] = R + (size_t)(c0 + c) * n;
        v[c] = V + (size_t)(c0 + c) * n;
        sv[c] = SV + (size_t)(c0 + c) * n;
        sh[c] = SH + (size_t)(c0 + c) * n;
        ss[c] = 0.0;
        const double rho = sums[c], rv = sums[K + c];
        alpha[c] = rho / rv;
        if (on[c] && uniform(!isfinite(rho) || !usable_divisor(rv) || !isfinite(alpha[c]))) {
            set_status(column_flags(flags), c0 + c, ST_BREAKDOWN);
            on[c] = false;
        }
        any = any || on[c];
    }
    if (!any) return;
    walk<K, U, 2>(
        n, on, InvDiag{dinv},
        [&](int c, int i, double(&in)[2], double) {
            in[0] = r[c][i];
            in[1] = v[c][i];
        },
        [&](int c, int i, const double(&in)[2], double di) {
            const double si = fma(-alpha[c], in[1], in[0]);
            sv[c][i] = si;
            sh[c][i] = dinv ? si * di : si;
            ss[c] = fma(si, si, ss[c]);
        });
    block_sum_n(ss);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<B_COUNT>(s, c0 + c, B_SS)[blockIdx.x] = ss[c];
    }
}

// step 5: partials of t.s and t.t in one pass
template <int K, int U>
__global__ __launch_bounds__(kThreads) void bicg_dot2_kernel(int n, const double* __restrict__ T, const double* __restrict__ SV,
                                                             double* __restrict__ s, const int* __restrict__ flags, int c0)
{
    bool on[K];
    if (!running<K>(column_flags(flags), c0, on)) return;
    const double* t[K];
    const double* sv[K];
    double acc[2 * K];  // t.s of the K columns, then t.t
#pragma unroll
    for (int c = 0; c < K; ++c) {
        t[c] = T + (size_t)(c0 + c) * n;
        sv[c] = SV + (size_t)(c0 + c) * n;
        acc[c] = acc[K + c] = 0.0;
    }
    walk<K, U, 2>(
        n, on, NoShared{},
        [&](int c, int i, double(&in)[2], int) {
            in[0] = t[c][i];
            in[1] = sv[c][i];
        },
        [&](int c, int, const double(&in)[2], int) {
            acc[c] = fma(in[0], in[1], acc[c]);
            acc[K + c] = fma(in[0], in[0], acc[K + c]);
        });
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!on[c]) continue;
            slot<B_COUNT>(s, c0 + c, B_TS)[blockIdx.x] = acc[c];
            slot<B_COUNT>(s, c0 + c, B_TT)[blockIdx.x] = acc[K + c];
        }
    }
}

// step 6: omega = t.s / t.t;  x += alpha p^ + omega s^;  r = s - omega t;  partials of rho_new = r^.r (the other rho slot)
// and r.r; the counter advances.  Half step (s.s <= thr b.b): x += alpha p^, r = s, partials of r.r only.  Each column takes
// its own way: the half-step columns first, one plain pass each, then the full updates together.
template <int K, int U>
__global__ __launch_bounds__(kThreads) void bicg_update_kernel(int n, const double* __restrict__ P, const double* __restrict__ SH,
                                                               const double* __restrict__ SV, const double* __restrict__ T,
                                                               const double* __restrict__ RH, double* __restrict__ X, long long ldx,
                                                               double* __restrict__ R, double* __restrict__ s,
                                                               int* __restrict__ flags, int c0, int cur, double thr)
{
    bool on[K];
    if (!running<K>(column_flags(flags), c0, on)) return;
    constexpr int slots[6] = {B_RHO0, B_RV, B_SS, B_BB, B_TS, B_TT};  // (B_RHO0: + 2 cur)
    double sums[6 * K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
#pragma unroll
        for (int w = 0; w < 6; ++w) sums[w * K + c] = on[c] ? partials_of(slot<B_COUNT>(s, c0 + c, slots[w] + (w == 0 ? 2 * cur : 0))) : 0.0;
    }
    block_sum_n(sums);
    const double* p[K];
    const double* sh[K];
    const double* sv[K];
    const double* t[K];
    const double* rh[K];
    double* x[K];
    double* r[K];
    double alpha[K], omega[K], rho[K], rr[K];
    bool half[K], full[K], any = false, any_half = false;
    const int stride = (int)gridDim.x * kThreads;
    const int i0 = blockIdx.x * kThreads + threadIdx.x;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        p[c] = P + (size_t)(c0 + c) * n;
        sh[c] = SH + (size_t)(c0 + c) * n;
        sv[c] = SV + (size_t)(c0 + c) * n;
        t[c] = T + (size_t)(c0 + c) * n;
        rh[c] = RH + (size_t)(c0 + c) * n;
        r[c] = R + (size_t)(c0 + c) * n;
        x[c] = X + (size_t)(c0 + c) * ldx;
        rho[c] = rr[c] = 0.0;
        alpha[c] = sums[c] / sums[K + c];
        const double bb = sums[3 * K + c] > 0 ? sums[3 * K + c] : 1.0, tt = sums[5 * K + c];
        omega[c] = sums[4 * K + c] / tt;
        half[c] = on[c] && uniform(sums[2 * K + c] <= thr * bb);  // s is small enough
        full[c] = on[c] && !half[c];
        if (full[c] && uniform(!usable_divisor(tt) || !isfinite(omega[c]))) {
            set_status(column_flags(flags), c0 + c, ST_BREAKDOWN);
            full[c] = false;
        }
        any = any || full[c];
        any_half = any_half || half[c];
        if (half[c]) {
            for (int i = i0; i < n; i += stride) {
                const double si = __builtin_nontemporal_load(&sv[c][i]);
                x[c][i] = fma(alpha[c], p[c][i], x[c][i]);
                r[c][i] = si;
                rr[c] = fma(si, si, rr[c]);
            }
        }
    }
    if (any) {
        enum { PV, SHV, SVV, TV, XV, RHV, NV };
        walk<K, U, NV>(
            n, full, NoShared{},
            [&](int c, int i, double(&in)[NV], int) {
                in[PV] = p[c][i];
                in[SHV] = __builtin_nontemporal_load(&sh[c][i]);  // s^, s and t are dead after this kernel, x is not
                in[SVV] = __builtin_nontemporal_load(&sv[c][i]);  // read again before the next update: streamed
                in[TV] = __builtin_nontemporal_load(&t[c][i]);    // past the caches, which hold the matrix's tail
                in[XV] = __builtin_nontemporal_load(&x[c][i]);
                in[RHV] = rh[c][i];
            },
            [&](int c, int i, const double(&in)[NV], int) {
                __builtin_nontemporal_store(fma(omega[c], in[SHV], fma(alpha[c], in[PV], in[XV])), &x[c][i]);
                const double ri = fma(-omega[c], in[TV], in[SVV]);
                r[c][i] = ri;
                rho[c] = fma(in[RHV], ri, rho[c]);
                rr[c] = fma(ri, ri, rr[c]);
            });
    }
    if (!any && !any_half) return;
    double out[2 * K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        out[c] = rho[c];
        out[K + c] = rr[c];
    }
    block_sum_n(out);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!half[c] && !full[c]) continue;
            if (full[c]) slot<B_COUNT>(s, c0 + c, B_RHO0 + 2 * (cur ^ 1))[blockIdx.x] = out[c];
            slot<B_COUNT>(s, c0 + c, B_RR)[blockIdx.x] = out[K + c];
            if (blockIdx.x == 0) flags[(c0 + c) * F_COUNT + F_ITERS] += 1;
        }
    }
}

// step 7: the stop test (converged: the half step was taken, or r.r <= thr b.b), then beta = (rho_new / rho) (alpha / omega)
// and p^ = M^-1 r + beta (p^ - omega M^-1 v)
template <int K, int U>
__global__ __launch_bounds__(kThreads) void bicg_direction_kernel(int n, const double* __restrict__ R, const double* __restrict__ V,
                                                                  const double* __restrict__ dinv, double* __restrict__ P,
                                                                  const double* __restrict__ s, int* __restrict__ flags, int c0,
                                                                  int cur, double thr)
{
    bool on[K];
    if (!running<K>(column_flags(flags), c0, on)) return;
    constexpr int slots[8] = {B_SS, B_RR, B_BB, B_RHO0, B_RHO0, B_RV, B_TS, B_TT};  // (the B_RHO0s: + 2 cur, + 2 (cur ^ 1))
    double sums[8 * K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
#pragma unroll
        for (int w = 0; w < 8; ++w)
            sums[w * K + c] = on[c] ? partials_of(slot<B_COUNT>(s, c0 + c, slots[w] + (w == 3 ? 2 * cur : w == 4 ? 2 * (cur ^ 1) : 0))) : 0.0;
    }
    block_sum_n(sums);
    const double* r[K];
    const double* v[K];
    double* p[K];
    double omega[K], beta[K];
    bool any = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        r[c] = R + (size_t)(c0 + c) * n;
        v[c] = V + (size_t)(c0 + c) * n;
        p[c] = P + (size_t)(c0 + c) * n;
        const double bb = sums[2 * K + c] > 0 ? sums[2 * K + c] : 1.0;
        const double rho = sums[3 * K + c], rho_new = sums[4 * K + c], alpha = rho / sums[5 * K + c];
        omega[c] = sums[6 * K + c] / sums[7 * K + c];
        beta[c] = (rho_new / rho) * (alpha / omega[c]);
        if (on[c] && uniform(sums[c] <= thr * bb || sums[K + c] <= thr * bb)) {
            set_status(column_flags(flags), c0 + c, ST_CONVERGED);
            on[c] = false;
        }
        if (on[c] && uniform(!usable_divisor(rho) || !usable_divisor(omega[c]) || !isfinite(rho_new) || !isfinite(beta[c]))) {
            set_status(column_flags(flags), c0 + c, ST_BREAKDOWN);
            on[c] = false;
        }
        any = any || on[c];
    }
    if (!any) return;
    walk<K, U, 3>(
        n, on, InvDiag{dinv},
        [&](int c, int i, double(&in)[3], double) {
            in[0] = p[c][i];
            in[1] = r[c][i];
            in[2] = __builtin_nontemporal_load(&v[c][i]);  // v is dead after this kernel
        },
        [&](int c, int i, const double(&in)[3], double di) {
            const double zi = dinv ? in[1] * di : in[1], wi = dinv ? in[2] * di : in[2];
            p[c][i] = fma(beta[c], fma(-omega[c], wi, in[0]), zi);
        });
}

// grid strides per trip: four wherever the loads of a trip fit the registers, fewer for the wide update and direction kernels
// (update: six vectors per column; at four strides and four columns its loads alone would be 192 doubles)
constexpr int kDotU = 4;
constexpr int s_depth(int K) { return K <= 2 ? 4 : 2; }
constexpr int update_depth(int K) { return K == 1 ? 4 : K == 2 ? 2 : 1; }
constexpr int direction_depth(int K) { return K <= 2 ? 4 : 2; }

// what one iteration launches for columns c0 .. c0 + K - 1 between its multiplies: after v = A p^ ...
template <int K>
void launch_after_v(int grid, hipStream_t st, int n, const double* r, const double* rh, const double* v, const double* dinv, double* sv,
                    double* sh, double* s, int* flags, int c0, int cur)
{
    hipLaunchKernelGGL((bicg_dot_kernel<K, kDotU>), dim3(grid), dim3(kThreads), 0, st, n, rh, v, s, flags, c0);
    hipLaunchKernelGGL((bicg_s_kernel<K, s_depth(K)>), dim3(grid), dim3(kThreads), 0, st, n, r, v, dinv, sv, sh, s, flags, c0, cur);
}

// ... and after t = A s^ (ph: the p^ of the update, p: what the direction kernel advances -- the same vector but for ehyb_bicgstab_bilu)
template <int K>
void launch_after_t(int grid, hipStream_t st, int n, const double* ph, double* p, const double* sh, const double* sv, const double* t, const double* rh,
                    const double* v, const double* dinv, double* x, long long ldx, double* r, double* s, int* flags, int c0, int cur,
                    double thr)
{
    hipLaunchKernelGGL((bicg_dot2_kernel<K, kDotU>), dim3(grid), dim3(kThreads), 0, st, n, t, sv, s, flags, c0);
    hipLaunchKernelGGL((bicg_update_kernel<K, update_depth(K)>), dim3(grid), dim3(kThreads), 0, st, n, ph, sh, sv, t, rh, x, ldx, r, s,
                       flags, c0, cur, thr);
    hipLaunchKernelGGL((bicg_direction_kernel<K, direction_depth(K)>), dim3(grid), dim3(kThreads), 0, st, n, r, v, dinv, p, s, flags,
                       c0, cur, thr);
}

// The one driver: k solves that share v = A p^ and t = A s^ (ehyb_spmm with explicit walks; its pass of width 1 is ehyb_spmv_walk,
// so k = 1 launches the one-vector sequence: the multiplies, one <1> launch per vector kernel, and the one-vector workspace).  Every
// column has its own slots, status word and counter and is decided on the device; the host reads all of them at a check point and
// goes on while any column is running.  A column that has nothing to do at the start, or a non-finite start, gets its status
// planted before the first burst -- where some column does start and some does not, so never at k = 1.  The entry points have
// made their checks (solve_loop.h); who: the entry point, name_column: whether the breakdown text says which column.
//   M (ehyb_bicgstab_bilu): the textbook right-preconditioned form with a general M.  The kernels run with dinv = NULL, which makes
// them the unpreconditioned recurrences -- p = r + beta (p - omega v) on the unpreconditioned p, s = r - alpha v --, and the apply
// kernel of ehyb_bic makes p^ = M^-1 p (one more vector) before v = A p^ and s^ = M^-1 s (over the copy of s the s kernel left in
// s^) before t = A s^; the update kernel reads p^ and s^ as ever.  The apply reads the columns' status words as the vector kernels
// do: a stopped column is skipped, its p^ and s^ stay.
int bicgstab_solve(const char* who, bool name_column, ehyb_plan* P, const double* dinv, const ehyb_bilu* M, const double* B, int64_t ldb, double* X,
                   int64_t ldx, int k, int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const int n = P->host.n_cols;
    SolveLoop L(n, check_every);
    const int grid = L.grid;
    double *r, *rh, *p, *v, *sv, *sh, *t, *s;
    // two ints per column behind the k sets of slots: one double each
    HIP_TRY(L.begin(stream, {&r, &rh, &p, &v, &sv, &sh, &t}, (size_t)n * k, &s, (size_t)k * B_COUNT, k));
    double* ph = p;
    if (M) HIP_TRY(L.more(&ph, (size_t)n * k));
    const size_t flags_at = (size_t)k * B_COUNT * kMaxGrid;
    int* flags = (int*)(s + flags_at);
    const hipStream_t st = L.st;
    const double thr = rtol * rtol;

    HIP_TRY(hipMemsetAsync(flags, 0, (size_t)k * F_COUNT * sizeof(int), st));
    // V = A X0, walked last to first so that the first iteration's first-to-last walk starts on what it left in the cache
    int rc = ehyb_spmm(P, X, ldx, v, n, k, st, EHYB_WALK_LAST_TO_FIRST);
    if (rc != EHYB_OK) return rc;
    for_each_group(k, [&](auto K, int c0) {
        hipLaunchKernelGGL(bicg_init_kernel<decltype(K)::value>, dim3(grid), dim3(kThreads), 0, st, n, B, (long long)ldb, v, dinv, r, rh,
                           p, s, c0);
    });
    HIP_TRY(L.read());
    std::vector<double> bb(k), rr(k);
    std::vector<int> f((size_t)k * F_COUNT, 0);  // {status, iterations} per column, as on the device
    int n_running = 0;
    for (int j = 0; j < k; ++j) {
        const double bb0 = L.sum(j * B_COUNT + B_BB);
        bb[j] = bb0 > 0 ? bb0 : 1.0;
        rr[j] = L.sum(j * B_COUNT + B_RR);
        const int status = !std::isfinite(bb0) || !std::isfinite(rr[j]) ? ST_BREAKDOWN : rr[j] <= thr * bb[j] ? ST_CONVERGED : ST_RUNNING;
        f[j * F_COUNT + F_STATUS] = status;
        n_running += status == ST_RUNNING;
    }
    if (n_running > 0 && n_running < k && max_iter > 0) {  // the columns that do not start: their status before the first burst
        HIP_TRY(hipMemcpyAsync(flags, f.data(), f.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
    }

    // An even and an odd iteration -- four multiplies walking first to last, last to first, first to last, last to first --
    // are one graph; the plain launches use the same walks.
    int it = 0;
    rc = L.run(
        P, max_iter, it, [&] { return n_running > 0; },
        [&](int cur, bool) -> int {
            int e = M ? bic_apply_columns(&M->core, st, p, n, ph, n, k, flags + F_STATUS, F_COUNT, true) : EHYB_OK;  // P^ = M^-1 P
            if (e != EHYB_OK) return e;
            if ((e = ehyb_spmm(P, ph, n, v, n, k, st, EHYB_WALK_FIRST_TO_LAST)) != EHYB_OK) return e;  // V = A P^, stopped columns included
            for_each_group(k, [&](auto K, int c0) { launch_after_v<decltype(K)::value>(grid, st, n, r, rh, v, dinv, sv, sh, s, flags, c0, cur); });
            if (M && (e = bic_apply_columns(&M->core, st, sv, n, sh, n, k, flags + F_STATUS, F_COUNT, true)) != EHYB_OK) return e;  // S^ = M^-1 S
            if ((e = ehyb_spmm(P, sh, n, t, n, k, st, EHYB_WALK_LAST_TO_FIRST)) != EHYB_OK) return e;  // T = A S^
            for_each_group(k, [&](auto K, int c0) {
                launch_after_t<decltype(K)::value>(grid, st, n, ph, p, sh, sv, t, rh, v, dinv, X, ldx, r, s, flags, c0, cur, thr);
            });
            return EHYB_OK;
        },
        [&](int) -> int {
            std::memcpy(f.data(), &L.h[flags_at], f.size() * sizeof(int));
            n_running = 0;
            for (int j = 0; j < k; ++j) {
                rr[j] = L.sum(j * B_COUNT + B_RR);
                n_running += f[j * F_COUNT + F_STATUS] == ST_RUNNING;
            }
            return EHYB_OK;
        });
    if (rc != EHYB_OK) return rc;
    int broke = -1;
    for (int j = k - 1; j >= 0; --j) {
        if (iters_done) iters_done[j] = f[j * F_COUNT + F_ITERS];
        if (rel_residual) rel_residual[j] = std::sqrt(rr[j] / bb[j]);
        if (f[j * F_COUNT + F_STATUS] == ST_BREAKDOWN) broke = j;
    }
    if (broke < 0) return EHYB_OK;
    const int done = f[broke * F_COUNT + F_ITERS];
    const char* what = "a zero or non-finite rho, r^.v, t.t or omega";
    if (name_column) EHYB_FAIL(EHYB_ERR_ARG, "%s: breakdown in column %d after %d iterations (%s)", who, broke, done, what);
    EHYB_FAIL(EHYB_ERR_ARG, "%s: breakdown after %d iterations (%s)", who, done, what);
}

}  // namespace

extern "C" int ehyb_bicgstab(ehyb_plan* P, const double* dinv, const double* b, double* x, int max_iter, double rtol,
                             int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const int rc = solve_prologue("ehyb_bicgstab", P, b && x, max_iter, rtol);
    if (rc != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    return bicgstab_solve("ehyb_bicgstab", false, P, dinv, nullptr, b, n, x, n, 1, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

// k right-hand sides, two multiplies per iteration
extern "C" int ehyb_bicgstab_multi(ehyb_plan* P, const double* dinv, const double* B, int64_t ldb, double* X, int64_t ldx, int k,
                                   int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const int rc = multi_prologue("ehyb_bicgstab_multi", P, B && X, ldb, ldx, k, max_iter, rtol);
    if (rc != EHYB_OK) return rc;
    return bicgstab_solve("ehyb_bicgstab_multi", true, P, dinv, nullptr, B, ldb, X, ldx, k, max_iter, rtol, check_every, stream, iters_done,
                          rel_residual);
}

// right-preconditioned with the block ILU(0) of `bilu`; the checks: what ehyb_bicgstab(_multi) rejects, the factor, the uploads
extern "C" int ehyb_bicgstab_bilu(ehyb_plan* P, ehyb_bilu* bilu, const double* b, double* x, int max_iter, double rtol, int check_every,
                                  void* stream, int* iters_done, double* rel_residual)
{
    const char* who = "ehyb_bicgstab_bilu";
    int rc = solve_args(who, P, b && x, max_iter, rtol);
    if (rc != EHYB_OK || (rc = bilu_solver_args(who, P, bilu)) != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    return bicgstab_solve(who, false, P, nullptr, bilu, b, n, x, n, 1, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

extern "C" int ehyb_bicgstab_bilu_multi(ehyb_plan* P, ehyb_bilu* bilu, const double* B, int64_t ldb, double* X, int64_t ldx, int k, int max_iter,
                                        double rtol, int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const char* who = "ehyb_bicgstab_bilu_multi";
    int rc = multi_args(who, P, ldb, ldx, k);
    if (rc == EHYB_OK) rc = solve_args(who, P, B && X, max_iter, rtol);
    if (rc != EHYB_OK || (rc = bilu_solver_args(who, P, bilu)) != EHYB_OK) return rc;
    return bicgstab_solve(who, true, P, nullptr, bilu, B, ldb, X, ldx, k, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

// ------------------------------------------------------------------ building blocks for a caller that owns the loop
// The six vector kernels above at K = 1, one launch each, for a caller that issues the multiplies itself (and for tests that
// look at one kernel at a time) -- the analogue of ehyb_cg_*_step.  s: `slots` slots of `slot_doubles` doubles and one more
// double behind them, whose two ints are the status word and the iteration counter (ehyb_bicgstab_layout); every launch uses
// slot_doubles / 2 workgroups.  Asynchronous on `stream`.
extern "C" int ehyb_bicgstab_layout(ehyb_bicgstab_slots* out)
{
    if (!out) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_bicgstab_layout: null argument");
    out->slots = B_COUNT;
    out->slot_doubles = kMaxGrid;
    out->slot_bb = B_BB;
    out->slot_rv = B_RV;
    out->slot_ss = B_SS;
    out->slot_ts = B_TS;
    out->slot_tt = B_TT;
    out->slot_rho0 = B_RHO0;
    out->slot_rr = B_RR;
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

inline int* flags_of(double* s) { return (int*)(s + (size_t)B_COUNT * kMaxGrid); }

}  // namespace

extern "C" int ehyb_bicgstab_init_step(int n, const double* b, const double* q, const double* dinv, double* r, double* rh, double* p,
                                       double* s, void* stream)
{
    int rc = check_step("ehyb_bicgstab_init_step", n, {b, q, r, rh, p, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(bicg_init_kernel<1>, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, b, (long long)n, q, dinv, r, rh,
                       p, s, 0);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_bicgstab_dot_step(int n, const double* rh, const double* v, double* s, void* stream)
{
    int rc = check_step("ehyb_bicgstab_dot_step", n, {rh, v, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL((bicg_dot_kernel<1, kDotU>), dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, rh, v, s, flags_of(s), 0);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_bicgstab_s_step(int n, const double* r, const double* v, const double* dinv, double* sv, double* sh, double* s,
                                    int cur, void* stream)
{
    int rc = check_step("ehyb_bicgstab_s_step", n, {r, v, sv, sh, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL((bicg_s_kernel<1, s_depth(1)>), dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, r, v, dinv, sv, sh, s,
                       flags_of(s), 0, cur & 1);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_bicgstab_dot2_step(int n, const double* t, const double* sv, double* s, void* stream)
{
    int rc = check_step("ehyb_bicgstab_dot2_step", n, {t, sv, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL((bicg_dot2_kernel<1, kDotU>), dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, t, sv, s, flags_of(s), 0);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_bicgstab_update_step(int n, const double* p, const double* sh, const double* sv, const double* t,
                                         const double* rh, double* x, double* r, double* s, int cur, double thr, void* stream)
{
    int rc = check_step("ehyb_bicgstab_update_step", n, {p, sh, sv, t, rh, x, r, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL((bicg_update_kernel<1, update_depth(1)>), dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, p, sh, sv, t,
                       rh, x, (long long)n, r, s, flags_of(s), 0, cur & 1, thr);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_bicgstab_direction_step(int n, const double* r, const double* v, const double* dinv, double* p, double* s, int cur,
                                            double thr, void* stream)
{
    int rc = check_step("ehyb_bicgstab_direction_step", n, {r, v, p, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL((bicg_direction_kernel<1, direction_depth(1)>), dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, r, v,
                       dinv, p, s, flags_of(s), 0, cur & 1, thr);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
