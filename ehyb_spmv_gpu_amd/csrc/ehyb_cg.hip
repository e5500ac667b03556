// Device-resident conjugate gradients on top of the EHYB plan (the iterative caller
// the reference repository was stripped down from).  Reference leftovers this stands in for:
// kernelMyxpy (y = x + gamma*y, kernel.cu:288-296), kernelInitializeAll / kernelInitializeR
// (kernel.cu:20-42), myxpy / initialize_all wrappers (kernel.cu:298-321).
//
// Per iteration: one ehyb_spmv (q = A p) and three memory-bound vector kernels, each a grid-stride
// pass over the vectors:
//   1. pq   = p . q
//   2. x += alpha p ; r -= alpha q ; rz_new = r . z ; rr = r . r   (alpha = rz / pq)
//   3. p  = z + beta p                                              (beta  = rz_new / rz)  [kernelMyxpy]
// with z = M^-1 r for the diagonal (Jacobi) preconditioner -- the PRECOND switch of the reference's
// cb_s (spmv.h:7-15) -- recomputed on the fly from 1/diag, or z = r without one.
//
// Dot products never leave the device and use no atomics: a kernel writes one partial sum per
// workgroup, and the kernel that needs the scalar adds the (at most 1024) partials up again in a
// fixed order -- every workgroup for itself, 8 KiB out of L2.  (A first version added the partials
// with one fp64 atomic per workgroup: 2048 same-address atomics cost 28 us per dot product,
// profiles/r01_j_cg.txt.)  Nothing has to be zeroed or rolled between iterations; r.z alternates
// between two partial arrays, so an even and an odd iteration differ in one kernel argument and
// are captured together into one hipGraph, replayed once per two iterations.  The sums have a
// fixed order, so a solve is reproducible run to run wherever the multiply is (plain storage).
// The host reads the partials every `check_every` iterations for the stopping test.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "cg_shared.h"
#include "ehyb_internal.h"
#include "solve_loop.h"
#include "vec_walk.h"

using namespace ehyb;

namespace {

// (the partial arrays of a column -- A_BB, A_PQ, A_RZ0, A_RR, A_RZ1 -- are cg_shared.h's: ehyb_cheb.hip uses the same layout)

// r = b - q (q = A x0), z = dinv .* r (or r), p = z; partials of r.z, r.r, b.b
__global__ __launch_bounds__(kThreads) void cg_init_kernel(int n, const double* __restrict__ b,
                                                           const double* __restrict__ q, const double* __restrict__ dinv,
                                                           double* __restrict__ r, double* __restrict__ p,
                                                           double* __restrict__ s)
{
    double rz = 0.0, rr = 0.0, bb = 0.0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const double bi = b[i], ri = bi - q[i];
        const double zi = dinv ? ri * dinv[i] : ri;
        r[i] = ri;
        p[i] = zi;
        rz = fma(ri, zi, rz);
        rr = fma(ri, ri, rr);
        bb = fma(bi, bi, bb);
    }
    put_partial(rz, s + A_RZ0 * kMaxGrid);
    put_partial(rr, s + A_RR * kMaxGrid);
    put_partial(bb, s + A_BB * kMaxGrid);
}

// ------------------------------------------------------------------ the vector kernels, K columns per launch
// One iteration of k independent solves on the same matrix that share every multiply (ehyb_pcg_multi) launches the three vector
// kernels K columns wide (K <= 4 per launch, ceil(k / 4) launches each); the one-vector solve (ehyb_pcg, and the ehyb_cg_*_step
// building blocks) launches them with K = 1.  Column j keeps its own alpha, beta and stopping test and its own set of partial
// slots (s + j * A_COUNT * kMaxGrid; column 0's set is the one-vector layout); the walk is vec_walk.h's at four strides per
// trip, so column j is ehyb_pcg(b_j) wherever the multiply is (plain storage).  A column whose active flag is 0 (converged or
// broken down) is skipped: its x, r, p and partials stay as they are.  A one-vector launch passes no flags (active = null: its
// column is live; K = 1 only, the wider kernels' code stays as it is).

// columns c0 .. c0 + K - 1: P, Q, R with leading dimension n, X with ldx.  pq = p . q
template <int K>
__global__ __launch_bounds__(kThreads) void cg_multi_dot_kernel(int n, const double* __restrict__ P, const double* __restrict__ Q,
                                                                double* __restrict__ s, const int* __restrict__ active, int c0)
{
    bool on[K];
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        acc[c] = 0.0;
    }
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const size_t o = (size_t)(c0 + c) * n + i;
            if (on[c]) acc[c] = fma(P[o], Q[o], acc[c]);
        }
    }
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<A_COUNT>(s, c0 + c, A_PQ)[blockIdx.x] = acc[c];
    }
}

// x += alpha p ; r -= alpha q ; rz_new = r . z ; rr = r . r  (alpha = rz / pq).  cur: which of the two r.z slots holds this
// iteration's r.z; the new one goes to the other
template <int K>
__global__ __launch_bounds__(kThreads) void cg_multi_update_kernel(int n, const double* __restrict__ P, const double* __restrict__ Q,
                                                                   const double* __restrict__ dinv, double* __restrict__ X, long long ldx,
                                                                   double* __restrict__ R, double* __restrict__ s,
                                                                   const int* __restrict__ active, int c0, int cur)
{
    bool on[K];
    double sums[2 * K], alpha[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        sums[c] = partials_of(slot<A_COUNT>(s, c0 + c, A_RZ0 + 2 * cur));
        sums[K + c] = partials_of(slot<A_COUNT>(s, c0 + c, A_PQ));
    }
    block_sum_n(sums);
    double rz[K], rr[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        alpha[c] = sums[c] / sums[K + c];
        rz[c] = rr[c] = 0.0;
    }
    const double* p[K];
    const double* q[K];
    double* x[K];
    double* r[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        p[c] = P + (size_t)(c0 + c) * n;
        q[c] = Q + (size_t)(c0 + c) * n;
        r[c] = R + (size_t)(c0 + c) * n;
        x[c] = X + (size_t)(c0 + c) * ldx;
    }
    // four grid strides per trip: sixteen (twenty with a preconditioner) loads in flight per thread and column instead of
    // four -- a thread sees only seven elements of the bench matrix's vectors, and one load round trip per element was most of
    // this kernel's time.  q is dead after this kernel and x is not read again before the next update: both streamed past the
    // caches, which hold the matrix's tail.
    walk<K, kWalkU, 4>(
        n, on, InvDiag{dinv},
        [&](int c, int i, double(&in)[4], double) {
            in[0] = p[c][i];
            in[1] = __builtin_nontemporal_load(&q[c][i]);
            in[2] = __builtin_nontemporal_load(&x[c][i]);
            in[3] = r[c][i];
        },
        [&](int c, int i, const double(&in)[4], double di) {
            __builtin_nontemporal_store(fma(alpha[c], in[0], in[2]), &x[c][i]);
            const double ri = fma(-alpha[c], in[1], in[3]);
            r[c][i] = ri;
            rz[c] = fma(ri, dinv ? ri * di : ri, rz[c]);
            rr[c] = fma(ri, ri, rr[c]);
        });
#pragma unroll
    for (int c = 0; c < K; ++c) {
        sums[c] = rz[c];
        sums[K + c] = rr[c];
    }
    block_sum_n(sums);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!on[c]) continue;
            slot<A_COUNT>(s, c0 + c, A_RZ0 + 2 * (cur ^ 1))[blockIdx.x] = sums[c];
            slot<A_COUNT>(s, c0 + c, A_RR)[blockIdx.x] = sums[K + c];
        }
    }
}

// p = z + beta p  (beta = rz_new / rz; the reference's kernelMyxpy with gamma = beta), four grid strides per trip as in the update
template <int K>
__global__ __launch_bounds__(kThreads) void cg_multi_direction_kernel(int n, const double* __restrict__ R, const double* __restrict__ dinv,
                                                                      double* __restrict__ P, const double* __restrict__ s,
                                                                      const int* __restrict__ active, int c0, int cur)
{
    bool on[K];
    double sums[2 * K], beta[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        sums[c] = partials_of(slot<A_COUNT>(s, c0 + c, A_RZ0 + 2 * (cur ^ 1)));
        sums[K + c] = partials_of(slot<A_COUNT>(s, c0 + c, A_RZ0 + 2 * cur));
    }
    block_sum_n(sums);
    const double* r[K];
    double* p[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        beta[c] = sums[c] / sums[K + c];
        r[c] = R + (size_t)(c0 + c) * n;
        p[c] = P + (size_t)(c0 + c) * n;
    }
    walk<K, kWalkU, 2>(
        n, on, InvDiag{dinv},
        [&](int c, int i, double(&in)[2], double) {
            in[0] = p[c][i];
            in[1] = r[c][i];
        },
        [&](int c, int i, const double(&in)[2], double di) { p[c][i] = fma(beta[c], in[0], dinv ? in[1] * di : in[1]); });
}

// the kernels of one iteration for columns c0 .. c0 + K - 1 (dot: p . q is not a by-product of the multiply)
template <int K>
void launch_vector_kernels(int grid, hipStream_t st, int n, double* P, const double* Q, const double* dinv, double* X, long long ldx,
                           double* R, double* s, const int* active, int c0, int cur, bool dot = true)
{
    if (dot) hipLaunchKernelGGL(cg_multi_dot_kernel<K>, dim3(grid), dim3(kThreads), 0, st, n, P, Q, s, active, c0);
    hipLaunchKernelGGL(cg_multi_update_kernel<K>, dim3(grid), dim3(kThreads), 0, st, n, P, Q, dinv, X, ldx, R, s, active, c0, cur);
    hipLaunchKernelGGL(cg_multi_direction_kernel<K>, dim3(grid), dim3(kThreads), 0, st, n, R, dinv, P, s, active, c0, cur);
}

// launch<K>(...) for a width known at run time
template <typename F>
void with_width(int K, F&& f)
{
    switch (K) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
    }
}

}  // namespace

// ------------------------------------------------------------------ the same kernels for ehyb_cheb.hip (cg_shared.h)
void ehyb::cg_launch_init(int grid, hipStream_t st, int n, const double* b, const double* q, const double* dinv, double* r, double* p,
                          double* s)
{
    hipLaunchKernelGGL(cg_init_kernel, dim3(grid), dim3(kThreads), 0, st, n, b, q, dinv, r, p, s);
}
void ehyb::cg_launch_dot(int K, int grid, hipStream_t st, int n, const double* P, const double* Q, double* s, const int* active, int c0)
{
    with_width(K, [&](auto W) {
        hipLaunchKernelGGL(cg_multi_dot_kernel<decltype(W)::value>, dim3(grid), dim3(kThreads), 0, st, n, P, Q, s, active, c0);
    });
}
void ehyb::cg_launch_update(int K, int grid, hipStream_t st, int n, const double* P, const double* Q, const double* dinv, double* X,
                            long long ldx, double* R, double* s, const int* active, int c0, int cur)
{
    with_width(K, [&](auto W) {
        hipLaunchKernelGGL(cg_multi_update_kernel<decltype(W)::value>, dim3(grid), dim3(kThreads), 0, st, n, P, Q, dinv, X, ldx, R, s, active,
                           c0, cur);
    });
}
void ehyb::cg_launch_direction(int K, int grid, hipStream_t st, int n, const double* Zv, const double* dinv, double* P, const double* s,
                               const int* active, int c0, int cur)
{
    with_width(K, [&](auto W) {
        hipLaunchKernelGGL(cg_multi_direction_kernel<decltype(W)::value>, dim3(grid), dim3(kThreads), 0, st, n, Zv, dinv, P, s, active, c0,
                           cur);
    });
}

extern "C" int ehyb_cg(ehyb_plan* P, const double* b, double* x, int max_iter, double rtol, int check_every,
                       void* stream, int* iters_done, double* rel_residual)
{
    return ehyb_pcg(P, nullptr, b, x, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

// A driver of its own, not ehyb_pcg_multi at k = 1: it fuses p . q into the multiply (spmv_xy) and issues its multiplies with the
// plan's own alternation, where a k = 1 ehyb_pcg_multi states explicit walks in its captured graph -- which ell_walk honours
// even on a plan that does not alternate.  Folding the two would change what a one-vector solve launches.
extern "C" int ehyb_pcg(ehyb_plan* P, const double* dinv, const double* b, double* x, int max_iter, double rtol,
                        int check_every, void* stream, int* iters_done, double* rel_residual)
{
    int rc = solve_prologue("ehyb_pcg", P, b && x, max_iter, rtol);
    if (rc != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    SolveLoop L(n, check_every);
    const int grid = L.grid;
    double *r, *p, *q, *s;
    HIP_TRY(L.begin(stream, {&r, &p, &q}, n, &s, A_COUNT));
    const hipStream_t st = L.st;

    if ((rc = ehyb_spmv(P, x, q, st)) != EHYB_OK) return rc;  // q = A x0
    hipLaunchKernelGGL(cg_init_kernel, dim3(grid), dim3(kThreads), 0, st, n, b, q, dinv, r, p, s);
    HIP_TRY(L.read());
    const double bb0 = L.sum(A_BB), bb = bb0 > 0 ? bb0 : 1.0;
    double rs = L.sum(A_RR);  // ||r||^2 (the preconditioned product r.z drives the recurrences, not the stop test)

    // p . q as a by-product of the multiply where one window launch writes all of q (the rows' p sits in its LDS window): the
    // launch leaves one partial per workgroup in the slot the dot kernel would fill -- at most `grid` of them, the rest of the
    // slot stays zero, and the update kernel adds the slot up in the same fixed order as ever.
    const int xy_parts = P->cfg.cg_fused_dot != 2 ? spmv_xy_partials(P) : 0;
    const bool fused = xy_parts > 0 && xy_parts <= grid;
    if (fused) HIP_TRY(hipMemsetAsync(s + (size_t)A_PQ * kMaxGrid, 0, kMaxGrid * sizeof(double), st));
    int it = 0;
    rc = L.run(
        P, max_iter, it, [&] { return std::sqrt(rs / bb) > rtol; },
        [&](int cur, bool) -> int {
            // q = A p: x of the multiply changes every time
            const int e = fused ? spmv_xy(P, p, q, st, s + (size_t)A_PQ * kMaxGrid) : ehyb_spmv(P, p, q, st);
            if (e == EHYB_OK) launch_vector_kernels<1>(grid, st, n, p, q, dinv, x, n, r, s, nullptr, 0, cur, !fused);
            return e;
        },
        [&](int cur) -> int {
            rs = L.sum(A_RR);
            const double rz = L.sum(A_RZ0 + 2 * cur);
            if (!(rs == rs) || !(rz == rz)) rs = NAN;  // NaN: breakdown (matrix or preconditioner not positive definite)
            return EHYB_OK;
        });
    if (rc != EHYB_OK) return rc;
    if (iters_done) *iters_done = it;
    if (rel_residual) *rel_residual = std::sqrt(rs / bb);
    if (!(rs == rs)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_pcg: breakdown (is the matrix symmetric positive definite?)");
    return EHYB_OK;
}

// ------------------------------------------------------------------ k right-hand sides, one multiply (ehyb_pcg_multi)
extern "C" int ehyb_cg_multi(ehyb_plan* P, const double* B, int64_t ldb, double* X, int64_t ldx, int k, int max_iter, double rtol,
                             int check_every, void* stream, int* iters_done, double* rel_residual)
{
    return ehyb_pcg_multi(P, nullptr, B, ldb, X, ldx, k, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

extern "C" int ehyb_pcg_multi(ehyb_plan* P, const double* dinv, const double* B, int64_t ldb, double* X, int64_t ldx, int k,
                              int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual)
{
    int rc = multi_prologue("ehyb_pcg_multi", P, B && X, ldb, ldx, k, max_iter, rtol);
    if (rc != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    SolveLoop L(n, check_every);
    const int grid = L.grid;
    double *R, *Pd, *Q, *s;
    HIP_TRY(L.begin(stream, {&R, &Pd, &Q}, (size_t)n * k, &s, (size_t)k * A_COUNT, (k + 1) / 2));  // the active flags behind the slots
    int* active = (int*)(s + (size_t)k * A_COUNT * kMaxGrid);
    const hipStream_t st = L.st;

    if ((rc = ehyb_spmm(P, X, ldx, Q, n, k, st, EHYB_WALK_AUTO)) != EHYB_OK) return rc;  // Q = A X0
    for (int j = 0; j < k; ++j)
        hipLaunchKernelGGL(cg_init_kernel, dim3(grid), dim3(kThreads), 0, st, n, B + (size_t)j * ldb, Q + (size_t)j * n, dinv,
                           R + (size_t)j * n, Pd + (size_t)j * n, s + (size_t)j * A_COUNT * kMaxGrid);
    HIP_TRY(L.read());
    std::vector<double> bb(k), rs(k);
    std::vector<int> live(k), iters(k, 0);
    int n_live = 0;
    for (int j = 0; j < k; ++j) {
        const double bb0 = L.sum(j * A_COUNT + A_BB);
        bb[j] = bb0 > 0 ? bb0 : 1.0;
        rs[j] = L.sum(j * A_COUNT + A_RR);
        live[j] = std::sqrt(rs[j] / bb[j]) > rtol;  // (NaN: frozen at once, reported as a breakdown)
        n_live += live[j];
    }
    HIP_TRY(hipMemcpyAsync(active, live.data(), (size_t)k * sizeof(int), hipMemcpyHostToDevice, st));

    int it = 0;
    rc = L.run(
        P, max_iter, it, [&] { return n_live > 0; },
        [&](int cur, bool captured) -> int {
            // Q = A P, frozen columns included (their q is not read).  A captured multiply keeps the direction it was captured
            // with, so the captured ones state their walks: first to last, then last to first.
            const int walk = !captured ? EHYB_WALK_AUTO : cur ? EHYB_WALK_LAST_TO_FIRST : EHYB_WALK_FIRST_TO_LAST;
            const int e = ehyb_spmm(P, Pd, n, Q, n, k, st, walk);
            if (e != EHYB_OK) return e;
            for_each_group(k, [&](auto K, int c0) {
                launch_vector_kernels<decltype(K)::value>(grid, st, n, Pd, Q, dinv, X, ldx, R, s, active, c0, cur);
            });
            return EHYB_OK;
        },
        [&](int cur) -> int {
            bool changed = false;
            for (int j = 0; j < k; ++j) {
                if (!live[j]) continue;
                rs[j] = L.sum(j * A_COUNT + A_RR);
                const double rz = L.sum(j * A_COUNT + A_RZ0 + 2 * cur);
                if (!(rs[j] == rs[j]) || !(rz == rz)) rs[j] = NAN;  // breakdown of this column: frozen, the others go on
                if (!(std::sqrt(rs[j] / bb[j]) > rtol)) {
                    live[j] = 0;
                    iters[j] = it;
                    --n_live;
                    changed = true;
                }
            }
            if (changed && n_live > 0) HIP_TRY(hipMemcpyAsync(active, live.data(), (size_t)k * sizeof(int), hipMemcpyHostToDevice, st));
            return EHYB_OK;
        });
    if (rc != EHYB_OK) return rc;
    bool broke = false;
    for (int j = 0; j < k; ++j) {
        if (live[j]) iters[j] = it;
        if (iters_done) iters_done[j] = iters[j];
        if (rel_residual) rel_residual[j] = std::sqrt(rs[j] / bb[j]);
        broke = broke || !(rs[j] == rs[j]);
    }
    if (broke) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_pcg_multi: breakdown in a column (is the matrix symmetric positive definite?)");
    return EHYB_OK;
}

// ------------------------------------------------------------------ building blocks for a multi-GPU caller
// The same four vector kernels (those of an iteration with K = 1) for a caller that owns the loop
// (ehyb_spmv_gpu_amd/dist.py HaloCG: one process per GPU, the multiply through the halo exchange): every
// rank runs them on its rows with the SAME grid, and an all_reduce (sum) of a slot of the partial array
// turns every rank's partials into the element-wise global ones -- the kernel that needs the scalar adds
// them up as before.
//   s: `slots` slots of `slot_doubles` doubles (ehyb_cg_layout); r.z number c (0/1) lives in slot rz0 + 2 c, r.r
//   between the two; every launch uses slot_doubles / 2 workgroups.
extern "C" int ehyb_cg_layout(int* slots, int* slot_doubles, int* slot_bb, int* slot_pq, int* slot_rr, int* slot_rz0)
{
    if (slots) *slots = A_COUNT;
    if (slot_doubles) *slot_doubles = kMaxGrid;
    if (slot_bb) *slot_bb = A_BB;
    if (slot_pq) *slot_pq = A_PQ;
    if (slot_rr) *slot_rr = A_RR;
    if (slot_rz0) *slot_rz0 = A_RZ0;
    return EHYB_OK;
}

// r = b - q, p = z = M^-1 r; partials of r.z (slot rz0), r.r, b.b
extern "C" int ehyb_cg_init_step(int n, const double* b, const double* q, const double* dinv, double* r, double* p, double* s,
                                 void* stream)
{
    int rc = check_step("ehyb_cg_init_step", n, {b, q, r, p, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(cg_init_kernel, dim3(kMaxGrid / 2), dim3(kThreads), 0, (hipStream_t)stream, n, b, q, dinv, r, p, s);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
// partials of p.q (slot pq)
extern "C" int ehyb_cg_dot_step(int n, const double* p, const double* q, double* s, void* stream)
{
    int rc = check_step("ehyb_cg_dot_step", n, {p, q, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(cg_multi_dot_kernel<1>, dim3(kMaxGrid / 2), dim3(kThreads), 0, (hipStream_t)stream, n, p, q, s, nullptr, 0);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
// alpha = rz[cur] / pq; x += alpha p; r -= alpha q; partials of the new r.z (slot rz0 + (cur ^ 1)) and r.r
extern "C" int ehyb_cg_update_step(int n, const double* p, const double* q, const double* dinv, double* x, double* r, double* s,
                                   int cur, void* stream)
{
    int rc = check_step("ehyb_cg_update_step", n, {p, q, x, r, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(cg_multi_update_kernel<1>, dim3(kMaxGrid / 2), dim3(kThreads), 0, (hipStream_t)stream, n, p, q, dinv, x, n, r, s,
                       nullptr, 0, cur & 1);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
// beta = rz[cur ^ 1] / rz[cur]; p = z + beta p
extern "C" int ehyb_cg_direction_step(int n, const double* r, const double* dinv, double* p, const double* s, int cur, void* stream)
{
    int rc = check_step("ehyb_cg_direction_step", n, {r, p, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(cg_multi_direction_kernel<1>, dim3(kMaxGrid / 2), dim3(kThreads), 0, (hipStream_t)stream, n, r, dinv, p, s, nullptr,
                       0, cur & 1);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
