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
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "ehyb_internal.h"
#include "solve_loop.h"

using namespace ehyb;

namespace {

// partial slots, kMaxGrid doubles each; rho number c = r^.r of iterations of parity c lives in slot B_RHO0 + 2 c.  Behind
// them two ints: the status word and the device's iteration counter.
enum { B_BB = 0, B_RV = 1, B_SS = 2, B_TS = 3, B_TT = 4, B_RHO0 = 5, B_RR = 6, B_RHO1 = 7, B_COUNT = 8 };
enum { F_STATUS = 0, F_ITERS = 1, F_COUNT = 2 };
enum { ST_RUNNING = 0, ST_CONVERGED = 1, ST_BREAKDOWN = 2 };

__device__ __forceinline__ double* slot(double* s, int which) { return s + (size_t)which * kMaxGrid; }
__device__ __forceinline__ const double* slot(const double* s, int which) { return s + (size_t)which * kMaxGrid; }
__device__ __forceinline__ bool usable_divisor(double d) { return d != 0.0 && isfinite(d); }

// the status as the workgroup saw it on entry, the same in every thread (a sibling workgroup of the launch may write it)
__device__ __forceinline__ bool stopped(const int* __restrict__ flags)
{
    __shared__ int st;
    if (threadIdx.x == 0) st = __atomic_load_n(&flags[F_STATUS], __ATOMIC_RELAXED);
    __syncthreads();
    return st != ST_RUNNING;
}

__device__ __forceinline__ void set_status(int* __restrict__ flags, int status)
{
    if (threadIdx.x == 0) __atomic_store_n(&flags[F_STATUS], status, __ATOMIC_RELAXED);
}

// r = b - q (q = A x0), r^ = r, p^ = M^-1 r; partials of rho = r^.r, r.r, b.b
__global__ __launch_bounds__(kThreads) void bicg_init_kernel(int n, const double* __restrict__ b, const double* __restrict__ q,
                                                             const double* __restrict__ dinv, double* __restrict__ r,
                                                             double* __restrict__ rh, double* __restrict__ p, double* __restrict__ s)
{
    double rr = 0.0, bb = 0.0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const double bi = b[i], ri = bi - q[i];
        r[i] = ri;
        rh[i] = ri;
        p[i] = dinv ? ri * dinv[i] : ri;
        rr = fma(ri, ri, rr);
        bb = fma(bi, bi, bb);
    }
    put_partial(rr, slot(s, B_RHO0));
    put_partial(rr, slot(s, B_RR));
    put_partial(bb, slot(s, B_BB));
}

// step 2: partials of r^.v
__global__ __launch_bounds__(kThreads) void bicg_dot_kernel(int n, const double* __restrict__ rh, const double* __restrict__ v,
                                                            double* __restrict__ s, const int* __restrict__ flags)
{
    if (stopped(flags)) return;
    double acc = 0.0;
    const int stride = (int)gridDim.x * kThreads;
    int i = blockIdx.x * kThreads + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {  // four grid strides per trip, as ehyb_cg.hip's update kernel
        double av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            av[u] = rh[i + u * stride];
            bv[u] = v[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fma(av[u], bv[u], acc);
    }
    for (; i < n; i += stride) acc = fma(rh[i], v[i], acc);
    put_partial(acc, slot(s, B_RV));
}

// step 3: alpha = rho / r^.v;  s = r - alpha v;  s^ = M^-1 s;  partials of s.s
__global__ __launch_bounds__(kThreads) void bicg_s_kernel(int n, const double* __restrict__ r, const double* __restrict__ v,
                                                          const double* __restrict__ dinv, double* __restrict__ sv,
                                                          double* __restrict__ sh, double* __restrict__ s, int* __restrict__ flags,
                                                          int cur)
{
    if (stopped(flags)) return;
    double sums[2] = {partials_of(slot(s, B_RHO0 + 2 * cur)), partials_of(slot(s, B_RV))};
    block_sum_n(sums);
    const double rho = sums[0], rv = sums[1], alpha = rho / rv;
    if (!isfinite(rho) || !usable_divisor(rv) || !isfinite(alpha)) {
        set_status(flags, ST_BREAKDOWN);
        return;
    }
    double ss = 0.0;
    const int stride = (int)gridDim.x * kThreads;
    int i = blockIdx.x * kThreads + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        double rv4[4], vv[4], dv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            rv4[u] = r[i + u * stride];
            vv[u] = v[i + u * stride];
            dv[u] = dinv ? dinv[i + u * stride] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double si = fma(-alpha, vv[u], rv4[u]);
            sv[i + u * stride] = si;
            sh[i + u * stride] = dinv ? si * dv[u] : si;
            ss = fma(si, si, ss);
        }
    }
    for (; i < n; i += stride) {
        const double si = fma(-alpha, v[i], r[i]);
        sv[i] = si;
        sh[i] = dinv ? si * dinv[i] : si;
        ss = fma(si, si, ss);
    }
    put_partial(ss, slot(s, B_SS));
}

// step 5: partials of t.s and t.t in one pass
__global__ __launch_bounds__(kThreads) void bicg_dot2_kernel(int n, const double* __restrict__ t, const double* __restrict__ sv,
                                                             double* __restrict__ s, const int* __restrict__ flags)
{
    if (stopped(flags)) return;
    double acc[2] = {0.0, 0.0};
    const int stride = (int)gridDim.x * kThreads;
    int i = blockIdx.x * kThreads + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        double tv[4], sv4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            tv[u] = t[i + u * stride];
            sv4[u] = sv[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[0] = fma(tv[u], sv4[u], acc[0]);
            acc[1] = fma(tv[u], tv[u], acc[1]);
        }
    }
    for (; i < n; i += stride) {
        acc[0] = fma(t[i], sv[i], acc[0]);
        acc[1] = fma(t[i], t[i], acc[1]);
    }
    block_sum_n(acc);
    if (threadIdx.x == 0) {
        slot(s, B_TS)[blockIdx.x] = acc[0];
        slot(s, B_TT)[blockIdx.x] = acc[1];
    }
}

// step 6: omega = t.s / t.t;  x += alpha p^ + omega s^;  r = s - omega t;  partials of rho_new = r^.r (the other rho slot)
// and r.r; the counter advances.  Half step (s.s <= thr b.b): x += alpha p^, r = s, partials of r.r only.
__global__ __launch_bounds__(kThreads) void bicg_update_kernel(int n, const double* __restrict__ p, const double* __restrict__ sh,
                                                               const double* __restrict__ sv, const double* __restrict__ t,
                                                               const double* __restrict__ rh, double* __restrict__ x,
                                                               double* __restrict__ r, double* __restrict__ s,
                                                               int* __restrict__ flags, int cur, double thr)
{
    if (stopped(flags)) return;
    double sums[6] = {partials_of(slot(s, B_RHO0 + 2 * cur)), partials_of(slot(s, B_RV)), partials_of(slot(s, B_SS)),
                      partials_of(slot(s, B_BB)), partials_of(slot(s, B_TS)), partials_of(slot(s, B_TT))};
    block_sum_n(sums);
    const double alpha = sums[0] / sums[1], bb = sums[3] > 0 ? sums[3] : 1.0;
    const int stride = (int)gridDim.x * kThreads;
    int i = blockIdx.x * kThreads + threadIdx.x;
    if (sums[2] <= thr * bb) {  // half step: s is small enough
        double rr = 0.0;
        for (; i < n; i += stride) {
            const double si = __builtin_nontemporal_load(&sv[i]);
            x[i] = fma(alpha, p[i], x[i]);
            r[i] = si;
            rr = fma(si, si, rr);
        }
        put_partial(rr, slot(s, B_RR));
        if (blockIdx.x == 0 && threadIdx.x == 0) flags[F_ITERS] += 1;
        return;
    }
    const double tt = sums[5], omega = sums[4] / tt;
    if (!usable_divisor(tt) || !isfinite(omega)) {
        set_status(flags, ST_BREAKDOWN);
        return;
    }
    double rho = 0.0, rr = 0.0;
    for (; i + 3 * stride < n; i += 4 * stride) {
        double pv[4], shv[4], sv4[4], tv[4], rhv[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            pv[u] = p[i + u * stride];
            shv[u] = __builtin_nontemporal_load(&sh[i + u * stride]);  // s^, s and t are dead after this kernel, x is not read
            sv4[u] = __builtin_nontemporal_load(&sv[i + u * stride]);  // again before the next update: streamed past the
            tv[u] = __builtin_nontemporal_load(&t[i + u * stride]);    // caches, which hold the matrix's tail
            xv[u] = __builtin_nontemporal_load(&x[i + u * stride]);
            rhv[u] = rh[i + u * stride];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            __builtin_nontemporal_store(fma(omega, shv[u], fma(alpha, pv[u], xv[u])), &x[i + u * stride]);
            const double ri = fma(-omega, tv[u], sv4[u]);
            r[i + u * stride] = ri;
            rho = fma(rhv[u], ri, rho);
            rr = fma(ri, ri, rr);
        }
    }
    for (; i < n; i += stride) {
        x[i] = fma(omega, sh[i], fma(alpha, p[i], x[i]));
        const double ri = fma(-omega, t[i], sv[i]);
        r[i] = ri;
        rho = fma(rh[i], ri, rho);
        rr = fma(ri, ri, rr);
    }
    double out[2] = {rho, rr};
    block_sum_n(out);
    if (threadIdx.x == 0) {
        slot(s, B_RHO0 + 2 * (cur ^ 1))[blockIdx.x] = out[0];
        slot(s, B_RR)[blockIdx.x] = out[1];
        if (blockIdx.x == 0) flags[F_ITERS] += 1;
    }
}

// step 7: the stop test (converged: the half step was taken, or r.r <= thr b.b), then beta = (rho_new / rho) (alpha / omega)
// and p^ = M^-1 r + beta (p^ - omega M^-1 v)
__global__ __launch_bounds__(kThreads) void bicg_direction_kernel(int n, const double* __restrict__ r, const double* __restrict__ v,
                                                                  const double* __restrict__ dinv, double* __restrict__ p,
                                                                  const double* __restrict__ s, int* __restrict__ flags, int cur,
                                                                  double thr)
{
    if (stopped(flags)) return;
    double sums[8] = {partials_of(slot(s, B_SS)), partials_of(slot(s, B_RR)), partials_of(slot(s, B_BB)),
                      partials_of(slot(s, B_RHO0 + 2 * cur)), partials_of(slot(s, B_RHO0 + 2 * (cur ^ 1))),
                      partials_of(slot(s, B_RV)), partials_of(slot(s, B_TS)), partials_of(slot(s, B_TT))};
    block_sum_n(sums);
    const double bb = sums[2] > 0 ? sums[2] : 1.0;
    if (sums[0] <= thr * bb || sums[1] <= thr * bb) {
        set_status(flags, ST_CONVERGED);
        return;
    }
    const double rho = sums[3], rho_new = sums[4], alpha = rho / sums[5], omega = sums[6] / sums[7];
    const double beta = (rho_new / rho) * (alpha / omega);
    if (!usable_divisor(rho) || !usable_divisor(omega) || !isfinite(rho_new) || !isfinite(beta)) {
        set_status(flags, ST_BREAKDOWN);
        return;
    }
    const int stride = (int)gridDim.x * kThreads;
    int i = blockIdx.x * kThreads + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        double pv[4], rv4[4], vv[4], dv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            pv[u] = p[i + u * stride];
            rv4[u] = r[i + u * stride];
            vv[u] = __builtin_nontemporal_load(&v[i + u * stride]);  // v is dead after this kernel
            dv[u] = dinv ? dinv[i + u * stride] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double zi = dinv ? rv4[u] * dv[u] : rv4[u], wi = dinv ? vv[u] * dv[u] : vv[u];
            p[i + u * stride] = fma(beta, fma(-omega, wi, pv[u]), zi);
        }
    }
    for (; i < n; i += stride) {
        const double zi = dinv ? r[i] * dinv[i] : r[i], wi = dinv ? v[i] * dinv[i] : v[i];
        p[i] = fma(beta, fma(-omega, wi, p[i]), zi);
    }
}

}  // namespace

extern "C" int ehyb_bicgstab(ehyb_plan* P, const double* dinv, const double* b, double* x, int max_iter, double rtol,
                             int check_every, void* stream, int* iters_done, double* rel_residual)
{
    int rc = solve_prologue("ehyb_bicgstab", P, b && x, max_iter, rtol);
    if (rc != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    SolveLoop L(n, check_every);
    const int grid = L.grid;
    double *r, *rh, *p, *v, *sv, *sh, *t, *s;
    HIP_TRY(L.begin(stream, {&r, &rh, &p, &v, &sv, &sh, &t}, n, &s, B_COUNT, 1));  // the flags in the double behind the slots
    int* flags = (int*)(s + (size_t)B_COUNT * kMaxGrid);
    const hipStream_t st = L.st;
    const double thr = rtol * rtol;

    HIP_TRY(hipMemsetAsync(flags, 0, F_COUNT * sizeof(int), st));
    // v = A x0, walked last to first so that the first iteration's first-to-last walk starts on what it left in the cache
    if ((rc = ehyb_spmv_walk(P, x, v, st, EHYB_WALK_LAST_TO_FIRST)) != EHYB_OK) return rc;
    hipLaunchKernelGGL(bicg_init_kernel, dim3(grid), dim3(kThreads), 0, st, n, b, v, dinv, r, rh, p, s);
    HIP_TRY(L.read());
    const double bb0 = L.sum(B_BB), bb = bb0 > 0 ? bb0 : 1.0;
    double rr = L.sum(B_RR);
    int status = !std::isfinite(bb0) || !std::isfinite(rr) ? ST_BREAKDOWN : rr <= thr * bb ? ST_CONVERGED : ST_RUNNING;
    int done = 0, it = 0;

    // An even and an odd iteration -- four multiplies walking first to last, last to first, first to last, last to first --
    // are one graph; the plain launches use the same walks.
    rc = L.run(
        P, max_iter, it, [&] { return status == ST_RUNNING; },
        [&](int cur, bool) -> int {
            int e = ehyb_spmv_walk(P, p, v, st, EHYB_WALK_FIRST_TO_LAST);  // v = A p^
            if (e != EHYB_OK) return e;
            hipLaunchKernelGGL(bicg_dot_kernel, dim3(grid), dim3(kThreads), 0, st, n, rh, v, s, flags);
            hipLaunchKernelGGL(bicg_s_kernel, dim3(grid), dim3(kThreads), 0, st, n, r, v, dinv, sv, sh, s, flags, cur);
            if ((e = ehyb_spmv_walk(P, sh, t, st, EHYB_WALK_LAST_TO_FIRST)) != EHYB_OK) return e;  // t = A s^
            hipLaunchKernelGGL(bicg_dot2_kernel, dim3(grid), dim3(kThreads), 0, st, n, t, sv, s, flags);
            hipLaunchKernelGGL(bicg_update_kernel, dim3(grid), dim3(kThreads), 0, st, n, p, sh, sv, t, rh, x, r, s, flags, cur, thr);
            hipLaunchKernelGGL(bicg_direction_kernel, dim3(grid), dim3(kThreads), 0, st, n, r, v, dinv, p, s, flags, cur, thr);
            return EHYB_OK;
        },
        [&](int) -> int {
            int f[F_COUNT];
            std::memcpy(f, &L.h[(size_t)B_COUNT * kMaxGrid], sizeof f);
            status = f[F_STATUS];
            done = f[F_ITERS];
            rr = L.sum(B_RR);
            return EHYB_OK;
        });
    if (rc != EHYB_OK) return rc;
    if (iters_done) *iters_done = done;
    if (rel_residual) *rel_residual = std::sqrt(rr / bb);
    if (status == ST_BREAKDOWN)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_bicgstab: breakdown after %d iterations (a zero or non-finite rho, r^.v, t.t or omega)", done);
    return EHYB_OK;
}

// ------------------------------------------------------------------ building blocks for a caller that owns the loop
// The six vector kernels above, one launch each, for a caller that issues the multiplies itself (and for tests that look at
// one kernel at a time) -- the analogue of ehyb_cg_*_step.  s: `slots` slots of `slot_doubles` doubles and one more double
// behind them, whose two ints are the status word and the iteration counter (ehyb_bicgstab_layout); every launch uses
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

inline int check_step(const char* who, int n, std::initializer_list<const void*> pointers)
{
    bool ok = n >= 0;
    for (const void* a : pointers) ok = ok && a;
    if (!ok) EHYB_FAIL(EHYB_ERR_ARG, "%s: bad arguments", who);
    return EHYB_OK;
}

inline int* flags_of(double* s) { return (int*)(s + (size_t)B_COUNT * kMaxGrid); }

}  // namespace

extern "C" int ehyb_bicgstab_init_step(int n, const double* b, const double* q, const double* dinv, double* r, double* rh, double* p,
                                       double* s, void* stream)
{
    int rc = check_step("ehyb_bicgstab_init_step", n, {b, q, r, rh, p, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(bicg_init_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, b, q, dinv, r, rh, p, s);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_bicgstab_dot_step(int n, const double* rh, const double* v, double* s, void* stream)
{
    int rc = check_step("ehyb_bicgstab_dot_step", n, {rh, v, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(bicg_dot_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, rh, v, s, flags_of(s));
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_bicgstab_s_step(int n, const double* r, const double* v, const double* dinv, double* sv, double* sh, double* s,
                                    int cur, void* stream)
{
    int rc = check_step("ehyb_bicgstab_s_step", n, {r, v, sv, sh, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(bicg_s_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, r, v, dinv, sv, sh, s, flags_of(s),
                       cur & 1);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_bicgstab_dot2_step(int n, const double* t, const double* sv, double* s, void* stream)
{
    int rc = check_step("ehyb_bicgstab_dot2_step", n, {t, sv, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(bicg_dot2_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, t, sv, s, flags_of(s));
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_bicgstab_update_step(int n, const double* p, const double* sh, const double* sv, const double* t,
                                         const double* rh, double* x, double* r, double* s, int cur, double thr, void* stream)
{
    int rc = check_step("ehyb_bicgstab_update_step", n, {p, sh, sv, t, rh, x, r, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(bicg_update_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, p, sh, sv, t, rh, x, r, s,
                       flags_of(s), cur & 1, thr);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_bicgstab_direction_step(int n, const double* r, const double* v, const double* dinv, double* p, double* s, int cur,
                                            double thr, void* stream)
{
    int rc = check_step("ehyb_bicgstab_direction_step", n, {r, v, p, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(bicg_direction_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, r, v, dinv, p, s, flags_of(s),
                       cur & 1, thr);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
