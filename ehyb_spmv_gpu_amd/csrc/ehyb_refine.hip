// Iterative refinement on top of the device-resident CG (ehyb_cg.hip): fp64 answers from a plan whose values the device holds in
// fp32 (cfg.val_f32).  The outer loop runs in fp64 on the fp64 plan -- r = b - A x, then x += d -- and the correction d comes
// from ehyb_pcg on the inner plan, which streams half the value bytes per multiply.  Two vector kernels of its own:
//   refine_residual_kernel  r = b - q, partials of r.r and b.b, one per workgroup (put_partial: the fixed order of vec_reduce.h)
//   refine_axpy_kernel      x += d
// Both walk the vectors as the CG kernels do (vec_walk.h, four grid strides per trip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "ehyb_internal.h"
#include "solve_loop.h"
#include "vec_walk.h"

using namespace ehyb;

namespace {

enum { R_RR = 0, R_BB = 1, R_COUNT = 2 };

__global__ __launch_bounds__(kThreads) void refine_residual_kernel(int n, const double* __restrict__ b, const double* __restrict__ q,
                                                                   double* __restrict__ r, double* __restrict__ s)
{
    double rr = 0.0, bb = 0.0;
    const bool live[1] = {true};  // one vector, always live
    walk<1, kWalkU, 2>(
        n, live, NoShared{},
        [&](int, int i, double(&in)[2], int) {
            in[0] = b[i];
            in[1] = q[i];
        },
        [&](int, int i, const double(&in)[2], int) {
            const double ri = in[0] - in[1];
            r[i] = ri;
            rr = fma(ri, ri, rr);
            bb = fma(in[0], in[0], bb);
        });
    put_partial(rr, s + R_RR * kMaxGrid);
    put_partial(bb, s + R_BB * kMaxGrid);
}

__global__ __launch_bounds__(kThreads) void refine_axpy_kernel(int n, const double* __restrict__ d, double* __restrict__ x)
{
    const bool live[1] = {true};
    walk<1, kWalkU, 2>(
        n, live, NoShared{},
        [&](int, int i, double(&in)[2], int) {
            in[0] = d[i];
            in[1] = x[i];
        },
        [&](int, int i, const double(&in)[2], int) { x[i] = in[1] + in[0]; });
}

}  // namespace

extern "C" int ehyb_pcg_refine(ehyb_plan* P, ehyb_plan* inner, const double* dinv, const double* b, double* x, int max_outer,
                               int inner_max_iter, double rtol, double inner_rtol, void* stream, int* outer_done, int* inner_iters_total,
                               double* rel_residual)
{
    int rc = solve_prologue("ehyb_pcg_refine", P, b && x, max_outer, rtol);
    if (rc == EHYB_OK) rc = solve_prologue("ehyb_pcg_refine (inner plan)", inner, true, inner_max_iter, inner_rtol);
    if (rc != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    if (inner->host.n_cols != n) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_pcg_refine: the inner plan has %d rows, the plan %d", inner->host.n_cols, n);
    SolveLoop L(n, 0);
    double *r, *d, *q, *s;
    HIP_TRY(L.begin(stream, {&r, &d, &q}, n, &s, R_COUNT));
    const hipStream_t st = L.st;
    int outer = 0, inner_total = 0;
    double rel = 0.0, prev = INFINITY;
    for (;;) {
        if ((rc = ehyb_spmv_walk(P, x, q, st, EHYB_WALK_FIRST_TO_LAST)) != EHYB_OK) return rc;
        hipLaunchKernelGGL(refine_residual_kernel, dim3(L.grid), dim3(kThreads), 0, st, n, b, q, r, s);
        HIP_TRY(L.read());
        const double bb0 = L.sum(R_BB), bb = bb0 > 0 ? bb0 : 1.0;
        rel = std::sqrt(L.sum(R_RR) / bb);
        // converged; stagnation (||r|| did not at least halve: what the inner plan can give is used up) or NaN; out of steps
        if (!(rel > rtol) || !(rel <= 0.5 * prev) || outer >= max_outer) break;
        prev = rel;
        HIP_TRY(hipMemsetAsync(d, 0, (size_t)n * sizeof(double), st));
        int it = 0;
        if ((rc = ehyb_pcg(inner, dinv, r, d, inner_max_iter, inner_rtol, 0, st, &it, nullptr)) != EHYB_OK) return rc;
        inner_total += it;
        hipLaunchKernelGGL(refine_axpy_kernel, dim3(L.grid), dim3(kThreads), 0, st, n, d, x);
        ++outer;
    }
    HIP_TRY(hipGetLastError());
    if (outer_done) *outer_done = outer;
    if (inner_iters_total) *inner_iters_total = inner_total;
    if (rel_residual) *rel_residual = rel;
    return EHYB_OK;
}

// ------------------------------------------------------------------ the two kernels one at a time (as ehyb_cg_*_step)
extern "C" int ehyb_refine_residual_step(int n, const double* b, const double* q, double* r, double* s, void* stream)
{
    int rc = check_step("ehyb_refine_residual_step", n, {b, q, r, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(refine_residual_kernel, dim3(kMaxGrid / 2), dim3(kThreads), 0, (hipStream_t)stream, n, b, q, r, s);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_refine_axpy_step(int n, const double* d, double* x, void* stream)
{
    int rc = check_step("ehyb_refine_axpy_step", n, {d, x});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(refine_axpy_kernel, dim3(kMaxGrid / 2), dim3(kThreads), 0, (hipStream_t)stream, n, d, x);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
