// CG with a Chebyshev polynomial preconditioner (ehyb_pcg_cheb, ehyb_pcg_cheb_multi) on top of the device-resident CG of
// ehyb_cg.hip, and the power-method estimate of its upper bound (ehyb_lambda_max).  The preconditioner is all multiplies: with
// [lmin, lmax] around the spectrum of D^-1 A (D^-1 = inv_diag, or the identity), theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2,
// sigma = theta / delta, z = M^-1 r of degree m is
//   c0 = 1 / theta;  rho_0 = 1 / sigma
//   d = c0 D^-1 r;  z = d;  w = r                                                       (cheb_multi_start_kernel)
//   j = 1 .. m:  t = A~ d                                                               (ehyb_spmm on the polynomial's plan)
//                w = w - t;  rho_j = 1 / (2 sigma - rho_{j-1});  a_j = rho_j rho_{j-1};  b_j = 2 rho_j / delta
//                d = a_j d + b_j D^-1 w;  z = z + d                                     (cheb_multi_step_kernel)
// -- no dot product inside, no triangular solve, and A~ may be the fp32-value plan of the same matrix (cfg.val_f32): a
// preconditioner need not be exact, the CG around it stays in fp64 on the fp64 plan.
//
// Per iteration of parity cur: Q = A P on the plan, the dot, update (no preconditioner: x += alpha p, r -= alpha q, r.r) and
// direction kernels of ehyb_cg.hip (cg_shared.h), and between update and direction the polynomial: whichever of its kernels
// finishes z also reads r and leaves the partials of r.z in the slot the update kernel would have filled (it did fill it, with
// r.r: overwritten).  w_in of the first step is r itself and every later w lives in the solver's own vector, so r is never
// written by the polynomial; t shares the vector of q, which is dead after the update.  The two new kernels are templated on K
// columns per launch like the CG kernels, take the coefficients by value (they are the same for every column) and sum in the fixed
// order of vec_reduce.h.  One driver serves one and k right-hand sides, so column j of a k-column solve is the one-vector solve
// of b_j wherever the multiply is (plain storage).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "cg_shared.h"
#include "ehyb_internal.h"
#include "pcg_loop.h"
#include "solve_loop.h"
#include "vec_walk.h"

using namespace ehyb;

namespace {

// d = z = coef * D^-1 r; rz >= 0: partials of r.z into r.z slot number rz.  Columns c0 .. c0 + K - 1, leading dimension n.
template <int K>
__global__ __launch_bounds__(kThreads) void cheb_multi_start_kernel(int n, const double* __restrict__ R, const double* __restrict__ dinv,
                                                                    double coef, double* __restrict__ D, double* __restrict__ Z,
                                                                    double* __restrict__ s, const int* __restrict__ active, int c0, int rz)
{
    bool on[K];
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        acc[c] = 0.0;
    }
    walk<K, kWalkU, 1>(
        n, on, InvDiag{dinv}, [&](int c, int i, double(&in)[1], double) { in[0] = R[(size_t)(c0 + c) * n + i]; },
        [&](int c, int i, const double(&in)[1], double dvi) {
            const size_t o = (size_t)(c0 + c) * n + i;
            const double di = coef * (dinv ? in[0] * dvi : in[0]);
            D[o] = di;
            Z[o] = di;
            acc[c] = fma(in[0], di, acc[c]);
        });
    if (rz < 0) return;  // (a kernel argument: the whole launch returns)
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<A_COUNT>(s, c0 + c, A_RZ0 + 2 * rz)[blockIdx.x] = acc[c];
    }
}

// w_out = w_in - t;  d = a d + b D^-1 w_out;  z += d;  rz >= 0: partials of r.z into r.z slot number rz.  w_out may be w_in
// (neither is __restrict__: every index is read before it is written, by the one thread that owns it); t and w_in are dead
// after the step and loaded past the caches, as the update kernel loads q.
template <int K>
__global__ __launch_bounds__(kThreads) void cheb_multi_step_kernel(int n, const double* Win, const double* __restrict__ T,
                                                                   const double* __restrict__ dinv, double a, double b, double* Wout,
                                                                   double* __restrict__ D, double* __restrict__ Z, const double* R,
                                                                   double* __restrict__ s, const int* __restrict__ active, int c0, int rz)
{
    bool on[K];
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        acc[c] = 0.0;
    }
    enum { WV, TV, PV, ZV, RV, NV };
    walk<K, kWalkU, NV>(
        n, on, InvDiag{dinv},
        [&](int c, int i, double(&in)[NV], double) {
            const size_t o = (size_t)(c0 + c) * n + i;
            in[WV] = __builtin_nontemporal_load(&Win[o]);
            in[TV] = __builtin_nontemporal_load(&T[o]);
            in[PV] = D[o];
            in[ZV] = Z[o];
            in[RV] = rz >= 0 ? R[o] : 0.0;
        },
        [&](int c, int i, const double(&in)[NV], double dvi) {
            const size_t o = (size_t)(c0 + c) * n + i;
            const double wi = in[WV] - in[TV];
            const double di = fma(a, in[PV], b * (dinv ? wi * dvi : wi));
            const double zi = in[ZV] + di;
            Wout[o] = wi;
            D[o] = di;
            Z[o] = zi;
            acc[c] = fma(in[RV], zi, acc[c]);
        });
    if (rz < 0) return;
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<A_COUNT>(s, c0 + c, A_RZ0 + 2 * rz)[blockIdx.x] = acc[c];
    }
}

// ------------------------------------------------------------------ the power method on D^-1 A
// u holds the iterate unnormalised, the partials of u.u alternate between two slots; a step scales by 1 / ||u|| on the fly:
// v = u / ||u||, q <- q / ||u|| = A v, partials of v.q and v.Dv (the Rayleigh quotient of v), u = D^-1 q and the partials of u.u.
enum { M_VQ = 0, M_VDV = 1, M_NN0 = 2, M_NN1 = 3, M_COUNT = 4 };

__global__ __launch_bounds__(kThreads) void lambda_start_kernel(int n, double* __restrict__ u, double* __restrict__ s)
{
    double nn = 0.0;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const double ui = 1.0 + (double)(i % 7) * 0.125;
        u[i] = ui;
        nn = fma(ui, ui, nn);
    }
    put_partial(nn, s + M_NN0 * kMaxGrid);
}

__global__ __launch_bounds__(kThreads) void lambda_step_kernel(int n, double* __restrict__ u, const double* __restrict__ q,
                                                               const double* __restrict__ dinv, double* __restrict__ s, int cur)
{
    const double scale = 1.0 / sqrt(block_sum(partials_of(s + (M_NN0 + cur) * kMaxGrid)));
    double sums[3] = {0.0, 0.0, 0.0};
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const double di = dinv ? dinv[i] : 1.0;
        const double vi = u[i] * scale, qi = q[i] * scale;
        sums[0] = fma(vi, qi, sums[0]);
        sums[1] = fma(vi, dinv ? vi / di : vi, sums[1]);
        const double wi = dinv ? qi * di : qi;
        u[i] = wi;
        sums[2] = fma(wi, wi, sums[2]);
    }
    block_sum_n(sums);
    if (threadIdx.x == 0) {
        s[M_VQ * kMaxGrid + blockIdx.x] = sums[0];
        s[M_VDV * kMaxGrid + blockIdx.x] = sums[1];
        s[(M_NN0 + (cur ^ 1)) * kMaxGrid + blockIdx.x] = sums[2];
    }
}

// in this order, all EHYB_ERR_ARG: the degree, the bounds, the polynomial's plan
int cheb_args(const char* who, const ehyb_plan* P, const ehyb_plan* poly, int degree, double lmin, double lmax)
{
    if (degree < 0 || degree > EHYB_CHEB_MAX_DEGREE) EHYB_FAIL(EHYB_ERR_ARG, "%s: degree %d (0 .. %d)", who, degree, EHYB_CHEB_MAX_DEGREE);
    if (lmin > 0 && lmax > 0 && lmin >= lmax) EHYB_FAIL(EHYB_ERR_ARG, "%s: lmin %g >= lmax %g", who, lmin, lmax);
    if (lmin != lmin || lmax != lmax) EHYB_FAIL(EHYB_ERR_ARG, "%s: a bound is NaN", who);
    if (poly->host.n_cols != P->host.n_cols)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the polynomial's plan has %d rows, the plan %d", who, poly->host.n_cols, P->host.n_cols);
    if (poly->host.row_begin != 0 || poly->host.row_end != poly->host.n_cols)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the polynomial's plan does not cover all rows", who);
    return EHYB_OK;
}

// The one driver: the loop of pcg_loop.h with the polynomial as its preconditioner, whose multiplies are ehyb_spmm with explicit
// walks too.  The arguments are checked (ehyb_pcg_cheb, ehyb_pcg_cheb_multi).
int cheb_solve(const char* who, ehyb_plan* P, ehyb_plan* poly, const double* dinv, const double* B, int64_t ldb, double* X, int64_t ldx,
               int k, int degree, double lmin, double lmax, int max_iter, double rtol, int check_every, void* stream, int* iters_done,
               double* rel_residual)
{
    const int n = P->host.n_cols;
    double *D, *W;
    double coef0, ca[EHYB_CHEB_MAX_DEGREE], cb[EHYB_CHEB_MAX_DEGREE];
    auto prepare = [&](const PcgState& S) -> int {
        int rc;
        if (!(lmax > 0)) {
            double lam = 0.0;
            if ((rc = ehyb_lambda_max(poly, dinv, 20, S.st, &lam)) != EHYB_OK) return rc;
            lmax = 1.1 * lam;
        }
        if (!(lmin > 0)) lmin = lmax / 30.0;
        return ehyb_cheb_coeffs(lmin, lmax, degree, &coef0, ca, cb);  // (lmin >= an estimated lmax ends here)
    };
    // The multiplies of an iteration state their walks, alternating along the sequence each plan sees: with one plan for both,
    // 1 + degree multiplies per iteration; with two, one on the plan and degree on the polynomial's.
    const bool same = poly == P;
    auto plan_walk = [&](int it) { return walk_of(same ? it * (degree + 1) : it); };
    auto poly_walk = [&](int it, int j) { return walk_of(same ? it * (degree + 1) + j : it * degree + j - 1); };
    // Z = M^-1 R for the live columns, the partials of r.z in slot number rz; t shares the vector of q
    auto precondition = [&](const PcgState& S, int it, int rz) -> int {
        for_each_group(k, [&](auto K, int c0) {
            hipLaunchKernelGGL(cheb_multi_start_kernel<decltype(K)::value>, dim3(S.grid), dim3(kThreads), 0, S.st, n, S.R, dinv, coef0, D, S.Z,
                               S.s, S.active, c0, degree == 0 ? rz : -1);
        });
        for (int j = 1; j <= degree; ++j) {
            const int e = ehyb_spmm(poly, D, n, S.Q, n, k, S.st, poly_walk(it, j));  // T = A~ D in q's vector, frozen columns included
            if (e != EHYB_OK) return e;
            for_each_group(k, [&](auto K, int c0) {
                hipLaunchKernelGGL(cheb_multi_step_kernel<decltype(K)::value>, dim3(S.grid), dim3(kThreads), 0, S.st, n, j == 1 ? S.R : W, S.Q,
                                   dinv, ca[j - 1], cb[j - 1], W, D, S.Z, S.R, S.s, S.active, c0, j == degree ? rz : -1);
            });
        }
        return EHYB_OK;
    };
    return pcg_solve(who, "is the matrix symmetric positive definite, and lmax an upper bound?", P, B, ldb, X, ldx, k, max_iter, rtol,
                     check_every, stream, iters_done, rel_residual, {{&D, (size_t)n * k}, {&W, (size_t)n * k}}, prepare, plan_walk, precondition);
}

}  // namespace

extern "C" int ehyb_cheb_coeffs(double lmin, double lmax, int degree, double* c0, double* a, double* b)
{
    clear_error();
    if (degree < 0 || degree > EHYB_CHEB_MAX_DEGREE) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_cheb_coeffs: degree %d (0 .. %d)", degree, EHYB_CHEB_MAX_DEGREE);
    if (!(lmin > 0) || !(lmax > lmin) || !std::isfinite(lmax)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_cheb_coeffs: needs 0 < lmin < lmax, got %g, %g", lmin, lmax);
    if (!c0 || (degree > 0 && (!a || !b))) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_cheb_coeffs: null argument");
    const double theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta;
    *c0 = 1.0 / theta;
    double rho = 1.0 / sigma;
    for (int j = 1; j <= degree; ++j) {
        const double rho_j = 1.0 / (2.0 * sigma - rho);
        a[j - 1] = rho_j * rho;
        b[j - 1] = 2.0 * rho_j / delta;
        rho = rho_j;
    }
    return EHYB_OK;
}

extern "C" int ehyb_lambda_max(ehyb_plan* P, const double* dinv, int iters, void* stream, double* lambda)
{
    int rc = solve_args("ehyb_lambda_max", P, lambda != nullptr, 0, 0.0);
    if (rc != EHYB_OK) return rc;
    if (iters < 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lambda_max: %d steps (at least 1)", iters);
    if ((rc = solve_uploaded("ehyb_lambda_max", P)) != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    SolveLoop L(n, 0);
    double *u, *q, *s;
    HIP_TRY(L.begin(stream, {&u, &q}, n, &s, M_COUNT));
    const hipStream_t st = L.st;
    hipLaunchKernelGGL(lambda_start_kernel, dim3(L.grid), dim3(kThreads), 0, st, n, u, s);
    // step j = 0 .. iters: the Rayleigh quotient of v_j, then v_{j+1}; the last step's quotient is the answer
    for (int j = 0; j <= iters; ++j) {
        if ((rc = ehyb_spmv_walk(P, u, q, st, walk_of(j))) != EHYB_OK) return rc;
        hipLaunchKernelGGL(lambda_step_kernel, dim3(L.grid), dim3(kThreads), 0, st, n, u, q, dinv, s, j & 1);
    }
    HIP_TRY(L.read());
    *lambda = L.sum(M_VQ) / L.sum(M_VDV);
    if (!(*lambda > 0) || !std::isfinite(*lambda))
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_lambda_max: the estimate is %g (is the matrix symmetric positive definite?)", *lambda);
    return EHYB_OK;
}

extern "C" int ehyb_pcg_cheb(ehyb_plan* P, ehyb_plan* poly, const double* dinv, const double* b, double* x, int degree, double lmin,
                             double lmax, int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const char* who = "ehyb_pcg_cheb";
    int rc = solve_args(who, P, b && x, max_iter, rtol);
    if (rc != EHYB_OK) return rc;
    if (!poly) poly = P;
    if ((rc = cheb_args(who, P, poly, degree, lmin, lmax)) != EHYB_OK) return rc;
    if ((rc = solve_uploaded(who, P)) != EHYB_OK || (rc = solve_uploaded("ehyb_pcg_cheb (the polynomial's plan)", poly)) != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    return cheb_solve(who, P, poly, dinv, b, n, x, n, 1, degree, lmin, lmax, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

extern "C" int ehyb_pcg_cheb_multi(ehyb_plan* P, ehyb_plan* poly, const double* dinv, const double* B, int64_t ldb, double* X, int64_t ldx,
                                   int k, int degree, double lmin, double lmax, int max_iter, double rtol, int check_every, void* stream,
                                   int* iters_done, double* rel_residual)
{
    const char* who = "ehyb_pcg_cheb_multi";
    int rc = multi_args(who, P, ldb, ldx, k);
    if (rc == EHYB_OK) rc = solve_args(who, P, B && X, max_iter, rtol);
    if (rc != EHYB_OK) return rc;
    if (!poly) poly = P;
    if ((rc = cheb_args(who, P, poly, degree, lmin, lmax)) != EHYB_OK) return rc;
    if ((rc = solve_uploaded(who, P)) != EHYB_OK || (rc = solve_uploaded("ehyb_pcg_cheb_multi (the polynomial's plan)", poly)) != EHYB_OK) return rc;
    return cheb_solve(who, P, poly, dinv, B, ldb, X, ldx, k, degree, lmin, lmax, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

// ------------------------------------------------------------------ the two kernels one at a time (as ehyb_cg_*_step)
extern "C" int ehyb_cheb_start_step(int n, const double* r, const double* dinv, double c0, double* d, double* z, double* s, int rz,
                                    void* stream)
{
    int rc = check_step("ehyb_cheb_start_step", rz >= -1 && rz <= 1 ? n : -1, {r, d, z, rz >= 0 ? s : r});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(cheb_multi_start_kernel<1>, dim3(kMaxGrid / 2), dim3(kThreads), 0, (hipStream_t)stream, n, r, dinv, c0, d, z, s, nullptr,
                       0, rz);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_cheb_step(int n, const double* w_in, const double* t, const double* dinv, double a, double b, double* w_out, double* d,
                              double* z, const double* r, double* s, int rz, void* stream)
{
    int rc = check_step("ehyb_cheb_step", rz >= -1 && rz <= 1 ? n : -1, {w_in, t, w_out, d, z, rz >= 0 ? r : t, rz >= 0 ? s : t});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(cheb_multi_step_kernel<1>, dim3(kMaxGrid / 2), dim3(kThreads), 0, (hipStream_t)stream, n, w_in, t, dinv, a, b, w_out, d,
                       z, r, s, nullptr, 0, rz);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
