// Device-resident restarted GMRES(m) for unsymmetric systems on top of the EHYB plan (ehyb_gmres), right-preconditioned with
// M = diag(A): the method for the systems on which ehyb_bicgstab breaks down or diverges.  Unlike every other solver here it
// keeps a GROWING set of vectors: the Arnoldi basis V, column-major, m + 1 columns with a leading dimension of n rounded up
// to even, so that every column is 16-byte aligned.  Beside it two fixed vectors: z = M^-1 v_j, the multiply's input, and w,
// its output.  ehyb_gmres_t is the same driver with one flag set: every multiply is ehyb_spmv_t, the system solved A^T x = b (the
// diagonal of A^T is A's: M stays); its multiplies add with atomics, so its outputs are reproducible up to summation order only.
//
// A cycle: w = A x;  start: w = b - w, partials of w.w (= r.r) and b.b;  next(-1): v_0 = w / sqrt(r.r), z = M^-1 v_0;
// then per step j = 0 .. m-1 one multiply and 2 * passes + 1 vector kernels
//   w = A z                                                   (ehyb_spmv_walk, walks alternating)
//   per pass:  dots    partials of c_i = v_i . w, i <= j, all from the same w: the columns in register groups of 8
//              update  w -= sum c_i v_i;  workgroup 0: h_i (+)= c_i;  on the last pass the partials of w.w
//   next(j)    h_{j+1} = sqrt(w.w); the Hessenberg column through the rotations 0 .. j-1, the new rotation, g, the counter
//              and the stop tests;  v_{j+1} = w / h_{j+1},  z = M^-1 v_{j+1}
// and at the end  solve_x: R y = g by back substitution, x += M^-1 (sum y_i v_i) over the J steps the device counted.
// The host knows j for every launch of a cycle, so j and the column count are kernel arguments and a whole cycle is one linear
// hipGraph, replayed per cycle; a last partial cycle is issued as plain launches.  The host looks once per cycle.
//
// Sums come from per-workgroup partials re-added in a fixed order (vec_reduce.h); no atomics.  What no sum gives back lives in
// the tail behind the slots: the rotations cs, sn, R (64 x 64, column-major), g~ (the unrotated right-hand side, g~_0 = beta)
// and g (the rotated one), one Hessenberg column per pass, rho, b.b, and three ints: status, counter, the counter at the cycle
// start.  Every workgroup of next() makes the whole decision for itself from the same words (so all take the same branch) and
// workgroup 0 alone writes the tail -- always to words that the launch does not read: step j reads cs, sn of i < j and g~_j and
// writes cs_j, sn_j, g_j, g~_{j+1} and column j of R; pass p of update reads Hessenberg copy p - 1 and writes copy p.  (The one
// exception is the house's: the counter, which only workgroup 0 touches.)  Once the status is set every kernel but solve_x
// returns at once; solve_x applies the steps counted in the cycle whatever the status.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "bilu.h"
#include "ehyb_internal.h"
#include "gmres_device.h"
#include "solve_loop.h"

using namespace ehyb;

namespace {

// what next() decides: go on; converged (counted, but for j = -1); breakdown before the step counts; breakdown after it counted
enum { D_GO = 0, D_CONVERGED = 1, D_BREAK_EARLY = 2, D_BREAK_COUNTED = 3 };

// ------------------------------------------------------------------ the vector kernels
// Every kernel but start walks PAIRS of elements: pair p = (2p, 2p + 1) with p = block * 256 + thread, stride grid * 256, one
// 16-byte access per vector and pair; for an odd n the last element is a pair of one and goes through 8-byte accesses.

// w = b - w (w = A x on entry); partials of w.w and b.b
__global__ __launch_bounds__(kThreads) void gmres_start_kernel(int n, const double* __restrict__ b, double* __restrict__ w,
                                                               double* __restrict__ s, const double* tail)
{
    if (!running(tail)) return;
    double sums[2] = {0.0, 0.0};
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const double bi = b[i], ri = bi - w[i];
        w[i] = ri;
        sums[0] = fma(ri, ri, sums[0]);
        sums[1] = fma(bi, bi, sums[1]);
    }
    block_sum_n(sums);
    if (threadIdx.x == 0) {
        gslot(s, G_WW)[blockIdx.x] = sums[0];
        gslot(s, G_BB)[blockIdx.x] = sums[1];
    }
}

// j = -1, the cycle start: w.w = r.r and b.b from the partials; a non-finite one: breakdown; r.r <= thr bb: converged; else
// beta = sqrt(r.r), g~_0 = beta, v_0 = w / beta.  Workgroup 0 also notes the counter at the cycle start, rho = r.r and bb.
// j >= 0: h_{j+1} = sqrt(w.w); h_0 .. h_j from Hessenberg copy passes - 1; a non-finite h: breakdown.  The rotations 0 .. j-1 on
// the column, gamma = hypot(h_j, h_{j+1}); zero or non-finite: breakdown.  cs_j, sn_j, column j of R, g~_{j+1} = -sn_j g~_j,
// g_j = cs_j g~_j, rho = g~_{j+1}^2, counter + 1.  Then g~_{j+1}^2 <= thr bb: converged; the unrotated h_{j+1} = 0: breakdown;
// else v_{j+1} = w / h_{j+1}.  With every new v: z = M^-1 v.
__global__ __launch_bounds__(kThreads) void gmres_next_kernel(int n, long long ld_, double* __restrict__ V, const double* __restrict__ w,
                                                              const double* __restrict__ dinv, double* __restrict__ z,
                                                              const double* __restrict__ s, double* tail, int j, int passes, double thr)
{
    if (!running(tail)) return;
    double sums[2];
    sums[0] = partials_of(gslot(s, G_WW));
    sums[1] = j < 0 ? partials_of(gslot(s, G_BB)) : 0.0;
    block_sum_n(sums);
    __shared__ double h_sh[kCols], cs_sh[kM], sn_sh[kM], out_sh[8];
    __shared__ int code_sh;
    if (j >= 0) {
        const int t = threadIdx.x;
        if (t <= j) h_sh[t] = tail[T_H + (passes - 1) * kCols + t];
        if (t < j) {
            cs_sh[t] = tail[T_CS + t];
            sn_sh[t] = tail[T_SN + t];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int code = D_GO;
        const double ww = sums[0];
        double hn = sqrt(ww), gamma = 0.0, cs = 0.0, sn = 0.0, gfin = 0.0, gnext = 0.0, bb = 0.0;
        if (j < 0) {
            const double bb0 = sums[1];
            bb = bb0 > 0 ? bb0 : (bb0 == 0 ? 1.0 : bb0);
            if (!isfinite(bb0) || !isfinite(ww))
                code = D_BREAK_EARLY;
            else if (ww <= thr * bb)
                code = D_CONVERGED;
        } else {
            bool finite = isfinite(ww);
            for (int i = 0; i <= j; ++i) finite = finite && isfinite(h_sh[i]);
            if (!finite) {
                code = D_BREAK_EARLY;
            } else {
                for (int i = 0; i < j; ++i) {
                    const double a = h_sh[i], b = h_sh[i + 1], t = fma(cs_sh[i], a, sn_sh[i] * b);
                    h_sh[i + 1] = fma(-sn_sh[i], a, cs_sh[i] * b);
                    h_sh[i] = t;
                }
                gamma = hypot(h_sh[j], hn);
                if (gamma == 0 || !isfinite(gamma)) {
                    code = D_BREAK_EARLY;
                } else {
                    cs = h_sh[j] / gamma;
                    sn = hn / gamma;
                    const double gt = tail[T_GT + j];
                    gnext = -sn * gt;
                    gfin = cs * gt;
                    bb = tail[T_BB];
                    if (gnext * gnext <= thr * bb)
                        code = D_CONVERGED;
                    else if (hn == 0)
                        code = D_BREAK_COUNTED;
                }
            }
        }
        out_sh[0] = hn;
        out_sh[1] = gamma;
        out_sh[2] = cs;
        out_sh[3] = sn;
        out_sh[4] = gfin;
        out_sh[5] = gnext;
        out_sh[6] = bb;
        code_sh = code;
    }
    __syncthreads();
    const int code = __builtin_amdgcn_readfirstlane(code_sh);
    const double hn = out_sh[0];
    if (blockIdx.x == 0) {
        int* flags = (int*)(tail + T_FLAGS);
        if (j >= 0 && code != D_BREAK_EARLY) {
            if ((int)threadIdx.x < j) tail[T_R + (size_t)j * kM + threadIdx.x] = h_sh[threadIdx.x];
            if (threadIdx.x == 0) {
                tail[T_R + (size_t)j * kM + j] = out_sh[1];
                tail[T_CS + j] = out_sh[2];
                tail[T_SN + j] = out_sh[3];
                tail[T_G + j] = out_sh[4];
                tail[T_GT + j + 1] = out_sh[5];
                tail[T_RHO] = out_sh[5] * out_sh[5];
                flags[F_ITERS] += 1;
            }
        }
        if (threadIdx.x == 0) {
            if (j < 0) {
                ((int*)(tail + T_CYCLE))[0] = flags[F_ITERS];
                tail[T_RHO] = sums[0];
                tail[T_BB] = out_sh[6];
                if (code == D_GO) tail[T_GT] = hn;
            }
            if (code != D_GO) __atomic_store_n(&flags[F_STATUS], code == D_CONVERGED ? ST_CONVERGED : ST_BREAKDOWN, __ATOMIC_RELAXED);
        }
    }
    if (code != D_GO) return;
    const size_t ld = (size_t)ld_;
    double* v = V + (size_t)(j + 1) * ld;
    const int stride = (int)gridDim.x * kThreads;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        if (i + 1 < (size_t)n) {
            const double2 wv = load2(w + i);
            double2 vv;
            vv.x = wv.x / hn;
            vv.y = wv.y / hn;
            store2(v + i, vv);
            if (!z) continue;  // (a preconditioner that reads v where it lies: ehyb_gmres_bilu)
            if (dinv) {
                const double2 d = load2(dinv + i);
                vv.x *= d.x;
                vv.y *= d.y;
            }
            store2(z + i, vv);
        } else {
            const double vi = w[i] / hn;
            v[i] = vi;
            if (z) z[i] = dinv ? vi * dinv[i] : vi;
        }
    }
}

// J = counter - counter at the cycle start; R y = g[0 .. J) by back substitution (column by column, every workgroup for itself,
// the same order in each); x += M^-1 (sum_{i < J} y_i v_i), the sum in rising i.  Does not look at the status: the steps before
// a stop are applied.  comb (ehyb_gmres_bilu): the combination sum y_i v_i goes there and x stays -- M^-1 and the addition follow.
__global__ __launch_bounds__(kThreads) void gmres_solve_x_kernel(int n, long long ld_, const double* __restrict__ V,
                                                                 const double* __restrict__ dinv, double* __restrict__ x,
                                                                 const double* __restrict__ tail, double* __restrict__ comb)
{
    __shared__ double r_sh[kM * kM], g_sh[kM], y_sh[kM];
    __shared__ int j_sh;
    if (threadIdx.x == 0) j_sh = ((const int*)(tail + T_FLAGS))[F_ITERS] - ((const int*)(tail + T_CYCLE))[0];
    __syncthreads();
    const int J = __builtin_amdgcn_readfirstlane(j_sh);
    if (J <= 0 || J > kM) return;
    for (int k = threadIdx.x; k < J * kM; k += kThreads) r_sh[k] = tail[T_R + k];
    if ((int)threadIdx.x < J) g_sh[threadIdx.x] = tail[T_G + threadIdx.x];
    __syncthreads();
    for (int i = J - 1; i >= 0; --i) {
        const double yi = g_sh[i] / r_sh[i * kM + i];
        if ((int)threadIdx.x < i) g_sh[threadIdx.x] = fma(-r_sh[i * kM + threadIdx.x], yi, g_sh[threadIdx.x]);
        if ((int)threadIdx.x == kThreads - 1) y_sh[i] = yi;
        __syncthreads();
    }
    const size_t ld = (size_t)ld_;
    const int stride = (int)gridDim.x * kThreads;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        if (i + 1 < (size_t)n) {
            double2 acc = {0.0, 0.0};
            int c0 = 0;
            for (; c0 + kGroup <= J; c0 += kGroup) {
                double2 vv[kGroup];
#pragma unroll
                for (int c = 0; c < kGroup; ++c) vv[c] = load2(V + (size_t)(c0 + c) * ld + i);
#pragma unroll
                for (int c = 0; c < kGroup; ++c) {
                    const double yi = y_sh[c0 + c];
                    acc.x = fma(yi, vv[c].x, acc.x);
                    acc.y = fma(yi, vv[c].y, acc.y);
                }
            }
            for (; c0 < J; ++c0) {
                const double2 v = load2(V + (size_t)c0 * ld + i);
                acc.x = fma(y_sh[c0], v.x, acc.x);
                acc.y = fma(y_sh[c0], v.y, acc.y);
            }
            if (dinv) {
                const double2 d = load2(dinv + i);
                acc.x *= d.x;
                acc.y *= d.y;
            }
            if (comb) {
                store2(comb + i, acc);
                continue;
            }
            double2 xv = load2(x + i);
            xv.x += acc.x;
            xv.y += acc.y;
            store2(x + i, xv);
        } else {
            double acc = 0.0;
            for (int c0 = 0; c0 < J; ++c0) acc = fma(y_sh[c0], V[(size_t)c0 * ld + i], acc);
            if (dinv) acc *= dinv[i];
            if (comb)
                comb[i] = acc;
            else
                x[i] += acc;
        }
    }
}

// x += z, z = M^-1 (sum y_i v_i), if the cycle counted a step (J as in solve_x: without one, solve_x wrote no combination and z
// holds nothing of this cycle).  Does not look at the status.
__global__ __launch_bounds__(kThreads) void gmres_add_kernel(int n, const double* __restrict__ z, double* __restrict__ x,
                                                             const double* __restrict__ tail)
{
    const int J = ((const int*)(tail + T_FLAGS))[F_ITERS] - ((const int*)(tail + T_CYCLE))[0];  // (the same word in every thread)
    if (J <= 0 || J > kM) return;
    const int stride = (int)gridDim.x * kThreads;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        if (i + 1 < (size_t)n) {
            const double2 zv = load2(z + i);
            double2 xv = load2(x + i);
            xv.x += zv.x;
            xv.y += zv.y;
            store2(x + i, xv);
        } else {
            x[i] += z[i];
        }
    }
}

// ------------------------------------------------------------------ the driver
struct Launcher {
    int grid, n;
    long long ld;
    hipStream_t st;
    double *V, *w, *z, *s, *tail;
    const double* dinv;
    const ehyb_bilu* M;  // ehyb_gmres_bilu: the preconditioner, applied by ehyb_bic_apply_kernel (dinv is NULL then)

    // z = M^-1 (basis column j), read where it lies; like the vector kernels it returns at once when the status is set
    int precondition(int j) const
    {
        if (!M) return EHYB_OK;
        return bic_apply_columns(&M->core, st, V + (size_t)j * ld, ld, z, ld, 1, (const int*)(tail + T_FLAGS) + F_STATUS, 1, true);
    }
    void start(const double* b) const { hipLaunchKernelGGL(gmres_start_kernel, dim3(grid), dim3(kThreads), 0, st, n, b, w, s, tail); }
    void dots(int cnt) const { hipLaunchKernelGGL(gmres_dots_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, V, w, cnt, s, tail); }
    void update(int cnt, int pass, int last) const
    {
        hipLaunchKernelGGL(gmres_update_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, V, w, cnt, s, tail, pass, last);
    }
    void next(int j, int passes, double thr) const
    {
        hipLaunchKernelGGL(gmres_next_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, V, w, dinv, M ? nullptr : z, s, tail, j, passes, thr);
    }
    // x += M^-1 (sum y_i v_i); with M the combination goes through w (free at a cycle's end), one apply and the add kernel
    int solve_x(double* x) const
    {
        hipLaunchKernelGGL(gmres_solve_x_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, V, dinv, x, tail, M ? w : nullptr);
        if (!M) return EHYB_OK;
        const int rc = bic_apply_columns(&M->core, st, w, ld, z, ld, 1, nullptr);
        if (rc != EHYB_OK) return rc;
        hipLaunchKernelGGL(gmres_add_kernel, dim3(grid), dim3(kThreads), 0, st, n, z, x, tail);
        return EHYB_OK;
    }
};

// transposed: every multiply is ehyb_spmv_t (A^T x = b; no walk: the transposed launch has none)
int gmres_solve(const char* who, ehyb_plan* P, bool transposed, const double* dinv, const ehyb_bilu* M, const double* b, double* x, int m, int passes, int max_iter, double rtol,
                void* stream, int* iters_done, double* rel_residual)
{
    const int n = P->host.n_cols;
    const size_t ld = (size_t)n + (n & 1);
    SolveLoop L(n, 0);
    double *w, *z, *s;
    HIP_TRY(L.begin(stream, {&w, &z}, ld, &s, G_COUNT, T_COUNT));
    DeviceArray V;
    HIP_TRY(hipMalloc((void**)&V.p, std::max<size_t>(1, ld * (size_t)(m + 1)) * sizeof(double)));
    const hipStream_t st = L.st;
    double* tail = s + (size_t)G_COUNT * kMaxGrid;
    const Launcher K{L.grid, n, (long long)ld, st, V.p, w, z, s, tail, dinv, M};
    const double thr = rtol * rtol;
    HIP_TRY(hipMemsetAsync(tail, 0, (size_t)T_COUNT * sizeof(double), st));

    const auto multiply = [&](const double* in, double* out, int walk) { return transposed ? ehyb_spmv_t(P, in, out, st) : ehyb_spmv_walk(P, in, out, st, walk); };
    // one cycle of `steps` steps; the multiplies walk last to first, then alternate
    auto cycle = [&](int steps) -> int {
        int rc = multiply(x, w, EHYB_WALK_LAST_TO_FIRST);
        if (rc != EHYB_OK) return rc;
        K.start(b);
        K.next(-1, passes, thr);
        for (int j = 0; j < steps; ++j) {
            if ((rc = K.precondition(j)) != EHYB_OK) return rc;
            rc = multiply(z, w, j & 1 ? EHYB_WALK_LAST_TO_FIRST : EHYB_WALK_FIRST_TO_LAST);
            if (rc != EHYB_OK) return rc;
            for (int p = 0; p < passes; ++p) {
                K.dots(j + 1);
                K.update(j + 1, p, p == passes - 1);
            }
            K.next(j, passes, thr);
        }
        return K.solve_x(x);
    };

    // a full cycle is captured once and replayed; cfg.graphs = 2 keeps the plain launches, and so does a capture that fails
    CycleGraph G;
    if (P->cfg.graphs != 2 && max_iter >= m && hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        const int erc = cycle(m);
        const hipError_t eend = hipStreamEndCapture(st, &G.graph);
        if (erc != EHYB_OK || eend != hipSuccess || hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0) != hipSuccess) G.exec = nullptr;
        (void)hipGetLastError();
    }
    double head[4] = {0, 0, 0, 0};  // flags, cycle, rho, bb as the device left them
    int f[F_COUNT] = {ST_RUNNING, 0};
    int issued = 0;
    do {
        const int steps = std::min(m, max_iter - issued);
        if (steps == m && G.exec) {
            HIP_TRY(hipGraphLaunch(G.exec, st));
        } else {
            const int rc = cycle(steps);
            if (rc != EHYB_OK) return rc;
        }
        issued += steps;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(head, tail, sizeof(head), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::memcpy(f, &head[T_FLAGS], sizeof(f));
    } while (f[F_STATUS] == ST_RUNNING && issued < max_iter);
    if (iters_done) *iters_done = f[F_ITERS];
    if (rel_residual) *rel_residual = std::sqrt(head[T_RHO] / head[T_BB]);
    if (f[F_STATUS] != ST_BREAKDOWN) return EHYB_OK;
    EHYB_FAIL(EHYB_ERR_ARG, "%s: breakdown after %d iterations (a non-finite b.b, r.r or Hessenberg entry, a zero or non-finite gamma, "
                            "or h_{j+1} = 0 short of convergence: a singular system)",
              who, f[F_ITERS]);
}

// the checks of both entry points, in the order ehyb.h states, then the solve
int gmres_entry(const char* who, bool transposed, ehyb_plan* P, const double* dinv, const ehyb_bilu* M, bool with_bilu, const double* b, double* x, int restart, int ortho_passes,
                int max_iter, double rtol, void* stream, int* iters_done, double* rel_residual)
{
    int rc = solve_args(who, P, b && x, max_iter, rtol);
    if (rc != EHYB_OK) return rc;
    if (restart < 0 || restart > kM || ortho_passes < 0 || ortho_passes > 2)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: restart %d (0 .. %d), ortho_passes %d (0 .. 2)", who, restart, kM, ortho_passes);
    if (transposed && (rc = ehyb_spmv_t_supported(P)) != EHYB_OK) return rc;  // (the form is named in ehyb_last_error)
    if ((rc = with_bilu ? bilu_solver_args(who, P, M) : solve_uploaded(who, P)) != EHYB_OK) return rc;
    return gmres_solve(who, P, transposed, dinv, M, b, x, restart == 0 ? 30 : restart, ortho_passes == 1 ? 1 : 2, max_iter, rtol, stream, iters_done,
                       rel_residual);
}

}  // namespace

extern "C" int ehyb_gmres(ehyb_plan* P, const double* dinv, const double* b, double* x, int restart, int ortho_passes, int max_iter,
                          double rtol, void* stream, int* iters_done, double* rel_residual)
{
    return gmres_entry("ehyb_gmres", false, P, dinv, nullptr, false, b, x, restart, ortho_passes, max_iter, rtol, stream, iters_done, rel_residual);
}

extern "C" int ehyb_gmres_t(ehyb_plan* P, const double* dinv, const double* b, double* x, int restart, int ortho_passes, int max_iter,
                            double rtol, void* stream, int* iters_done, double* rel_residual)
{
    return gmres_entry("ehyb_gmres_t", true, P, dinv, nullptr, false, b, x, restart, ortho_passes, max_iter, rtol, stream, iters_done, rel_residual);
}

// right-preconditioned with the block ILU(0) of `bilu`: z = M^-1 v_j by the apply kernel on the basis column where it lies
extern "C" int ehyb_gmres_bilu(ehyb_plan* P, ehyb_bilu* bilu, const double* b, double* x, int restart, int ortho_passes, int max_iter,
                               double rtol, void* stream, int* iters_done, double* rel_residual)
{
    return gmres_entry("ehyb_gmres_bilu", false, P, nullptr, bilu, true, b, x, restart, ortho_passes, max_iter, rtol, stream, iters_done, rel_residual);
}

// ------------------------------------------------------------------ building blocks for a caller that owns the loop
// The five vector kernels one launch each, for a caller that issues the multiplies itself (and for tests that look at one kernel
// at a time) -- the analogue of ehyb_minres_*_step.  s: `slots` slots of `slot_doubles` doubles and tail_doubles more behind them
// (ehyb_gmres_layout); every launch uses slot_doubles / 2 workgroups.  Asynchronous on `stream`.
extern "C" int ehyb_gmres_layout(ehyb_gmres_slots* out)
{
    if (!out) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_gmres_layout: null argument");
    out->slots = G_COUNT;
    out->slot_doubles = kMaxGrid;
    out->slot_bb = G_BB;
    out->slot_ww = G_WW;
    out->slot_c0 = G_C0;
    out->max_restart = kM;
    out->tail_doubles = T_COUNT;
    out->flags_at = T_FLAGS;
    out->flag_status = F_STATUS;
    out->flag_iters = F_ITERS;
    out->flag_count = F_COUNT;
    out->cycle_at = T_CYCLE;
    out->rho_at = T_RHO;
    out->bb_at = T_BB;
    out->cs_at = T_CS;
    out->sn_at = T_SN;
    out->gt_at = T_GT;
    out->g_at = T_G;
    out->h_at = T_H;
    out->h_stride = kCols;
    out->r_at = T_R;
    out->r_stride = kM;
    out->status_running = ST_RUNNING;
    out->status_converged = ST_CONVERGED;
    out->status_breakdown = ST_BREAKDOWN;
    return EHYB_OK;
}


extern "C" int ehyb_gmres_start_step(int n, const double* b, double* w, double* s, void* stream)
{
    const int rc = check_step("ehyb_gmres_start_step", n, {b, w, s});
    if (rc != EHYB_OK) return rc;
    hipLaunchKernelGGL(gmres_start_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, b, w, s, step_tail(s));
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_gmres_dots_step(int n, int64_t ld, const double* V, const double* w, int count, double* s, void* stream)
{
    int rc = check_step("ehyb_gmres_dots_step", n, {V, w, s});
    if (rc != EHYB_OK) return rc;
    if (count < 1 || count > kCols) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_gmres_dots_step: bad arguments (count %d, 1 .. %d)", count, kCols);
    if ((rc = check_pairs("ehyb_gmres_dots_step", n, ld, {V, w})) != EHYB_OK) return rc;
    hipLaunchKernelGGL(gmres_dots_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, (long long)ld, V, w, count, s,
                       step_tail(s));
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_gmres_update_step(int n, int64_t ld, const double* V, double* w, int count, double* s, int pass, int last, void* stream)
{
    int rc = check_step("ehyb_gmres_update_step", n, {V, w, s});
    if (rc != EHYB_OK) return rc;
    if (count < 1 || count > kCols || pass < 0 || pass > 1)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_gmres_update_step: bad arguments (count %d, 1 .. %d; pass %d, 0 or 1)", count, kCols, pass);
    if ((rc = check_pairs("ehyb_gmres_update_step", n, ld, {V, w})) != EHYB_OK) return rc;
    hipLaunchKernelGGL(gmres_update_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, (long long)ld, V, w, count, s,
                       step_tail(s), pass, last != 0);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_gmres_next_step(int n, int64_t ld, double* V, const double* w, const double* dinv, double* z, double* s, int j,
                                    int passes, double thr, void* stream)
{
    int rc = check_step("ehyb_gmres_next_step", n, {V, w, z, s});
    if (rc != EHYB_OK) return rc;
    if (j < -1 || j >= kM || passes < 1 || passes > 2)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_gmres_next_step: bad arguments (j %d, -1 .. %d; passes %d, 1 or 2)", j, kM - 1, passes);
    if ((rc = check_pairs("ehyb_gmres_next_step", n, ld, {V, w, dinv, z})) != EHYB_OK) return rc;
    hipLaunchKernelGGL(gmres_next_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, (long long)ld, V, w, dinv, z, s,
                       step_tail(s), j, passes, thr);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_gmres_solve_x_step(int n, int64_t ld, const double* V, const double* dinv, double* x, double* s, void* stream)
{
    int rc = check_step("ehyb_gmres_solve_x_step", n, {V, x, s});
    if (rc != EHYB_OK) return rc;
    if ((rc = check_pairs("ehyb_gmres_solve_x_step", n, ld, {V, dinv, x})) != EHYB_OK) return rc;
    hipLaunchKernelGGL(gmres_solve_x_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, (long long)ld, V, dinv, x,
                       step_tail(s), nullptr);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

// solve_x with the combination written to comb_dev and x untouched (ehyb_gmres_bilu)
extern "C" int ehyb_bilu_gmres_combine_step(int n, int64_t ld, const double* V, double* comb, double* s, void* stream)
{
    int rc = check_step("ehyb_bilu_gmres_combine_step", n, {V, comb, s});
    if (rc != EHYB_OK) return rc;
    if ((rc = check_pairs("ehyb_bilu_gmres_combine_step", n, ld, {V, comb})) != EHYB_OK) return rc;
    hipLaunchKernelGGL(gmres_solve_x_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, (long long)ld, V, nullptr, nullptr, step_tail(s), comb);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

// x += z if the cycle counted a step (ehyb_gmres_bilu's last kernel of a cycle)
extern "C" int ehyb_bilu_gmres_add_step(int n, const double* z, double* x, double* s, void* stream)
{
    int rc = check_step("ehyb_bilu_gmres_add_step", n, {z, x, s});
    if (rc != EHYB_OK) return rc;
    if ((rc = check_pairs("ehyb_bilu_gmres_add_step", n, n + (n & 1), {z, x})) != EHYB_OK) return rc;
    hipLaunchKernelGGL(gmres_add_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, z, x, step_tail(s));
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
