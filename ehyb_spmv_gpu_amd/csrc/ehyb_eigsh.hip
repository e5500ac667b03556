// Thick-restart Lanczos with full reorthogonalisation for the nev largest or smallest eigenpairs of the plan's symmetric matrix
// (ehyb_eigsh), entirely on the device but for the projected problem: the host looks once per restart cycle, solves T y = theta y
// for a T of at most 64 x 64 (ehyb_sym_eig), decides convergence and uploads the rotation.
//
// The orthogonalisation is GMRES's, kernel for kernel (gmres_device.h): the basis V, column-major with an even leading dimension,
// dots and update twice per step on GMRES's slot and tail layout.  The status and the counter keep their meaning (the counter
// counts multiplies), the two Hessenberg copies are h after each pass, the R area is T (column j, rows 0 .. j: the upper
// triangle, which is all ehyb_sym_eig reads) and gt[j + 1] holds beta_{j+1}.
//
// A step j (the basis holds v_0 .. v_j):  w = A z, z = scale o v_j;  [scale: w = scale o w];  dots, update, dots, update;
//   next(j)  beta^2 = w.w, h from Hessenberg copy 1.  A non-finite one: breakdown.  beta^2 <= 2^-90 (h.h + beta^2): an invariant
//            subspace -- column j, beta = 0 and the counter are written, the status becomes converged and no v_{j+1} is written.
//            Else column j, beta, the counter; v_{j+1} = w / beta, z = scale o v_{j+1}.
// Every workgroup of next() decides for itself from the same words and workgroup 0 alone writes the tail, to words the launch does
// not read (but the counter, which it owns) -- the rule of ehyb_gmres.hip.
//
// A restart keeps kk Ritz vectors: V2[:, i] = sum_l Y[l, i] v_l for i < kk and the old v_J as column kk (Y gets the extra column
// e_J), one launch of the rotation kernel into a second buffer of keep + 1 columns and one device-to-device copy back.  The next
// cycle starts at j = kk; its first column re-measures the arrow entries through the full orthogonalisation.  The final Ritz vectors
// are the same kernel writing into the caller's array.
//
// The host knows j for every launch: the first cycle and a cycle after a short restart are plain launches, the steady cycle
// (j = keep .. m - 1) is captured once as a linear hipGraph and replayed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ehyb_internal.h"
#include "gmres_device.h"
#include "solve_loop.h"

using namespace ehyb;

namespace {

constexpr double kInvariant = 0x1p-90;  // beta^2 <= 2^-90 (h.h + beta^2): the orthogonalisation removed all but 2^-45 of w
// what next() decides: go on; an invariant subspace (the step counts); breakdown before the step counts
enum { E_GO = 0, E_INVARIANT = 1, E_BREAK = 2 };

// j = -1: w.w from the partials; zero or non-finite: breakdown; else beta_0 = sqrt(w.w) into gt[0], v_0 = w / beta_0.
// j >= 0: the step rules above.  With every new v: z = scale o v.
__global__ __launch_bounds__(kThreads) void eigsh_next_kernel(int n, long long ld_, double* __restrict__ V, const double* __restrict__ w,
                                                              const double* __restrict__ scale, double* __restrict__ z,
                                                              const double* __restrict__ s, double* tail, int j)
{
    if (!running(tail)) return;
    double sums[1];
    sums[0] = partials_of(gslot(s, G_WW));
    block_sum_n(sums);
    __shared__ double h_sh[kCols], beta_sh;
    __shared__ int code_sh;
    if (j >= 0 && (int)threadIdx.x <= j) h_sh[threadIdx.x] = tail[T_H + kCols + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        int code = E_GO;
        const double ww = sums[0];
        if (j < 0) {
            if (!isfinite(ww) || !(ww > 0)) code = E_BREAK;
        } else {
            double hh = 0.0;
            bool finite = isfinite(ww);
            for (int i = 0; i <= j; ++i) {
                finite = finite && isfinite(h_sh[i]);
                hh = fma(h_sh[i], h_sh[i], hh);
            }
            if (!finite || !isfinite(hh + ww))
                code = E_BREAK;
            else if (ww <= kInvariant * (hh + ww))
                code = E_INVARIANT;
        }
        beta_sh = code == E_GO ? sqrt(ww) : 0.0;
        code_sh = code;
    }
    __syncthreads();
    const int code = __builtin_amdgcn_readfirstlane(code_sh);
    const double beta = beta_sh;
    if (blockIdx.x == 0) {
        int* flags = (int*)(tail + T_FLAGS);
        if (j >= 0 && code != E_BREAK && (int)threadIdx.x <= j) tail[T_R + (size_t)j * kM + threadIdx.x] = h_sh[threadIdx.x];
        if (threadIdx.x == 0) {
            if (code != E_BREAK) {
                tail[T_GT + j + 1] = beta;
                if (j >= 0) flags[F_ITERS] += 1;
            }
            if (code != E_GO) __atomic_store_n(&flags[F_STATUS], code == E_INVARIANT ? ST_CONVERGED : ST_BREAKDOWN, __ATOMIC_RELAXED);
        }
    }
    if (code != E_GO) return;
    const size_t ld = (size_t)ld_;
    double* v = V + (size_t)(j + 1) * ld;
    const int stride = (int)gridDim.x * kThreads;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        if (i + 1 < (size_t)n) {
            const double2 wv = load2(w + i);
            double2 vv;
            vv.x = wv.x / beta;
            vv.y = wv.y / beta;
            store2(v + i, vv);
            if (scale) {
                const double2 d = load2(scale + i);
                vv.x *= d.x;
                vv.y *= d.y;
            }
            store2(z + i, vv);
        } else {
            const double vi = w[i] / beta;
            v[i] = vi;
            z[i] = scale ? vi * scale[i] : vi;
        }
    }
}

// w = scale o w
__global__ __launch_bounds__(kThreads) void eigsh_scale_kernel(int n, const double* __restrict__ scale, double* __restrict__ w,
                                                               const double* tail)
{
    if (!running(tail)) return;
    const int stride = (int)gridDim.x * kThreads;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        if (i + 1 < (size_t)n) {
            const double2 d = load2(scale + i);
            double2 wv = load2(w + i);
            wv.x *= d.x;
            wv.y *= d.y;
            store2(w + i, wv);
        } else {
            w[i] *= scale[i];
        }
    }
}

// dst[:, c] = sum_{l < mc} Y[l, c] src[:, l] for c < kc, the sum in rising l.  Y (mc x kc, column-major, leading dimension mc) is
// staged in LDS row by row with the columns padded with zeros to a whole register group, so that every group runs the same
// arithmetic on 8 accumulators and only the stores look at kc.  src is read once per group of 8 output columns.
__global__ __launch_bounds__(kThreads) void eigsh_rotate_kernel(int n, long long ld_src, const double* __restrict__ src, long long ld_dst,
                                                                double* __restrict__ dst, const double* __restrict__ Y, int mc, int kc)
{
    __shared__ double y_sh[kCols * kM];
    const int kpad = (kc + kGroup - 1) / kGroup * kGroup;
    for (int k = threadIdx.x; k < mc * kpad; k += kThreads) {
        const int l = k / kpad, c = k - l * kpad;
        y_sh[l * kM + c] = c < kc ? Y[(size_t)c * mc + l] : 0.0;
    }
    __syncthreads();
    const size_t lds = (size_t)ld_src, ldd = (size_t)ld_dst;
    const int stride = (int)gridDim.x * kThreads;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        const bool pair = i + 1 < (size_t)n;
        for (int c0 = 0; c0 < kc; c0 += kGroup) {
            double2 acc[kGroup];
#pragma unroll
            for (int c = 0; c < kGroup; ++c) acc[c] = {0.0, 0.0};
            if (pair) {
#pragma unroll 4
                for (int l = 0; l < mc; ++l) {
                    const double2 sv = load2(src + (size_t)l * lds + i);
                    const double* y = y_sh + l * kM + c0;
#pragma unroll
                    for (int c = 0; c < kGroup; ++c) {
                        acc[c].x = fma(y[c], sv.x, acc[c].x);
                        acc[c].y = fma(y[c], sv.y, acc[c].y);
                    }
                }
#pragma unroll
                for (int c = 0; c < kGroup; ++c)
                    if (c0 + c < kc) store2(dst + (size_t)(c0 + c) * ldd + i, acc[c]);
            } else {
                for (int l = 0; l < mc; ++l) {
                    const double sv = src[(size_t)l * lds + i];
                    const double* y = y_sh + l * kM + c0;
#pragma unroll
                    for (int c = 0; c < kGroup; ++c) acc[c].x = fma(y[c], sv, acc[c].x);
                }
#pragma unroll
                for (int c = 0; c < kGroup; ++c)
                    if (c0 + c < kc) dst[(size_t)(c0 + c) * ldd + i] = acc[c].x;
            }
        }
    }
}

// ------------------------------------------------------------------ the driver
struct Launcher {
    int grid, n;
    long long ld;
    hipStream_t st;
    double *V, *w, *z, *s, *tail;
    const double* scale;

    void dots(int cnt) const { hipLaunchKernelGGL(gmres_dots_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, V, w, cnt, s, tail); }
    void update(int cnt, int pass, int last) const
    {
        hipLaunchKernelGGL(gmres_update_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, V, w, cnt, s, tail, pass, last);
    }
    void next(int j) const { hipLaunchKernelGGL(eigsh_next_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, V, w, scale, z, s, tail, j); }
    void scale_w() const { hipLaunchKernelGGL(eigsh_scale_kernel, dim3(grid), dim3(kThreads), 0, st, n, scale, w, tail); }
    void rotate(long long ld_dst, double* dst, const double* Y, int mc, int kc) const
    {
        hipLaunchKernelGGL(eigsh_rotate_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, V, ld_dst, dst, Y, mc, kc);
    }
};

struct Outputs {
    double *evals, *resid;
    int *found, *nconv, *multiplies, *restarts;
    void counts(int f, int c, int mu, int r) const
    {
        if (found) *found = f;
        if (nconv) *nconv = c;
        if (multiplies) *multiplies = mu;
        if (restarts) *restarts = r;
    }
};

int eigsh_solve(ehyb_plan* P, const double* scale, const double* v0, int nev, int which, int m, int keep, int max_restarts, double tol,
                double* evecs, int64_t ldv, void* stream, const Outputs& out)
{
    const int n = P->host.n_cols;
    const size_t ld = (size_t)n + (n & 1);
    SolveLoop L(n, 0);
    double *w, *z, *s;
    HIP_TRY(L.begin(stream, {&w, &z}, ld, &s, G_COUNT, T_COUNT));
    DeviceArray V, V2, Yd;
    HIP_TRY(hipMalloc((void**)&V.p, std::max<size_t>(1, ld * (size_t)(m + 1)) * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&V2.p, std::max<size_t>(1, ld * (size_t)(keep + 1)) * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&Yd.p, (size_t)kCols * kM * sizeof(double)));
    const hipStream_t st = L.st;
    double* tail = s + (size_t)G_COUNT * kMaxGrid;
    const Launcher K{L.grid, n, (long long)ld, st, V.p, w, z, s, tail, scale};
    HIP_TRY(hipMemsetAsync(tail, 0, (size_t)T_COUNT * sizeof(double), st));

    // the start vector into w, its norm through the update kernel without columns, v_0 and z through next(-1)
    std::vector<double> start;
    if (v0) {
        HIP_TRY(hipMemcpyAsync(w, v0, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    } else {
        start.resize(n);
        for (int i = 0; i < n; ++i) start[i] = 1.0 + (double)(i % 7) * 0.125;
        HIP_TRY(hipMemcpyAsync(w, start.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    K.update(0, 0, 1);
    K.next(-1);

    // steps j0 .. j1 - 1; the multiplies state their walk, alternating
    auto cycle = [&](int j0, int j1) -> int {
        for (int j = j0; j < j1; ++j) {
            const int rc = ehyb_spmv_walk(P, z, w, st, j & 1 ? EHYB_WALK_LAST_TO_FIRST : EHYB_WALK_FIRST_TO_LAST);
            if (rc != EHYB_OK) return rc;
            if (scale) K.scale_w();
            for (int p = 0; p < 2; ++p) {
                K.dots(j + 1);
                K.update(j + 1, p, p);
            }
            K.next(j);
        }
        return EHYB_OK;
    };

    CycleGraph G;  // the steady cycle keep .. m - 1, captured when it is first needed
    bool tried = P->cfg.graphs == 2;
    std::vector<double> th((size_t)T_COUNT), T((size_t)kM * kM, 0.0), theta(kM), Yr((size_t)kM * kM), Y((size_t)kCols * kM), res(kM);
    int f[F_COUNT] = {ST_RUNNING, 0};
    int k = 0, restarts = 0, J = 0, want = 0, nconv = 0;
    // Ritz pair i from the wanted end is column col(i) of the rising order
    auto col = [&](int i) { return which == EHYB_EIG_LARGEST ? J - 1 - i : i; };
    for (;;) {
        if (k == keep && k > 0 && !tried) {
            tried = true;
            if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                const int erc = cycle(keep, m);
                const hipError_t eend = hipStreamEndCapture(st, &G.graph);
                if (erc != EHYB_OK || eend != hipSuccess || hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0) != hipSuccess)
                    G.exec = nullptr;
                (void)hipGetLastError();
            }
        }
        if (k == keep && k > 0 && G.exec) {
            HIP_TRY(hipGraphLaunch(G.exec, st));
        } else {
            const int rc = cycle(k, m);
            if (rc != EHYB_OK) return rc;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(th.data(), tail, th.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int before = f[F_ITERS];
        std::memcpy(f, &th[T_FLAGS], sizeof(f));
        if (f[F_STATUS] == ST_BREAKDOWN) {
            out.counts(0, 0, f[F_ITERS], restarts);
            EHYB_FAIL(EHYB_ERR_ARG, "ehyb_eigsh: breakdown after %d multiplies (a zero or non-finite start vector, or a non-finite entry of the "
                                    "projected matrix)",
                      f[F_ITERS]);
        }
        const bool invariant = f[F_STATUS] == ST_CONVERGED;
        J = k + (f[F_ITERS] - before);
        for (int j = k; j < J; ++j)
            for (int i = 0; i <= j; ++i) T[(size_t)j * kM + i] = th[T_R + (size_t)j * kM + i];
        const double beta = invariant ? 0.0 : th[T_GT + J];
        const int rc = ehyb_sym_eig(J, T.data(), kM, theta.data(), Yr.data());
        if (rc != EHYB_OK) return rc;
        const double nrm = std::max(std::fabs(theta[0]), std::fabs(theta[J - 1]));
        want = std::min(nev, J);
        for (int i = 0; i < J; ++i) res[i] = std::fabs(beta * Yr[(size_t)col(i) * J + (J - 1)]);
        for (nconv = 0; nconv < want && res[nconv] <= tol * nrm;) ++nconv;
        if (nconv == want || invariant || restarts == max_restarts) break;

        // the restart: kk Ritz vectors and the old v_J, rotated into V2 and copied back; T = diag(theta)
        const int kk = std::min(keep, J - 1), mc = J + 1;
        std::fill(Y.begin(), Y.begin() + (size_t)mc * (kk + 1), 0.0);
        for (int i = 0; i < kk; ++i) std::memcpy(&Y[(size_t)i * mc], &Yr[(size_t)col(i) * J], (size_t)J * sizeof(double));
        Y[(size_t)kk * mc + J] = 1.0;
        HIP_TRY(hipMemcpyAsync(Yd.p, Y.data(), (size_t)mc * (kk + 1) * sizeof(double), hipMemcpyHostToDevice, st));
        K.rotate((long long)ld, V2.p, Yd.p, mc, kk + 1);
        HIP_TRY(hipMemcpyAsync(V.p, V2.p, ld * (size_t)(kk + 1) * sizeof(double), hipMemcpyDeviceToDevice, st));
        std::fill(T.begin(), T.end(), 0.0);
        for (int i = 0; i < kk; ++i) T[(size_t)i * kM + i] = theta[col(i)];
        HIP_TRY(hipStreamSynchronize(st));  // Y is the host's again
        k = kk;
        ++restarts;
    }
    for (int i = 0; i < want; ++i) {
        if (out.evals) out.evals[i] = theta[col(i)];
        if (out.resid) out.resid[i] = res[i];
    }
    if (evecs && want > 0) {
        for (int i = 0; i < want; ++i) std::memcpy(&Y[(size_t)i * J], &Yr[(size_t)col(i) * J], (size_t)J * sizeof(double));
        HIP_TRY(hipMemcpyAsync(Yd.p, Y.data(), (size_t)J * want * sizeof(double), hipMemcpyHostToDevice, st));
        K.rotate((long long)ldv, evecs, Yd.p, J, want);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    out.counts(want, nconv, f[F_ITERS], restarts);
    return EHYB_OK;
}

}  // namespace

extern "C" int ehyb_eigsh(ehyb_plan* P, const double* scale, const double* v0, int nev, int which, int basis, int max_restarts, double tol,
                          double* evals, double* evecs, int64_t ldv, void* stream, int* found, int* nconv, int* multiplies, int* restarts,
                          double* resid)
{
    clear_error();
    if (!P) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_eigsh: null argument");
    if (nev < 1 || nev > EHYB_EIGSH_MAX_NEV || (which != EHYB_EIG_LARGEST && which != EHYB_EIG_SMALLEST) ||
        (basis != 0 && (basis < nev + 2 || basis > EHYB_EIGSH_MAX_BASIS)) || max_restarts < 0)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_eigsh: nev %d (1 .. %d), which %d (0 or 1), basis %d (0 or nev + 2 .. %d), max_restarts %d", nev,
                  EHYB_EIGSH_MAX_NEV, which, basis, EHYB_EIGSH_MAX_BASIS, max_restarts);
    if (!(tol >= 0)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_eigsh: tol %g", tol);
    if (P->host.row_begin != 0 || P->host.row_end != P->host.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_eigsh: needs a plan over all rows");
    const int n = P->host.n_cols;
    if (evecs && (ldv < n || (ldv & 1))) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_eigsh: ldv %lld must be even and >= %d rows", (long long)ldv, n);
    if ((((uintptr_t)evecs | (uintptr_t)scale | (uintptr_t)v0) & 15) != 0)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_eigsh: evecs_dev, scale_dev and v0_dev must be 16-byte aligned");
    const int rc = solve_uploaded("ehyb_eigsh", P);
    if (rc != EHYB_OK) return rc;
    const Outputs out{evals, resid, found, nconv, multiplies, restarts};
    if (n < 1) {
        out.counts(0, 0, 0, 0);
        return EHYB_OK;
    }
    int m = 0, keep = 0;
    ehyb_eigsh_basis(nev, basis, n, &m, &keep);
    return eigsh_solve(P, scale, v0, nev, which, m, keep, max_restarts, tol, evecs, ldv, stream, out);
}

// host only: the effective basis and the number of Ritz vectors a restart keeps
extern "C" int ehyb_eigsh_basis(int nev, int basis, int n, int* m_out, int* keep_out)
{
    const int b = basis == 0 ? std::min(std::max(2 * nev + 1, 20), EHYB_EIGSH_MAX_BASIS) : basis;
    const int m = std::min(b, n);
    if (m_out) *m_out = m;
    if (keep_out) *keep_out = nev + std::max(m - nev, 0) / 2;
    return EHYB_OK;
}

// ------------------------------------------------------------------ building blocks: one launch each, slot_doubles / 2 workgroups
extern "C" int ehyb_eigsh_next_step(int n, int64_t ld, double* V, const double* w, const double* scale, double* z, double* s, int j,
                                    void* stream)
{
    clear_error();
    int rc = check_step("ehyb_eigsh_next_step", n, {V, w, z, s});
    if (rc != EHYB_OK) return rc;
    if (j < -1 || j >= kM) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_eigsh_next_step: bad arguments (j %d, -1 .. %d)", j, kM - 1);
    if ((rc = check_pairs("ehyb_eigsh_next_step", n, ld, {V, w, scale, z})) != EHYB_OK) return rc;
    hipLaunchKernelGGL(eigsh_next_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, (long long)ld, V, w, scale, z, s,
                       step_tail(s), j);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_eigsh_scale_step(int n, const double* scale, double* w, double* s, void* stream)
{
    clear_error();
    int rc = check_step("ehyb_eigsh_scale_step", n, {scale, w, s});
    if (rc != EHYB_OK) return rc;
    if ((rc = check_pairs("ehyb_eigsh_scale_step", n, n + (n & 1), {scale, w})) != EHYB_OK) return rc;
    hipLaunchKernelGGL(eigsh_scale_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, scale, w, step_tail(s));
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_eigsh_rotate_step(int n, int64_t ld_src, const double* src, int64_t ld_dst, double* dst, const double* Y, int mc, int kc,
                                      void* stream)
{
    clear_error();
    int rc = check_step("ehyb_eigsh_rotate_step", n, {src, dst, Y});
    if (rc != EHYB_OK) return rc;
    if (mc < 1 || mc > kCols || kc < 1 || kc > kM)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_eigsh_rotate_step: bad arguments (mc %d, 1 .. %d; kc %d, 1 .. %d)", mc, kCols, kc, kM);
    if ((rc = check_pairs("ehyb_eigsh_rotate_step", n, ld_src, {src})) != EHYB_OK) return rc;
    if ((rc = check_pairs("ehyb_eigsh_rotate_step", n, ld_dst, {dst})) != EHYB_OK) return rc;
    hipLaunchKernelGGL(eigsh_rotate_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, (long long)ld_src, src,
                       (long long)ld_dst, dst, Y, mc, kc);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
