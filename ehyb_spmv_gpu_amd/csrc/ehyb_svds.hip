// The nsv largest singular triplets of the plan's matrix by Golub-Kahan-Lanczos bidiagonalisation with full two-sided
// reorthogonalisation and a thick restart with Ritz vectors (Baglama and Reichel 2005, restarted as ehyb_eigsh restarts), entirely
// on the device but for the projected problem: the host looks once per restart cycle, takes the SVD of a B of at most 64 x 64
// (ehyb_small_svd), decides convergence and uploads the two rotations.  It works on A and A^T directly -- in the numbering and on
// the plan(s) the caller holds --, not on A^T A (which squares the condition number) nor on [0 A; A^T 0] (which doubles every
// vector and finds every sigma twice).
//
// ONE kernel is new: svds_next_kernel.  Everything else on the device is existing kernels launched as they are: GMRES's dots and
// update (gmres_device.h) on GMRES's slot and tail layout, ehyb_eigsh's rotation kernel (ehyb_eigsh_rotate_step), the multiply
// (ehyb_spmv_walk) and the transposed multiply (transpose_pair.h: ehyb_spmm on a plan of A^T, or ehyb_spmv_t on the plan of A).
//
// Two bases, column-major with the even leading dimension n + (n & 1): P, the right vectors, m + 1 columns; Q, the left ones, m
// columns.  The multiplies read their input straight from a basis column (there is no scale, so no z copy).  The status and the
// counter keep their meaning (the counter counts multiplies, two per full step), the two Hessenberg copies are the coefficients
// after each pass, the R area is B (column j, rows 0 .. j: B is upper triangular) and gt[j + 1] holds beta_{j+1}.
//
// A step j (P holds p_0 .. p_j, Q holds q_0 .. q_{j-1}):
//   left   w = A p_j;  dots, update, dots, update against Q (count j; j = 0: the norm alone);
//          next(left, j)   alpha^2 = w.w, h from Hessenberg copy 1.  A non-finite one: breakdown.  alpha^2 <= 2^-90 (h.h + alpha^2):
//                          a LEFT COLLAPSE, A p_j lies in the span of Q -- column j with alpha = 0 and the counter are written, the
//                          status becomes converged, no q_j is written.  Else column j, the counter; q_j = w / alpha.
//   right  w = A^T q_j;  dots, update, dots, update against P (count j + 1);
//          next(right, j)  beta^2 = w.w, g from Hessenberg copy 1, read for the finiteness and collapse tests only (B is measured by
//                          the left halves).  beta^2 <= 2^-90 (g.g + beta^2): an invariant subspace -- beta = 0, the counter, the
//                          status converged, no p_{j+1}.  Else beta, the counter; p_{j+1} = w / beta.
// Every workgroup of next() decides for itself from the same words and workgroup 0 alone writes the tail, to words the launch does
// not read (but the counter, which it owns) -- the rule of ehyb_gmres.hip and ehyb_eigsh.hip.  The host tells a left collapse from a
// right one by the parity of the multiplies the cycle made.
//
// A restart keeps kk triplets: two launches of the rotation kernel, P (with the old p_J as column kk) then Q, through one spare
// buffer of keep + 1 columns, each with its device-to-device copy back.  The next cycle starts at j = kk; its left half re-measures
// the arrow column beta X[J-1, i] through the full orthogonalisation: the host never plants it.  The final U and V are the same
// kernel writing into the caller's arrays.
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
#include "transpose_pair.h"

using namespace ehyb;

namespace {

constexpr double kCollapse = 0x1p-90;  // w.w <= 2^-90 (c.c + w.w): the orthogonalisation removed all but 2^-45 of w
enum { SIDE_LEFT = 0, SIDE_RIGHT = 1 };
// what next() decides: go on; a collapse (the multiply counts); breakdown before it counts
enum { S_GO = 0, S_COLLAPSE = 1, S_BREAK = 2 };

// side LEFT, j >= 0:   alpha^2 from slot G_WW, h_0 .. h_{j-1} from Hessenberg copy 1;  R[0 .. j-1, j] = h, R[j, j] = alpha (0 at a
//                      collapse), counter + 1;  q_j = w / alpha into column j of dst (Q).
// side RIGHT, j >= 0:  beta^2 from slot G_WW, g_0 .. g_j from Hessenberg copy 1, only tested;  gt[j + 1] = beta (0 at a collapse),
//                      counter + 1;  p_{j+1} = w / beta into column j + 1 of dst (P).
// side RIGHT, j = -1:  the start: w.w zero or non-finite: breakdown; else gt[0] = sqrt(w.w), p_0 = w / gt[0]; the counter stays.
// A breakdown sets the status and writes nothing else; a collapse writes no vector.  Streaming: 8 n bytes read, 8 n written.
__global__ __launch_bounds__(kThreads) void svds_next_kernel(int n, long long ld_, double* __restrict__ dst, const double* __restrict__ w,
                                                             const double* __restrict__ s, double* tail, int side, int j)
{
    if (!running(tail)) return;
    double sums[1];
    sums[0] = partials_of(gslot(s, G_WW));
    block_sum_n(sums);
    const int cnt = j < 0 ? 0 : side == SIDE_LEFT ? j : j + 1;  // coefficients of the orthogonalisation
    __shared__ double c_sh[kCols], norm_sh;
    __shared__ int code_sh;
    if ((int)threadIdx.x < cnt) c_sh[threadIdx.x] = tail[T_H + kCols + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        int code = S_GO;
        const double ww = sums[0];
        if (j < 0) {
            if (!isfinite(ww) || !(ww > 0)) code = S_BREAK;
        } else {
            double cc = 0.0;
            bool finite = isfinite(ww);
            for (int i = 0; i < cnt; ++i) {
                finite = finite && isfinite(c_sh[i]);
                cc = fma(c_sh[i], c_sh[i], cc);
            }
            if (!finite || !isfinite(cc + ww))
                code = S_BREAK;
            else if (ww <= kCollapse * (cc + ww))
                code = S_COLLAPSE;
        }
        norm_sh = code == S_GO ? sqrt(ww) : 0.0;
        code_sh = code;
    }
    __syncthreads();
    const int code = __builtin_amdgcn_readfirstlane(code_sh);
    const double norm = norm_sh;
    if (blockIdx.x == 0 && code != S_BREAK) {
        int* flags = (int*)(tail + T_FLAGS);
        if (side == SIDE_LEFT && (int)threadIdx.x < cnt) tail[T_R + (size_t)j * kM + threadIdx.x] = c_sh[threadIdx.x];
        if (threadIdx.x == 0) {
            if (side == SIDE_LEFT)
                tail[T_R + (size_t)j * kM + j] = norm;
            else
                tail[T_GT + j + 1] = norm;
            if (j >= 0) flags[F_ITERS] += 1;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && code != S_GO)
        __atomic_store_n(&((int*)(tail + T_FLAGS))[F_STATUS], code == S_COLLAPSE ? ST_CONVERGED : ST_BREAKDOWN, __ATOMIC_RELAXED);
    if (code != S_GO) return;
    double* v = dst + (size_t)(side == SIDE_LEFT ? j : j + 1) * (size_t)ld_;
    const int stride = (int)gridDim.x * kThreads;
    for (int p = blockIdx.x * kThreads + threadIdx.x; 2 * (long long)p < n; p += stride) {
        const size_t i = 2 * (size_t)p;
        if (i + 1 < (size_t)n) {
            const double2 wv = load2(w + i);
            double2 vv;
            vv.x = wv.x / norm;
            vv.y = wv.y / norm;
            store2(v + i, vv);
        } else {
            v[i] = w[i] / norm;
        }
    }
}

// ------------------------------------------------------------------ the driver
struct Launcher {
    int grid, n;
    long long ld;
    hipStream_t st;
    double *w, *s, *tail;

    void dots(const double* basis, int cnt) const
    {
        hipLaunchKernelGGL(gmres_dots_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, basis, w, cnt, s, tail);
    }
    void update(const double* basis, int cnt, int pass, int last) const
    {
        hipLaunchKernelGGL(gmres_update_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, basis, w, cnt, s, tail, pass, last);
    }
    // classical Gram-Schmidt twice against `cnt` columns; without columns the norm alone
    void orthogonalise(const double* basis, int cnt) const
    {
        if (cnt == 0) return update(basis, 0, 0, 1);
        for (int p = 0; p < 2; ++p) {
            dots(basis, cnt);
            update(basis, cnt, p, p);
        }
    }
    void next(double* dst, int side, int j) const
    {
        hipLaunchKernelGGL(svds_next_kernel, dim3(grid), dim3(kThreads), 0, st, n, ld, dst, w, s, tail, side, j);
    }
};

struct Outputs {
    double *svals, *resid;
    int *found, *nconv, *multiplies, *restarts;
    void counts(int f, int c, int mu, int r) const
    {
        if (found) *found = f;
        if (nconv) *nconv = c;
        if (multiplies) *multiplies = mu;
        if (restarts) *restarts = r;
    }
};

int svds_solve(ehyb_plan* A, ehyb_plan* AT, const double* v0, int nsv, int m, int keep, int max_restarts, double tol, double* U, int64_t ldu,
               double* V, int64_t ldv, void* stream, const Outputs& out)
{
    const int n = A->host.n_cols;
    const size_t ld = (size_t)n + (n & 1);
    SolveLoop L(n, 0);
    double *w, *s;
    HIP_TRY(L.begin(stream, {&w}, ld, &s, G_COUNT, T_COUNT));
    DeviceArray P, Q, spare, Yp, Yq;
    HIP_TRY(hipMalloc((void**)&P.p, ld * (size_t)(m + 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&Q.p, ld * (size_t)m * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&spare.p, ld * (size_t)(keep + 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&Yp.p, (size_t)kCols * kM * sizeof(double)));
    HIP_TRY(hipMalloc((void**)&Yq.p, (size_t)kCols * kM * sizeof(double)));
    const hipStream_t st = L.st;
    double* tail = s + (size_t)G_COUNT * kMaxGrid;
    const Launcher K{L.grid, n, (long long)ld, st, w, s, tail};
    HIP_TRY(hipMemsetAsync(tail, 0, (size_t)T_COUNT * sizeof(double), st));

    // the start vector into w, its norm through the update kernel without columns, p_0 through next(right, -1)
    std::vector<double> start;
    if (v0) {
        HIP_TRY(hipMemcpyAsync(w, v0, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    } else {
        start.resize(n);
        for (int i = 0; i < n; ++i) start[i] = 1.0 + (double)(i % 7) * 0.125;
        HIP_TRY(hipMemcpyAsync(w, start.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    K.orthogonalise(P.p, 0);
    K.next(P.p, SIDE_RIGHT, -1);

    // steps j0 .. j1 - 1; the multiplies state their walk, A and A^T in opposite directions, alternating
    auto cycle = [&](int j0, int j1) -> int {
        for (int j = j0; j < j1; ++j) {
            const int fwd = j & 1 ? EHYB_WALK_LAST_TO_FIRST : EHYB_WALK_FIRST_TO_LAST, back = j & 1 ? EHYB_WALK_FIRST_TO_LAST : EHYB_WALK_LAST_TO_FIRST;
            int rc = ehyb_spmv_walk(A, P.p + (size_t)j * ld, w, st, fwd);
            if (rc != EHYB_OK) return rc;
            K.orthogonalise(Q.p, j);
            K.next(Q.p, SIDE_LEFT, j);
            if ((rc = multiply_t(A, AT, Q.p + (size_t)j * ld, w, n, 1, st, back)) != EHYB_OK) return rc;
            K.orthogonalise(P.p, j + 1);
            K.next(P.p, SIDE_RIGHT, j);
        }
        return EHYB_OK;
    };
    // one launch of ehyb_eigsh's rotation kernel: dst[:, c] = sum_{l < mc} Y[l, c] src[:, l] for c < kc
    auto rotate = [&](const double* src, int64_t ld_dst, double* dst, const double* Yhost, double* Ydev, int mc, int kc) -> int {
        HIP_TRY(hipMemcpyAsync(Ydev, Yhost, (size_t)mc * kc * sizeof(double), hipMemcpyHostToDevice, st));
        return ehyb_eigsh_rotate_step(n, (int64_t)ld, src, ld_dst, dst, Ydev, mc, kc, st);
    };

    CycleGraph G;  // the steady cycle keep .. m - 1, captured when it is first needed
    bool tried = A->cfg.graphs == 2;
    // B column-major with leading dimension kM; its transpose for ehyb_small_svd, whose X is then Y (on P) and whose Y is X (on Q)
    std::vector<double> th((size_t)T_COUNT), B((size_t)kM * kM, 0.0), Bt((size_t)kM * kM), sigma(kM), Yr((size_t)kM * kM), Xl((size_t)kM * kM),
        Yh((size_t)kCols * kM), Xh((size_t)kCols * kM), res(kM);
    int f[F_COUNT] = {ST_RUNNING, 0};
    int k = 0, restarts = 0, J = 0, Jl = 0, want = 0, nconv = 0;
    for (;;) {
        if (k == keep && k > 0 && keep < m && !tried) {
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
            EHYB_FAIL(EHYB_ERR_ARG, "ehyb_svds: breakdown after %d multiplies (a zero or non-finite start vector, or a non-finite coefficient "
                                    "or norm of the bidiagonalisation)",
                      f[F_ITERS]);
        }
        // made = 2 per full step; an odd count: the last left half collapsed
        const bool collapse = f[F_STATUS] == ST_CONVERGED;
        const int made = f[F_ITERS] - before;
        Jl = k + made / 2;
        J = Jl + (made & 1);
        for (int j = k; j < J; ++j)
            for (int i = 0; i <= j; ++i) B[(size_t)j * kM + i] = th[T_R + (size_t)j * kM + i];
        const double beta = collapse ? 0.0 : th[T_GT + J];
        if (Jl == 0) {  // a zero matrix: A p_0 = 0
            want = nconv = 0;
            break;
        }
        for (int c = 0; c < Jl; ++c)
            for (int r = 0; r < J; ++r) Bt[(size_t)c * J + r] = B[(size_t)r * kM + c];
        const int rc = ehyb_small_svd(J, Jl, Bt.data(), J, sigma.data(), Yr.data(), Xl.data());
        if (rc != EHYB_OK) return rc;
        want = std::min(nsv, Jl);
        for (int i = 0; i < Jl; ++i) res[i] = std::fabs(beta * Xl[(size_t)i * Jl + (Jl - 1)]);
        for (nconv = 0; nconv < want && res[nconv] <= tol * sigma[0];) ++nconv;
        if (nconv == want || collapse || restarts == max_restarts) break;

        // the restart (J = Jl = m): kk triplets and the old p_J; B = diag(sigma)
        const int kk = std::min(keep, J - 1), mc = J + 1;
        std::fill(Yh.begin(), Yh.begin() + (size_t)mc * (kk + 1), 0.0);
        for (int i = 0; i < kk; ++i) std::memcpy(&Yh[(size_t)i * mc], &Yr[(size_t)i * J], (size_t)J * sizeof(double));
        Yh[(size_t)kk * mc + J] = 1.0;
        int rrc = rotate(P.p, (int64_t)ld, spare.p, Yh.data(), Yp.p, mc, kk + 1);
        if (rrc != EHYB_OK) return rrc;
        HIP_TRY(hipMemcpyAsync(P.p, spare.p, ld * (size_t)(kk + 1) * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (kk > 0) {
            if ((rrc = rotate(Q.p, (int64_t)ld, spare.p, Xl.data(), Yq.p, Jl, kk)) != EHYB_OK) return rrc;
            HIP_TRY(hipMemcpyAsync(Q.p, spare.p, ld * (size_t)kk * sizeof(double), hipMemcpyDeviceToDevice, st));
        }
        std::fill(B.begin(), B.end(), 0.0);
        for (int i = 0; i < kk; ++i) B[(size_t)i * kM + i] = sigma[i];
        HIP_TRY(hipStreamSynchronize(st));  // the rotations are the host's again
        k = kk;
        ++restarts;
    }
    for (int i = 0; i < want; ++i) {
        if (out.svals) out.svals[i] = sigma[i];
        if (out.resid) out.resid[i] = res[i];
    }
    if (want > 0 && (U || V)) {
        int rc = EHYB_OK;
        if (U) rc = rotate(Q.p, ldu, U, Xl.data(), Yq.p, Jl, want);
        if (rc == EHYB_OK && V) rc = rotate(P.p, ldv, V, Yr.data(), Yp.p, J, want);
        if (rc != EHYB_OK) return rc;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    out.counts(want, nconv, f[F_ITERS], restarts);
    return EHYB_OK;
}

}  // namespace

extern "C" int ehyb_svds(ehyb_plan* P, ehyb_plan* PT, const double* v0, int nsv, int basis, int max_restarts, double tol, double* svals,
                         double* U, int64_t ldu, double* V, int64_t ldv, void* stream, int* found, int* nconv, int* multiplies, int* restarts,
                         double* resid)
{
    clear_error();
    if (!P) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_svds: null argument");
    if (nsv < 1 || nsv > EHYB_SVDS_MAX_NSV || (basis != 0 && (basis < nsv + 2 || basis > EHYB_SVDS_MAX_BASIS)) || max_restarts < 0)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_svds: nsv %d (1 .. %d), basis %d (0 or nsv + 2 .. %d), max_restarts %d", nsv, EHYB_SVDS_MAX_NSV, basis,
                  EHYB_SVDS_MAX_BASIS, max_restarts);
    if (!(tol >= 0)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_svds: tol %g", tol);
    int rc = pair_args("ehyb_svds", P, PT);
    if (rc != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    if ((U && (ldu < n || (ldu & 1))) || (V && (ldv < n || (ldv & 1))))
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_svds: ldu %lld, ldv %lld must be even and >= %d rows", (long long)ldu, (long long)ldv, n);
    if ((((uintptr_t)U | (uintptr_t)V | (uintptr_t)v0) & 15) != 0) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_svds: U_dev, V_dev and v0_dev must be 16-byte aligned");
    if ((rc = pair_uploaded("ehyb_svds", P, PT)) != EHYB_OK) return rc;
    const Outputs out{svals, resid, found, nconv, multiplies, restarts};
    if (n < 1) {
        out.counts(0, 0, 0, 0);
        return EHYB_OK;
    }
    int m = 0, keep = 0;
    ehyb_svds_basis(nsv, basis, n, &m, &keep);
    return svds_solve(P, PT, v0, nsv, m, keep, max_restarts, tol, U, ldu, V, ldv, stream, out);
}

// host only: the effective basis and the number of triplets a restart keeps -- the rule of ehyb_eigsh_basis, nsv for nev
extern "C" int ehyb_svds_basis(int nsv, int basis, int n, int* m_out, int* keep_out) { return ehyb_eigsh_basis(nsv, basis, n, m_out, keep_out); }

// ------------------------------------------------------------------ building block: one launch, slot_doubles / 2 workgroups
extern "C" int ehyb_svds_next_step(int n, int64_t ld_dst, double* dst, const double* w, double* s, int side, int j, void* stream)
{
    clear_error();
    int rc = check_step("ehyb_svds_next_step", n, {dst, w, s});
    if (rc != EHYB_OK) return rc;
    if ((side != SIDE_LEFT && side != SIDE_RIGHT) || j < (side == SIDE_RIGHT ? -1 : 0) || j >= kM)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_svds_next_step: bad arguments (side %d, 0 or 1; j %d, 0 .. %d, -1 with side 1)", side, j, kM - 1);
    if ((rc = check_pairs("ehyb_svds_next_step", n, ld_dst, {dst, w})) != EHYB_OK) return rc;
    hipLaunchKernelGGL(svds_next_kernel, dim3(kStepGrid), dim3(kThreads), 0, (hipStream_t)stream, n, (long long)ld_dst, dst, w, s, step_tail(s),
                       side, j);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
