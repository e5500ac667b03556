// Two-level PCG with an aggregate coarse space (ehyb_pcg_coarse, ehyb_pcg_coarse_multi, ehyb_coarse_apply): the CG loop of
// pcg_loop.h around z = M^-1 r = D^-1 r + P E^-1 P^T r, where P is piecewise constant over the aggregates of coarse.cpp and
// E^-1 = (P^T A P)^-1 is dense (nc <= EHYB_COARSE_MAX), inverted once on the host.  Three streaming kernels and no multiply:
//   restrict  T[u] = sum of r over the rows of unknown u        one wave per unknown, the rows through ROWS (the transposed map)
//   solve     C = E^-1 T                                        one wave per row of E^-1, T staged in LDS once per workgroup
//   prolong   z = D^-1 r + C[map], the partials of r.z          the walk of the Chebyshev kernels
// All three are templated on K columns per launch like the CG kernels (active flags, column offset c0; leading dimension n for
// the vectors, nc for T and C).  Every sum runs in a fixed order -- a lane's own terms in rising order, then the shuffle tree of
// vec_reduce.h -- with no atomics and no LDS adds, so a solve is the same bits from run to run.
// A vector object (P of local bases from near-null-space vectors, coarse.cpp) keeps the solve kernel and has a weighted
// restrict and a weighted prolong of its own, further down; launch_restrict and launch_prolong choose by the kind of the object.
//
// Loads.  E^-1 is re-read every iteration (8 nc^2 bytes, 33.5 MB at most) and wants to stay cached: plain loads.  r is read by
// restrict and again, one kernel later, by prolong, map and ROWS are read once per iteration but again in the next: plain loads
// too -- nothing here is dead after its read the way q is after the update kernel.
#include <hip/hip_runtime.h>

#include "coarse.h"
#include "pcg_loop.h"
#include "vec_walk.h"

using namespace ehyb;

namespace {

constexpr int kWaves = kThreads / 64;  // unknowns (restrict) or rows of E^-1 (solve) per workgroup

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// T[u] = sum over q in [row_ptr[u], row_ptr[u + 1]) of r[rows[q]]: lane l takes q = begin + l, + 64, ...; four index loads in
// flight per trip, added in the order of q.  K columns share the index loads.
template <int K>
__global__ __launch_bounds__(kThreads) void coarse_restrict_kernel(int n, int nc, const int32_t* __restrict__ row_ptr,
                                                                   const int32_t* __restrict__ rows, const double* __restrict__ R,
                                                                   double* __restrict__ T, const int* __restrict__ active, int c0)
{
    const int u = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (u >= nc) return;  // (a whole wave: no shuffle below misses a lane)
    bool on[K];
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        acc[c] = 0.0;
    }
    const int end = row_ptr[u + 1];
    int q = row_ptr[u] + (threadIdx.x & 63);
    for (; q + 192 < end; q += 256) {
        int idx[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) idx[t] = rows[q + 64 * t];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!on[c]) continue;
            const double* Rc = R + (size_t)(c0 + c) * n;
            double rv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) rv[t] = Rc[idx[t]];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[c] += rv[t];
        }
    }
    for (; q < end; q += 64) {
        const int i = rows[q];
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) acc[c] += R[(size_t)(c0 + c) * n + i];
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        if (!on[c]) continue;  // (uniform over the launch)
        const double t = wave_sum(acc[c]);
        if ((threadIdx.x & 63) == 0) T[(size_t)(c0 + c) * nc + u] = t;
    }
}

// C[u] = sum over d of Einv[u][d] T[d].  Einv has ld = nc rounded up to even doubles per row (the pad zero), so a row starts on
// 16 bytes: lane l reads the double2 at d = 2 l, + 128, ...  T of the live columns is staged in LDS (ld doubles per column, the
// pad zero) once per workgroup.  K columns share the row.  (A vector object's solve too: its T and C hold nc entries.)
template <int K>
__global__ __launch_bounds__(kThreads) void coarse_solve_kernel(int nc, int ld, const double* __restrict__ Einv, const double* __restrict__ T,
                                                                double* __restrict__ Cv, const int* __restrict__ active, int c0)
{
    extern __shared__ double Ts[];  // [K][ld]
    bool on[K];
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        acc[c] = 0.0;
        if (!on[c]) continue;
        for (int d = threadIdx.x; d < ld; d += kThreads) Ts[c * ld + d] = d < nc ? T[(size_t)(c0 + c) * nc + d] : 0.0;
    }
    __syncthreads();
    const int u = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (u >= nc) return;
    const double* row = Einv + (size_t)u * ld;
    for (int d = 2 * (threadIdx.x & 63); d < ld; d += 128) {
        const double2 e = *reinterpret_cast<const double2*>(row + d);
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!on[c]) continue;
            acc[c] = fma(e.x, Ts[c * ld + d], acc[c]);
            acc[c] = fma(e.y, Ts[c * ld + d + 1], acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        if (!on[c]) continue;
        const double t = wave_sum(acc[c]);
        if ((threadIdx.x & 63) == 0) Cv[(size_t)(c0 + c) * nc + u] = t;
    }
}

// z = dinv .* r + C[map] (dinv null: r + C[map]); rz >= 0: partials of r.z into r.z slot number rz.  The grid, the walk and the
// tail of cheb_multi_start_kernel.
template <int K>
__global__ __launch_bounds__(kThreads) void coarse_prolong_kernel(int n, int nc, const int32_t* __restrict__ map, const double* __restrict__ R,
                                                                  const double* __restrict__ dinv, const double* __restrict__ Cv,
                                                                  double* __restrict__ Z, double* __restrict__ s,
                                                                  const int* __restrict__ active, int c0, int rz)
{
    bool on[K];
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        acc[c] = 0.0;
    }
    struct Row {  // what the columns share at a row: 1/diag and the aggregate
        double dinv;
        int agg;
    };
    walk<K, kWalkU, 2>(
        n, on, [&](int i) { return Row{dinv ? dinv[i] : 1.0, map[i]}; },
        [&](int c, int i, double(&in)[2], Row row) {
            in[0] = R[(size_t)(c0 + c) * n + i];
            in[1] = Cv[(size_t)(c0 + c) * nc + row.agg];
        },
        [&](int c, int i, const double(&in)[2], Row row) {
            const double zi = dinv ? fma(in[0], row.dinv, in[1]) : in[0] + in[1];
            Z[(size_t)(c0 + c) * n + i] = zi;
            acc[c] = fma(in[0], zi, acc[c]);
        });
    if (rz < 0) return;  // (a kernel argument: the whole launch returns)
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<A_COUNT>(s, c0 + c, A_RZ0 + 2 * rz)[blockIdx.x] = acc[c];
    }
}

// ------------------------------------------------------------------ the vector object (ehyb_coarse_create_host_vecs)
// The two kernels beside restrict and prolong when P holds local bases: aggregate a owns the unknowns off[a] .. off[a + 1), one
// per kept column j, and W[j * n + i] is row i of column j.  NV bounds the columns at compile time (nv rounded up to 1, 2, 3, 4,
// 6 or 8), so the K * NV accumulators stay in registers; a column j >= kept is never touched -- neither its W nor its T or C.
//
// T[off[a] + j] = sum over q in [row_ptr[a], row_ptr[a + 1]) of W[j][rows[q]] r[rows[q]]: one wave per aggregate (workgroups of
// any whole number of waves), lane l takes q = begin + l, + 64, ... by fma in rising q, four index loads in flight per trip; then
// the shuffle tree.
template <int K, int NV>
__global__ __launch_bounds__(kThreads) void coarse_restrict_vec_kernel(int n, int nc, int nagg, const int32_t* __restrict__ row_ptr,
                                                                       const int32_t* __restrict__ rows, const int32_t* __restrict__ off,
                                                                       const double* __restrict__ W, const double* __restrict__ R,
                                                                       double* __restrict__ T, const int* __restrict__ active, int c0)
{
    const int a = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (a >= nagg) return;  // (a whole wave)
    const int o0 = off[a], kept = min(off[a + 1] - o0, NV);
    if (kept <= 0) return;
    bool on[K];
    double acc[K][NV];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
#pragma unroll
        for (int j = 0; j < NV; ++j) acc[c][j] = 0.0;
    }
    const int end = row_ptr[a + 1];
    int q = row_ptr[a] + (threadIdx.x & 63);
    for (; q + 192 < end; q += 256) {
        int idx[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) idx[t] = rows[q + 64 * t];
        // every load of the trip is issued before the first fma waits: a guard, not a break, so that the loads of column j + 1 do
        // not wait behind the sums of column j (an aggregate holds thousands of rows and only nagg waves run: latency is the cost)
        double rv[K][4], wv[NV][4];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!on[c]) continue;
#pragma unroll
            for (int t = 0; t < 4; ++t) rv[c][t] = R[(size_t)(c0 + c) * n + idx[t]];
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (j < kept) {  // (uniform over the wave)
#pragma unroll
                for (int t = 0; t < 4; ++t) wv[j][t] = W[(size_t)j * n + idx[t]];
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (j < kept) {
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    if (!on[c]) continue;
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[c][j] = fma(wv[j][t], rv[c][t], acc[c][j]);
                }
            }
        }
    }
    for (; q < end; q += 64) {
        const int i = rows[q];
        double rv[K];
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) rv[c] = R[(size_t)(c0 + c) * n + i];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (j >= kept) break;
            const double w = W[(size_t)j * n + i];
#pragma unroll
            for (int c = 0; c < K; ++c)
                if (on[c]) acc[c][j] = fma(w, rv[c], acc[c][j]);
        }
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        if (!on[c]) continue;  // (uniform over the launch)
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            if (j >= kept) break;
            const double t = wave_sum(acc[c][j]);
            if ((threadIdx.x & 63) == 0) T[(size_t)(c0 + c) * nc + o0 + j] = t;
        }
    }
}

// s = sum over the kept columns j of the row's aggregate of W[j][i] C[off[agg[i]] + j], by fma from 0 in rising j
template <int NV>
__device__ __forceinline__ double coarse_vec_term(const double (&w)[NV], const double* __restrict__ Cc, int o0, int kept)
{
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (j < kept) s = fma(w[j], Cc[o0 + j], s);
    return s;
}

// z = dinv .* r + s (dinv null: r + s), s as above; rz >= 0: partials of r.z into r.z slot number rz.  The grid, the walk and the
// tail of coarse_prolong_kernel; a row's W is loaded once for the K columns.  The loops are written out here: a trip goes stride
// by stride, one row of W in registers at a time, where the walk of vec_walk.h would load four rows before the first store.
template <int K, int NV>
__global__ __launch_bounds__(kThreads) void coarse_prolong_vec_kernel(int n, int nc, const int32_t* __restrict__ agg,
                                                                      const int32_t* __restrict__ off, const double* __restrict__ W,
                                                                      const double* __restrict__ R, const double* __restrict__ dinv,
                                                                      const double* __restrict__ Cv, double* __restrict__ Z,
                                                                      double* __restrict__ s, const int* __restrict__ active, int c0, int rz)
{
    bool on[K];
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        acc[c] = 0.0;
    }
    const int stride = (int)gridDim.x * kThreads;
    int i = blockIdx.x * kThreads + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        int au[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) au[u] = agg[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int iu = i + u * stride;
            const double dv = dinv ? dinv[iu] : 1.0;
            const int o0 = off[au[u]], kept = min(off[au[u] + 1] - o0, NV);
            double w[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (j < kept) w[j] = W[(size_t)j * n + iu];
#pragma unroll
            for (int c = 0; c < K; ++c) {
                if (!on[c]) continue;
                const size_t o = (size_t)(c0 + c) * n + iu;
                const double rv = R[o];
                const double cv = coarse_vec_term<NV>(w, Cv + (size_t)(c0 + c) * nc, o0, kept);
                const double zi = dinv ? fma(rv, dv, cv) : rv + cv;
                Z[o] = zi;
                acc[c] = fma(rv, zi, acc[c]);
            }
        }
    }
    for (; i < n; i += stride) {
        const double dvi = dinv ? dinv[i] : 1.0;
        const int ai = agg[i];
        const int o0 = off[ai], kept = min(off[ai + 1] - o0, NV);
        double w[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (j < kept) w[j] = W[(size_t)j * n + i];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            if (!on[c]) continue;
            const size_t o = (size_t)(c0 + c) * n + i;
            const double ri = R[o];
            const double ci = coarse_vec_term<NV>(w, Cv + (size_t)(c0 + c) * nc, o0, kept);
            const double zi = dinv ? fma(ri, dvi, ci) : ri + ci;
            Z[o] = zi;
            acc[c] = fma(ri, zi, acc[c]);
        }
    }
    if (rz < 0) return;  // (a kernel argument: the whole launch returns)
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<A_COUNT>(s, c0 + c, A_RZ0 + 2 * rz)[blockIdx.x] = acc[c];
    }
}

// f(integral_constant<NV>) with nv rounded up to an instantiated bound
template <typename F>
void with_vec_bound(int nv, F&& f)
{
    switch (nv) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5:
    case 6: f(std::integral_constant<int, 6>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
    }
}

inline int wave_grid(int nc) { return (nc + kWaves - 1) / kWaves; }
inline int vector_grid(int n) { return std::max(1, std::min((n + kThreads - 1) / kThreads, kMaxGrid / 2)); }

template <int K>
void launch_restrict(const ehyb_coarse* c, hipStream_t st, const double* R, double* T, const int* active, int c0)
{
    if (c->nv) {  // a vector object: one wave per aggregate, and one per workgroup -- a few hundred long sums, spread over every CU
        with_vec_bound(c->nv, [&](auto NV) {
            hipLaunchKernelGGL((coarse_restrict_vec_kernel<K, decltype(NV)::value>), dim3(c->nagg), dim3(64), 0, st, c->n, c->nc,
                               c->nagg, c->d_row_ptr, c->d_rows, c->d_off, c->d_w, R, T, active, c0);
        });
        return;
    }
    hipLaunchKernelGGL(coarse_restrict_kernel<K>, dim3(wave_grid(c->nc)), dim3(kThreads), 0, st, c->n, c->nc, c->d_row_ptr, c->d_rows, R, T,
                       active, c0);
}
template <int K>
void launch_solve(const ehyb_coarse* c, hipStream_t st, const double* T, double* Cv, const int* active, int c0)
{
    hipLaunchKernelGGL(coarse_solve_kernel<K>, dim3(wave_grid(c->nc)), dim3(kThreads), (size_t)K * c->ld * sizeof(double), st, c->nc, c->ld,
                       c->d_einv, T, Cv, active, c0);
}
template <int K>
void launch_prolong(const ehyb_coarse* c, int grid, hipStream_t st, const double* R, const double* dinv, const double* Cv, double* Z,
                    double* s, const int* active, int c0, int rz)
{
    if (c->nv) {
        with_vec_bound(c->nv, [&](auto NV) {
            hipLaunchKernelGGL((coarse_prolong_vec_kernel<K, decltype(NV)::value>), dim3(grid), dim3(kThreads), 0, st, c->n, c->nc, c->d_map,
                               c->d_off, c->d_w, R, dinv, Cv, Z, s, active, c0, rz);
        });
        return;
    }
    hipLaunchKernelGGL(coarse_prolong_kernel<K>, dim3(grid), dim3(kThreads), 0, st, c->n, c->nc, c->d_map, R, dinv, Cv, Z, s, active, c0, rz);
}

// in this order: what the plain solver rejects (done by the caller), the coarse object, then the two uploads
int coarse_args(const char* who, const ehyb_plan* P, const ehyb_coarse* c)
{
    if (!c) EHYB_FAIL(EHYB_ERR_ARG, "%s: null coarse object", who);
    if (c->n != P->host.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "%s: the coarse object has %d rows, the plan %d", who, c->n, P->host.n_cols);
    int rc = solve_uploaded(who, P);
    if (rc != EHYB_OK) return rc;
    if (!c->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: coarse object not uploaded", who);
    return EHYB_OK;
}

// The one driver: the loop of pcg_loop.h, one multiply per iteration (walks alternating), restrict -> solve -> prolong between
// update and direction.  The arguments are checked.
int coarse_solve(const char* who, ehyb_plan* P, ehyb_coarse* c, const double* dinv, const double* B, int64_t ldb, double* X, int64_t ldx,
                 int k, int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual)
{
    double *T, *Cv;
    auto precondition = [&](const PcgState& S, int, int rz) -> int {
        for_each_group(k, [&](auto K, int c0) {
            constexpr int W = decltype(K)::value;
            launch_restrict<W>(c, S.st, S.R, T, S.active, c0);
            launch_solve<W>(c, S.st, T, Cv, S.active, c0);
            launch_prolong<W>(c, S.grid, S.st, S.R, dinv, Cv, S.Z, S.s, S.active, c0, rz);
        });
        return EHYB_OK;
    };
    return pcg_solve(
        who, "is the matrix symmetric positive definite?", P, B, ldb, X, ldx, k, max_iter, rtol, check_every, stream, iters_done, rel_residual,
        {{&T, (size_t)c->nc * k}, {&Cv, (size_t)c->nc * k}}, [](const PcgState&) { return EHYB_OK; }, [](int it) { return walk_of(it); },
        precondition);
}

template <typename T>
hipError_t to_device(T** d, const T* h, size_t count)
{
    hipError_t e = hipMalloc((void**)d, std::max<size_t>(1, count) * sizeof(T));
    if (e == hipSuccess && count) e = hipMemcpy(*d, h, count * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

void release_device(ehyb_coarse* c)
{
    for (void* p : {(void*)c->d_map, (void*)c->d_row_ptr, (void*)c->d_rows, (void*)c->d_off, (void*)c->d_w, (void*)c->d_einv, (void*)c->d_scratch})
        if (p) (void)hipFree(p);
    c->d_map = c->d_row_ptr = c->d_rows = c->d_off = nullptr;
    c->d_w = c->d_einv = c->d_scratch = nullptr;
    c->uploaded = false;
}

}  // namespace

extern "C" int ehyb_coarse_upload(ehyb_coarse* c)
{
    clear_error();
    if (!c) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_coarse_upload: null argument");
    if (c->uploaded) return EHYB_OK;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) {
        (void)hipGetLastError();
        EHYB_FAIL(EHYB_ERR_NO_DEVICE, "ehyb_coarse_upload: no HIP device visible (no CPU fallback exists)");
    }
    // E^-1 with rows of ld doubles, the pad column zero
    std::vector<double> padded((size_t)c->nc * c->ld, 0.0);
    for (int u = 0; u < c->nc; ++u) std::copy(&c->Einv[(size_t)u * c->nc], &c->Einv[(size_t)(u + 1) * c->nc], &padded[(size_t)u * c->ld]);
    hipError_t e = to_device(&c->d_map, c->map.data(), c->map.size());
    if (e == hipSuccess) e = to_device(&c->d_row_ptr, c->row_ptr.data(), c->row_ptr.size());
    if (e == hipSuccess) e = to_device(&c->d_rows, c->rows.data(), c->rows.size());
    if (e == hipSuccess && c->nv) e = to_device(&c->d_off, c->off.data(), c->off.size());
    if (e == hipSuccess && c->nv) e = to_device(&c->d_w, c->W.data(), c->W.size());
    if (e == hipSuccess) e = to_device(&c->d_einv, padded.data(), padded.size());
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_scratch, (size_t)2 * c->nc * sizeof(double));
    if (e != hipSuccess) {
        release_device(c);
        EHYB_FAIL(EHYB_ERR_HIP, "ehyb_coarse_upload: %s", hipGetErrorString(e));
    }
    c->uploaded = true;
    return EHYB_OK;
}

extern "C" void ehyb_coarse_destroy(ehyb_coarse* c)
{
    if (!c) return;
    if (c->uploaded) release_device(c);
    delete c;
}

extern "C" int ehyb_coarse_apply(ehyb_coarse* c, const double* dinv, const double* r, double* z, void* stream)
{
    clear_error();
    if (!c || !r || !z) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_coarse_apply: null argument");
    if (!c->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_coarse_apply: coarse object not uploaded");
    const hipStream_t st = (hipStream_t)stream;
    double *T = c->d_scratch, *Cv = c->d_scratch + c->nc;
    launch_restrict<1>(c, st, r, T, nullptr, 0);
    launch_solve<1>(c, st, T, Cv, nullptr, 0);
    launch_prolong<1>(c, vector_grid(c->n), st, r, dinv, Cv, z, nullptr, nullptr, 0, -1);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_pcg_coarse(ehyb_plan* P, ehyb_coarse* c, const double* dinv, const double* b, double* x, int max_iter, double rtol,
                               int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const char* who = "ehyb_pcg_coarse";
    int rc = solve_args(who, P, b && x, max_iter, rtol);
    if (rc != EHYB_OK || (rc = coarse_args(who, P, c)) != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    return coarse_solve(who, P, c, dinv, b, n, x, n, 1, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

extern "C" int ehyb_pcg_coarse_multi(ehyb_plan* P, ehyb_coarse* c, const double* dinv, const double* B, int64_t ldb, double* X, int64_t ldx,
                                     int k, int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const char* who = "ehyb_pcg_coarse_multi";
    int rc = multi_args(who, P, ldb, ldx, k);
    if (rc == EHYB_OK) rc = solve_args(who, P, B && X, max_iter, rtol);
    if (rc != EHYB_OK || (rc = coarse_args(who, P, c)) != EHYB_OK) return rc;
    return coarse_solve(who, P, c, dinv, B, ldb, X, ldx, k, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

// ------------------------------------------------------------------ the three kernels one at a time (as ehyb_cheb_*_step)
extern "C" int ehyb_coarse_restrict_step(ehyb_coarse* c, const double* r, double* t, void* stream)
{
    clear_error();
    if (!c || !r || !t) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_coarse_restrict_step: null argument");
    if (!c->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_coarse_restrict_step: coarse object not uploaded");
    launch_restrict<1>(c, (hipStream_t)stream, r, t, nullptr, 0);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_coarse_solve_step(ehyb_coarse* c, const double* t, double* cv, void* stream)
{
    clear_error();
    if (!c || !t || !cv) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_coarse_solve_step: null argument");
    if (!c->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_coarse_solve_step: coarse object not uploaded");
    launch_solve<1>(c, (hipStream_t)stream, t, cv, nullptr, 0);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

extern "C" int ehyb_coarse_prolong_step(ehyb_coarse* c, const double* r, const double* dinv, const double* cv, double* z, double* s, int rz,
                                        void* stream)
{
    clear_error();
    if (!c || !r || !cv || !z || rz < -1 || rz > 1 || (rz >= 0 && !s)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_coarse_prolong_step: bad arguments");
    if (!c->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_coarse_prolong_step: coarse object not uploaded");
    launch_prolong<1>(c, kMaxGrid / 2, (hipStream_t)stream, r, dinv, cv, z, s, nullptr, 0, rz);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
