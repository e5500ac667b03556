// PCG with a factorised sparse approximate inverse (ehyb_pcg_fsai, ehyb_pcg_fsai_multi, ehyb_fsai_apply, ehyb_fsai_set_values):
// the CG loop of pcg_loop.h around z = M^-1 r = G^T (G r), G lower triangular on the pattern of tril(A) (fsai.cpp).  Both
// products are multiplies on G's own plans (ehyb_spmm; or ehyb_spmv_t on the plan of G for the second), so the only kernels here
// are
//   factor    row i of G from the dense block A[J_i, J_i]        one wave per row, the block's lower triangle in that wave's LDS
//   tt        the partials of t.t = r.z, t = G r                 the walk of the other vector kernels
//
// The factor kernel (the numeric phase of the build, repeated on the device for new values of A).  A wave owns one row i of G:
//   pattern   J = the row's m <= cap columns, rising, the diagonal last: lane l puts J[l], the first entry of row J[l] of A and
//             the number of entries of the rows before it (a prefix sum over the lanes) into the wave's three LDS lists
//   assemble  the entries of the rows J[0], J[1], ... of A are walked as one run, 256 a trip: a lane finds the row k of each of
//             its four entries in the prefix list, loads the four columns (and entry-order values) together, and stores an entry
//             whose column is J[c], c <= k (a binary search in the list), at S[k (k + 1) / 2 + c].  What is not stored stays
//             0.  Only the lower triangle of A is read: the matrix is taken to be symmetric.
//   factor    S = L L^T right-looking: per column j the pivot's root, lane r scales L[r][j], stores it and keeps it in a
//             register, then for r = j + 1 .. m - 1, four rows a trip, lane c, j < c <= r, takes L[r][j] L[c][j] off S[r][c] --
//             L[r][j] one LDS word for all lanes, S[r][c] at consecutive LDS words
//   solve     L^T g = e_m from the last unknown up: lane r carries its right-hand side, unknown c is divided out by lane c and
//             handed round by a shuffle, lanes r < c take L[c][r] g[c] off (row c of L: consecutive LDS words)
//   store     g in CSR order; a pivot that is not a positive finite number: the Jacobi form of the row, counted
// LDS per workgroup of kFactorWaves waves: per wave cap (cap + 1) / 2 doubles (rounded up to even) and, behind all of them, three
// lists of cap ints (rounded up to four) -- 69,632 bytes at cap = 64, so the kernel opts in to the large LDS like the window
// kernels.  cap is the longest row the pattern HAS, which is what the LDS is sized from.  A wave never waits for another: no
// barrier, no flag, no atomics but the four counters; the data it shares are its own lanes' (wave_sync orders the LDS traffic
// for the compiler, the hardware keeps a wave's LDS operations in order).  Every index that comes from an array -- a row pointer,
// a column, an entry-order value -- is held against the length of the array it goes into before it is used.
#include <hip/hip_runtime.h>

#include "fsai.h"
#include "pcg_loop.h"
#include "vec_walk.h"

using namespace ehyb;

namespace {

constexpr int kFactorWaves = 4;
constexpr int kFactorThreads = 64 * kFactorWaves;
enum { C_FALLBACK = 0, C_BAD_DIAG = 1, C_BAD_ORDER = 2, C_BAD_PATTERN = 3, C_COUNT = 4 };

inline int tri_doubles(int cap) { return (cap * (cap + 1) / 2 + 1) & ~1; }
inline int list_ints(int cap) { return (cap + 3) & ~3; }
inline size_t factor_lds(int cap) { return (size_t)kFactorWaves * ((size_t)tri_doubles(cap) * 8 + (size_t)3 * list_ints(cap) * 4); }

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool positive_finite(double v) { return v > 0 && v <= 1.7976931348623157e308; }

__global__ __launch_bounds__(kFactorThreads) void ehyb_fsai_factor_kernel(int n, int cap, int tri_cap, int list_cap, const int32_t* __restrict__ a_ptr,
                                                                          const int32_t* __restrict__ a_cols, long long nnz_a,
                                                                          const double* __restrict__ values, const int32_t* __restrict__ order,
                                                                          long long count, const int64_t* __restrict__ g_ptr,
                                                                          const int32_t* __restrict__ g_cols, long long nnz_g,
                                                                          double* __restrict__ g_vals, int* __restrict__ counters)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = blockIdx.x * kFactorWaves + w;
    if (i >= n) return;  // (a whole wave: no shuffle below misses a lane)
    double* S = reinterpret_cast<double*>(smem) + (size_t)w * tri_cap;
    int32_t* Js = reinterpret_cast<int32_t*>(smem + (size_t)kFactorWaves * tri_cap * 8) + (size_t)w * 3 * list_cap;
    int32_t* Rb = Js + list_cap;       // first entry of row J[k] of A
    int32_t* Pre = Js + 2 * list_cap;  // entries of the rows J[0 .. k - 1] of A
    const long long gb = g_ptr[i], ge = g_ptr[i + 1];
    if (gb < 0 || ge > nnz_g || ge - gb < 1 || ge - gb > cap) {  // (uniform over the wave) nothing of this row is written
        if (lane == 0) atomicAdd(&counters[C_BAD_PATTERN], 1);
        return;
    }
    const int m = (int)(ge - gb);
    const int tri_m = m * (m + 1) / 2;
    // lane l: column J[l] and the stretch of A's entries that is row J[l], cut down to the arrays; a row outside them is empty
    int my_col = -1, rb = 0, len = 0;
    if (lane < m) {
        my_col = g_cols[gb + lane];
        if ((unsigned)my_col < (unsigned)n) {
            long long b0 = a_ptr[my_col], e0 = a_ptr[my_col + 1];
            if (b0 < 0) b0 = 0;
            if (e0 > nnz_a) e0 = nnz_a;
            if (order && e0 > count) e0 = count;  // (order holds count values)
            if (e0 - b0 > (1 << 24)) e0 = b0 + (1 << 24);  // (so that 64 lengths add up in an int)
            if (e0 > b0) rb = (int)b0, len = (int)(e0 - b0);
        }
    }
    int upto = len;  // inclusive prefix sum over the lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int below = __shfl_up(upto, off, 64);
        if (lane >= off) upto += below;
    }
    const int total = __shfl(upto, 63, 64);
    if (lane < m) Js[lane] = my_col, Rb[lane] = rb, Pre[lane] = upto - len;
    for (int t = lane; t < tri_m; t += 64) S[t] = 0.0;
    wave_sync();

    // ---- assemble: the entries of the rows J[0], J[1], ... of A in one run, 256 a trip -- four per lane, their loads in flight
    // together.  Entry number t belongs to the last row k with Pre[k] <= t; it lands in row k of S where its column is one of
    // J[0 .. k].  (Row i walks all of row i of A for its last row of S: every entry_order value is looked at by some wave.)
    int bad_order = 0;
    // (the loads of the next trip are issued before this trip's entries are matched: two trips in flight)
    // Both searches take six steps whatever they find, the four entries of a lane side by side: four LDS reads in flight per step.
    auto fetch = [&](int t0, int (&kk)[4], int (&col)[4], long long (&src)[4]) {
        int k[4] = {0, 0, 0, 0};
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = k[u] + step;
                if (c < m && Pre[c] <= t0 + 64 * u + lane) k[u] = c;  // the last row that starts at or before the entry
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + 64 * u + lane;
            kk[u] = -1;
            if (t >= total) continue;
            const long long e = (long long)Rb[k[u]] + (t - Pre[k[u]]);
            kk[u] = k[u];
            col[u] = a_cols[e];
            src[u] = order ? (long long)order[e] : e;
        }
    };
    int kk[4], col[4], kk_next[4], col_next[4];
    long long src[4], src_next[4];
    fetch(0, kk, col, src);
    for (int t0 = 0; t0 < total; t0 += 256) {
        fetch(t0 + 256, kk_next, col_next, src_next);
        int at[4] = {0, 0, 0, 0};
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = at[u] + step;
                if (c <= kk[u] && Js[c] <= col[u]) at[u] = c;  // the last of J[0 .. k] at or below the column
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = kk[u];
            if (k >= 0 && (src[u] < 0 || src[u] >= count)) bad_order = 1;
            if (k >= 0 && src[u] >= 0 && src[u] < count && Js[at[u]] == col[u]) S[k * (k + 1) / 2 + at[u]] = values[src[u]];
            kk[u] = kk_next[u], col[u] = col_next[u], src[u] = src_next[u];
        }
    }
    if (bad_order) atomicAdd(&counters[C_BAD_ORDER], 1);
    wave_sync();

    const double aii = S[tri_m - 1];
    if (!positive_finite(aii)) {  // (uniform) the caller fails: "not positive definite"
        if (lane == 0) atomicAdd(&counters[C_BAD_DIAG], 1);
        if (lane < m) g_vals[gb + lane] = 0.0;
        return;
    }

    // ---- S = L L^T
    const int my = lane * (lane + 1) / 2;  // where row `lane` of S starts
    bool ok = true;
    for (int j = 0; j < m; ++j) {
        const double d = S[j * (j + 1) / 2 + j];
        if (!positive_finite(d)) {  // (uniform)
            ok = false;
            break;
        }
        const double ljj = sqrt(d);
        double lj = 0.0;  // L[lane][j]
        if (lane > j && lane < m) {
            lj = S[my + j] / ljj;
            S[my + j] = lj;
        }
        if (lane == j) S[my + j] = ljj;
        wave_sync();  // column j of L is in LDS
        for (int r = j + 1; r < m; r += 4) {  // four rows a trip: their eight loads, then their four stores
            double l[4], v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = (r + u) * (r + u + 1) / 2;
                l[u] = v[u] = 0.0;
                if (r + u < m && lane > j && lane <= r + u) l[u] = S[row + j], v[u] = S[row + lane];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r + u < m && lane > j && lane <= r + u) S[(r + u) * (r + u + 1) / 2 + lane] = v[u] - l[u] * lj;
        }
        wave_sync();
    }

    double g = 0.0;
    if (ok) {
        // ---- L^T g = e_m
        const double dl = lane < m ? S[my + lane] : 1.0;
        double acc = lane == m - 1 ? 1.0 : 0.0;
        for (int c = m - 1; c >= 0; --c) {
            double q = 0.0;
            if (lane == c) q = acc / dl;
            const double gc = __shfl(q, c, 64);
            if (lane == c) g = gc;
            if (lane < c) acc = acc - S[c * (c + 1) / 2 + lane] * gc;
        }
    } else {
        if (lane == 0) atomicAdd(&counters[C_FALLBACK], 1);
        if (lane == m - 1) g = 1.0 / sqrt(aii);
    }
    if (lane < m) g_vals[gb + lane] = g;
}

// the partials of t.t into r.z slot number rz: the grid, the walk and the tail of coarse_prolong_kernel
template <int K>
__global__ __launch_bounds__(kThreads) void fsai_tt_kernel(int n, const double* __restrict__ T, double* __restrict__ s, const int* __restrict__ active,
                                                           int c0, int rz)
{
    bool on[K];
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        acc[c] = 0.0;
    }
    walk<K, kWalkU, 1>(
        n, on, NoShared{}, [&](int c, int i, double(&in)[1], int) { in[0] = T[(size_t)(c0 + c) * n + i]; },
        [&](int c, int, const double(&in)[1], int) { acc[c] = fma(in[0], in[0], acc[c]); });
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<A_COUNT>(s, c0 + c, A_RZ0 + 2 * rz)[blockIdx.x] = acc[c];
    }
}

template <int K>
void launch_tt(int n, int grid, hipStream_t st, const double* T, double* s, const int* active, int c0, int rz)
{
    hipLaunchKernelGGL(fsai_tt_kernel<K>, dim3(grid), dim3(kThreads), 0, st, n, T, s, active, c0, rz);
}

// The factor launch: cap = the longest row of the pattern (1 .. EHYB_FSAI_MAX_ROW, checked by the caller); counters zeroed by the caller
hipError_t launch_factor(int n, int cap, const int32_t* a_ptr, const int32_t* a_cols, long long nnz_a, const double* values, const int32_t* order,
                         long long count, const int64_t* g_ptr, const int32_t* g_cols, long long nnz_g, double* g_vals, int* counters,
                         hipStream_t st)
{
    if (n < 1) return hipSuccess;
    const size_t lds = factor_lds(cap);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ehyb_fsai_factor_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)factor_lds(EHYB_FSAI_MAX_ROW));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ehyb_fsai_factor_kernel, dim3((n + kFactorWaves - 1) / kFactorWaves), dim3(kFactorThreads), lds, st, n, cap, tri_doubles(cap),
                       list_ints(cap), a_ptr, a_cols, nnz_a, values, order, count, g_ptr, g_cols, nnz_g, g_vals, counters);
    return hipGetLastError();
}

// what the counters say once the stream has drained; fallback: where the count of fallback rows goes
int read_counters(const char* who, const int* d_counters, hipStream_t st, int64_t* fallback)
{
    int c[C_COUNT];
    HIP_TRY(hipMemcpyAsync(c, d_counters, sizeof c, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c[C_BAD_PATTERN]) EHYB_FAIL(EHYB_ERR_ARG, "%s: %d rows of the pattern are empty, longer than the cap or outside the arrays", who, c[C_BAD_PATTERN]);
    if (c[C_BAD_ORDER]) EHYB_FAIL(EHYB_ERR_ARG, "%s: entry_order values outside [0, count) (seen by %d lanes)", who, c[C_BAD_ORDER]);
    if (c[C_BAD_DIAG])
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the matrix is not positive definite (%d diagonal entries are missing or not positive finite numbers)", who,
                  c[C_BAD_DIAG]);
    *fallback = c[C_FALLBACK];
    return EHYB_OK;
}

template <typename T>
hipError_t to_device(T** d, const T* h, size_t count)
{
    hipError_t e = hipMalloc((void**)d, std::max<size_t>(1, count) * sizeof(T));
    if (e == hipSuccess && count) e = hipMemcpy(*d, h, count * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

void release_device(ehyb_fsai* f)
{
    for (void* p : {(void*)f->d_a_ptr, (void*)f->d_a_cols, (void*)f->d_row_ptr, (void*)f->d_cols, (void*)f->d_order_t, (void*)f->d_vals, (void*)f->d_t,
                    (void*)f->d_count})
        if (p) (void)hipFree(p);
    f->d_a_ptr = f->d_a_cols = f->d_cols = f->d_order_t = nullptr;
    f->d_row_ptr = nullptr;
    f->d_vals = f->d_t = nullptr;
    f->d_count = nullptr;
    f->uploaded = false;
}

// what owns the temporaries of a call
struct Temp {
    std::vector<void*> bufs;
    ~Temp()
    {
        for (void* p : bufs) (void)hipFree(p);
    }
    template <typename T>
    hipError_t put(T** d, const T* h, size_t count)
    {
        const hipError_t e = to_device(d, h, count);
        if (*d) bufs.push_back(*d);
        return e;
    }
};

// in this order: what the plain solver rejects (done by the caller), the object, then the uploads
int fsai_args(const char* who, const ehyb_plan* P, const ehyb_fsai* f)
{
    if (!f) EHYB_FAIL(EHYB_ERR_ARG, "%s: null fsai object", who);
    if (f->n != P->host.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "%s: the fsai object has %d rows, the plan %d", who, f->n, P->host.n_cols);
    int rc = solve_uploaded(who, P);
    if (rc != EHYB_OK) return rc;
    if (!f->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: fsai object not uploaded", who);
    return EHYB_OK;
}

// Z = G^T (G R) for k columns of leading dimension n, T the k columns in between; the partials of t.t where s is given
int apply_columns(ehyb_fsai* f, int k, int grid, hipStream_t st, const double* R, double* T, double* Z, double* s, const int* active, int rz, int it)
{
    const int n = f->n;
    int rc;
    if (f->transpose_mode == 0) {
        if ((rc = ehyb_spmm(f->plan_g, R, n, T, n, k, st, walk_of(it))) != EHYB_OK) return rc;
    } else {
        for (int j = 0; j < k; ++j)
            if ((rc = ehyb_spmv_walk(f->plan_g, R + (size_t)j * n, T + (size_t)j * n, st, walk_of(it))) != EHYB_OK) return rc;
    }
    if (s) for_each_group(k, [&](auto K, int c0) { launch_tt<decltype(K)::value>(n, grid, st, T, s, active, c0, rz); });
    if (f->transpose_mode == 0) return ehyb_spmm(f->plan_t, T, n, Z, n, k, st, walk_of(it + 1));
    for (int j = 0; j < k; ++j)
        if ((rc = ehyb_spmv_t(f->plan_g, T + (size_t)j * n, Z + (size_t)j * n, st)) != EHYB_OK) return rc;
    return EHYB_OK;
}

// The one driver: the loop of pcg_loop.h, one multiply with A per iteration (walks alternating), G and G^T between update and
// direction.  The arguments are checked.
int fsai_solve(const char* who, ehyb_plan* P, ehyb_fsai* f, const double* B, int64_t ldb, double* X, int64_t ldx, int k, int max_iter, double rtol,
               int check_every, void* stream, int* iters_done, double* rel_residual)
{
    double* T;
    auto precondition = [&](const PcgState& S, int it, int rz) -> int { return apply_columns(f, k, S.grid, S.st, S.R, T, S.Z, S.s, S.active, rz, it); };
    return pcg_solve(
        who, "is the matrix symmetric positive definite?", P, B, ldb, X, ldx, k, max_iter, rtol, check_every, stream, iters_done, rel_residual,
        {{&T, (size_t)f->n * k}}, [](const PcgState&) { return EHYB_OK; }, [](int it) { return walk_of(it); }, precondition);
}

}  // namespace

extern "C" int ehyb_fsai_upload(ehyb_fsai* f)
{
    clear_error();
    if (!f) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_fsai_upload: null argument");
    if (f->uploaded) return EHYB_OK;
    int rc = ehyb_plan_upload(f->plan_g);
    if (rc == EHYB_OK && f->plan_t) rc = ehyb_plan_upload(f->plan_t);
    if (rc != EHYB_OK) return rc;
    hipError_t e = to_device(&f->d_a_ptr, f->a_ptr.data(), f->a_ptr.size());
    if (e == hipSuccess) e = to_device(&f->d_a_cols, f->a_cols.data(), f->a_cols.size());
    if (e == hipSuccess) e = to_device(&f->d_row_ptr, f->row_ptr.data(), f->row_ptr.size());
    if (e == hipSuccess) e = to_device(&f->d_cols, f->cols.data(), f->cols.size());
    if (e == hipSuccess && f->plan_t) e = to_device(&f->d_order_t, f->order_t.data(), f->order_t.size());
    if (e == hipSuccess) e = to_device(&f->d_vals, f->vals.data(), f->vals.size());
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_t, std::max<size_t>(1, (size_t)f->n) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&f->d_count, C_COUNT * sizeof(int));
    if (e != hipSuccess) {
        release_device(f);
        EHYB_FAIL(EHYB_ERR_HIP, "ehyb_fsai_upload: %s", hipGetErrorString(e));
    }
    f->uploaded = true;
    return EHYB_OK;
}

extern "C" void ehyb_fsai_destroy(ehyb_fsai* f)
{
    if (!f) return;
    if (f->uploaded) release_device(f);
    if (f->plan_g) ehyb_plan_destroy(f->plan_g);
    if (f->plan_t) ehyb_plan_destroy(f->plan_t);
    delete f;
}

extern "C" int ehyb_fsai_set_values(ehyb_fsai* f, const double* values, int64_t count, const int32_t* entry_order, int on_device, void* stream)
{
    const char* who = "ehyb_fsai_set_values";
    clear_error();
    if (!f || !values) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    if (!f->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: fsai object not uploaded (the numeric phase runs on the device)", who);
    const long long nnz_a = (long long)f->a_cols.size(), nnz_g = (long long)f->cols.size();
    if (count != nnz_a) EHYB_FAIL(EHYB_ERR_ARG, "%s: %lld values for a matrix of %lld entries", who, (long long)count, nnz_a);
    const hipStream_t st = (hipStream_t)stream;
    Temp tmp;
    const double* dV = values;
    const int32_t* dOrder = entry_order;
    if (!on_device) {
        double* v = nullptr;
        HIP_TRY(tmp.put(&v, values, (size_t)count));
        dV = v;
        if (entry_order) {
            int32_t* o = nullptr;
            HIP_TRY(tmp.put(&o, entry_order, (size_t)count));
            dOrder = o;
        }
    }
    // ---- nothing of the plans is written before the counters have been read
    HIP_TRY(hipMemsetAsync(f->d_count, 0, C_COUNT * sizeof(int), st));
    HIP_TRY(launch_factor(f->n, f->max_row, f->d_a_ptr, f->d_a_cols, nnz_a, dV, dOrder, count, f->d_row_ptr, f->d_cols, nnz_g, f->d_vals, f->d_count, st));
    int64_t fallback = 0;
    int rc = read_counters(who, f->d_count, st, &fallback);
    if (rc != EHYB_OK) return rc;
    if ((rc = ehyb_plan_set_values(f->plan_g, f->d_vals, nnz_g, nullptr, 1, st)) != EHYB_OK) return rc;
    if (f->plan_t && (rc = ehyb_plan_set_values(f->plan_t, f->d_vals, nnz_g, f->d_order_t, 1, st)) != EHYB_OK) return rc;
    f->counts[1] = fallback;
    if (!on_device) HIP_TRY(hipStreamSynchronize(st));  // the temporaries go away with this call
    return EHYB_OK;
}

extern "C" int ehyb_fsai_apply(ehyb_fsai* f, const double* r, double* z, void* stream)
{
    clear_error();
    if (!f || !r || !z) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_fsai_apply: null argument");
    if (!f->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_fsai_apply: fsai object not uploaded");
    return apply_columns(f, 1, 0, (hipStream_t)stream, r, f->d_t, z, nullptr, nullptr, -1, 0);
}

extern "C" int ehyb_pcg_fsai(ehyb_plan* P, ehyb_fsai* f, const double* b, double* x, int max_iter, double rtol, int check_every, void* stream,
                             int* iters_done, double* rel_residual)
{
    const char* who = "ehyb_pcg_fsai";
    int rc = solve_args(who, P, b && x, max_iter, rtol);
    if (rc != EHYB_OK || (rc = fsai_args(who, P, f)) != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    return fsai_solve(who, P, f, b, n, x, n, 1, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

extern "C" int ehyb_pcg_fsai_multi(ehyb_plan* P, ehyb_fsai* f, const double* B, int64_t ldb, double* X, int64_t ldx, int k, int max_iter, double rtol,
                                   int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const char* who = "ehyb_pcg_fsai_multi";
    int rc = multi_args(who, P, ldb, ldx, k);
    if (rc == EHYB_OK) rc = solve_args(who, P, B && X, max_iter, rtol);
    if (rc != EHYB_OK || (rc = fsai_args(who, P, f)) != EHYB_OK) return rc;
    return fsai_solve(who, P, f, B, ldb, X, ldx, k, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

// ------------------------------------------------------------------ the two kernels one launch at a time
extern "C" int ehyb_fsai_factor_step(int n, const int32_t* a_ptr, const int32_t* a_cols, const double* a_vals, const int64_t* g_ptr,
                                     const int32_t* g_cols, double* g_out, int* fallback_rows, void* stream)
{
    const char* who = "ehyb_fsai_factor_step";
    clear_error();
    if (n < 1 || !a_ptr || !a_cols || !a_vals || !g_ptr || !g_cols || !g_out) EHYB_FAIL(EHYB_ERR_ARG, "%s: bad arguments", who);
    if (a_ptr[0] != 0 || g_ptr[0] != 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: a row pointer does not start at 0", who);
    int cap = 1;
    for (int i = 0; i < n; ++i) {
        const int64_t len = g_ptr[i + 1] - g_ptr[i];
        if (a_ptr[i + 1] < a_ptr[i] || len < 1 || len > EHYB_FSAI_MAX_ROW)
            EHYB_FAIL(EHYB_ERR_ARG, "%s: row %d: %d entries of A, %lld of the pattern (1 .. %d)", who, i, a_ptr[i + 1] - a_ptr[i], (long long)len,
                      EHYB_FSAI_MAX_ROW);
        cap = std::max(cap, (int)len);
    }
    const long long nnz_a = a_ptr[n], nnz_g = g_ptr[n];
    const hipStream_t st = (hipStream_t)stream;
    Temp tmp;
    int32_t *d_ap = nullptr, *d_ac = nullptr, *d_gc = nullptr;
    int64_t* d_gp = nullptr;
    double *d_av = nullptr, *d_g = nullptr;
    int* d_count = nullptr;
    const int zero[C_COUNT] = {0, 0, 0, 0};
    std::vector<double> nan_fill((size_t)nnz_g, NAN);  // a row the kernel does not write shows
    HIP_TRY(tmp.put(&d_ap, a_ptr, (size_t)n + 1));
    HIP_TRY(tmp.put(&d_ac, a_cols, (size_t)nnz_a));
    HIP_TRY(tmp.put(&d_av, a_vals, (size_t)nnz_a));
    HIP_TRY(tmp.put(&d_gp, g_ptr, (size_t)n + 1));
    HIP_TRY(tmp.put(&d_gc, g_cols, (size_t)nnz_g));
    HIP_TRY(tmp.put(&d_g, nan_fill.data(), (size_t)nnz_g));
    HIP_TRY(tmp.put(&d_count, zero, (size_t)C_COUNT));
    HIP_TRY(launch_factor(n, cap, d_ap, d_ac, nnz_a, d_av, nullptr, nnz_a, d_gp, d_gc, nnz_g, d_g, d_count, st));
    int64_t fallback = 0;
    const int rc = read_counters(who, d_count, st, &fallback);
    if (rc != EHYB_OK) return rc;
    HIP_TRY(hipMemcpy(g_out, d_g, (size_t)nnz_g * sizeof(double), hipMemcpyDeviceToHost));
    if (fallback_rows) *fallback_rows = (int)fallback;
    return EHYB_OK;
}

extern "C" int ehyb_fsai_tt_step(int n, const double* t, double* s, int rz, void* stream)
{
    clear_error();
    if (n < 0 || !t || !s || rz < 0 || rz > 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_fsai_tt_step: bad arguments");
    launch_tt<1>(n, kMaxGrid / 2, (hipStream_t)stream, t, s, nullptr, 0, rz);
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}
