// PCG with a block incomplete Cholesky preconditioner (ehyb_pcg_bic, ehyb_pcg_bic_multi, ehyb_bic_apply): the CG loop of
// pcg_loop.h around Z = (L L^T)^-1 R, L the IC(0) factor of every diagonal block of the reordered matrix (bic.cpp).  The kernels:
//   apply   one workgroup per block: the block's rows of R (through PERM) into LDS, the forward solve with L and the backward
//           solve with L^T in place there, the rows of Z out (through PERM)
//   rz      the partials of r.z                                   the walk of the other vector kernels
//
// The apply kernel.  A block's vector -- rows x K doubles, K <= ehyb_bic_max_k columns -- is the whole dynamic LDS of the
// workgroup (up to 160 KiB: the kernel declares no static LDS and opts in to the large LDS like the window kernels).  A solve
// goes level by level, the levels of bic.cpp: the rows of a level depend on rows of lower levels alone, so they are served
// together and a __syncthreads() ends the level.  Every thread of the workgroup executes the same barriers: the rounds of a
// direction come from the block's record, and what a round does -- its rows, its lane groups, its passes, whether it ends a
// level -- from the round's word and the pass counts, the same in every thread, never from a lane's data.  No workgroup waits
// for another: no flag, no counter, no atomics.
//   A level of w rows is served by lane groups of g = 2^gl lanes (bic_group_log2), threads / g rows a round.  Lane j of a group
//   takes entries j, j + g, ... of its row -- one fma each into one accumulator per column, in rising stream order -- then the
//   g accumulators are added by a fixed xor-shuffle tree and lane 0 of the group stores x = (x - sum) * dinv.  The order of a
//   row's sum depends on g alone, never on K: column j of a K-column apply has the bits of the one-column apply.
//   The stream of a round holds, pass by pass, (rows that reach the pass) * g (column, value) pairs at [pass][lane]: consecutive
//   lanes read consecutive addresses, every word once.  The rows of a level fall in length, so the rows that reach a pass are
//   the round's first ones and a pass is not padded to the longest row (jagged diagonals); kBicNoEntry fills what a row lacks of
//   its own last pass.  The columns are 16-bit block-local positions.
// Every index the kernel forms comes from arrays bic.cpp built and checked: columns below the block's length, rows a permutation
// of it, PERM a permutation of 0 .. n - 1.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bic.h"
#include "bilu.h"
#include "pcg_loop.h"
#include "vec_walk.h"

using namespace ehyb;

namespace {

constexpr int kBicMaxThreads = 1024;
constexpr int kBicLdsBytes = EHYB_BIC_MAX_BLOCK * 8;

template <int K>
__global__ __launch_bounds__(kBicMaxThreads) void ehyb_bic_apply_kernel(int n, const BicBlock* __restrict__ blocks, const int32_t* __restrict__ order,
                                                                        const int32_t* __restrict__ perm, const uint32_t* __restrict__ rounds,
                                                                        const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ meta,
                                                                        const double* __restrict__ dinv, const uint16_t* __restrict__ cols,
                                                                        const double* __restrict__ vals, const double* __restrict__ R, long long ldr,
                                                                        double* __restrict__ Z, long long ldz, const int* __restrict__ active, int astride,
                                                                        int inverted, int c0)
{
    extern __shared__ __attribute__((aligned(16))) double xs[];
    const BicBlock B = blocks[order[blockIdx.x]];
    const int T = (int)blockDim.x, t = (int)threadIdx.x;
    const int rows = B.rows;
    bool on[K];
    bool any = false;
#pragma unroll
    for (int c = 0; c < K; ++c) {
        // column c's flag: the word at active[(c0 + c) * astride], on where it is nonzero -- or, inverted, where it is zero (a
        // solver's status word, 0 while the column runs)
        on[c] = !active || (active[(size_t)(c0 + c) * astride] != 0) != (inverted != 0);
        any = any || on[c];
    }
    if (!any) return;  // (the same in every thread)
    for (int i = t; i < rows; i += T) {
        const size_t src = (size_t)perm[B.row0 + i];
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) xs[c * rows + i] = R[(size_t)(c0 + c) * ldr + src];
    }
    __syncthreads();
    for (int dir = 0; dir < 2; ++dir) {
        size_t slot = (size_t)dir * n + B.row0;
        long long ent = B.ent0[dir];
        const uint32_t* rw = rounds + B.rnd0[dir];
        const uint32_t* pc = cnt + B.cnt0[dir];
        const int nround = B.nround[dir];
        for (int r = 0; r < nround; ++r) {
            // (the round's word is the same in every thread, and with it every trip count and the barrier below)
            const uint32_t word = rw[r];
            const int nr = (int)(word & 0x7FF), gl = (int)(word >> 11 & 7), g = 1 << gl, passes = (int)(word >> 15);
            const bool last = (word >> 14 & 1) != 0;
            const int grp = t >> gl, j = t & (g - 1);
            const bool mine = grp < nr;
            // the row and its 1 / l_ii: asked for before the stream, used after it
            uint32_t mw = 0;
            double di = 0.0;
            if (mine) {
                mw = meta[slot + grp];
                di = dinv[slot + grp];
            }
            double acc[K];
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = 0.0;
            for (int p = 0; p < passes; p += 4) {  // four passes a trip: their counts, their loads, then their terms in rising order
                int live[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) live[u] = p + u < passes ? (int)pc[p + u] : 0;
                uint16_t cc[4];
                double vv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    cc[u] = kBicNoEntry;
                    vv[u] = 0.0;
                    if (grp < live[u]) {  // (live <= nr: the rows of a round fall in length)
                        cc[u] = cols[ent + t];
                        vv[u] = vals[ent + t];
                    }
                    ent += (long long)live[u] << gl;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (cc[u] == kBicNoEntry) continue;
#pragma unroll
                    for (int c = 0; c < K; ++c)
                        if (on[c]) acc[c] = fma(vv[u], xs[c * rows + cc[u]], acc[c]);
                }
            }
            pc += passes;
            for (int off = g >> 1; off > 0; off >>= 1) {  // (g, and with it the tree, is the same in every thread)
#pragma unroll
                for (int c = 0; c < K; ++c) acc[c] += __shfl_xor(acc[c], off, 64);
            }
            if (mine && j == 0) {
                const int row = (int)(mw & 0xFFFF);
#pragma unroll
                for (int c = 0; c < K; ++c)
                    if (on[c]) xs[c * rows + row] = (xs[c * rows + row] - acc[c]) * di;
            }
            slot += nr;
            if (last) __syncthreads();
        }
    }
    for (int i = t; i < rows; i += T) {
        const size_t dst = (size_t)perm[B.row0 + i];
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) Z[(size_t)(c0 + c) * ldz + dst] = xs[c * rows + i];
    }
}

// the partials of r.z into r.z slot number rz: the grid, the walk and the tail of fsai_tt_kernel
template <int K>
__global__ __launch_bounds__(kThreads) void bic_rz_kernel(int n, const double* __restrict__ R, const double* __restrict__ Zv, double* __restrict__ s,
                                                          const int* __restrict__ active, int c0, int rz)
{
    bool on[K];
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        on[c] = (K == 1 && !active) || active[c0 + c] != 0;
        acc[c] = 0.0;
    }
    walk<K, kWalkU, 2>(
        n, on, NoShared{},
        [&](int c, int i, double(&in)[2], int) {
            in[0] = R[(size_t)(c0 + c) * n + i];
            in[1] = Zv[(size_t)(c0 + c) * n + i];
        },
        [&](int c, int, const double(&in)[2], int) { acc[c] = fma(in[0], in[1], acc[c]); });
    block_sum_n(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (on[c]) slot<A_COUNT>(s, c0 + c, A_RZ0 + 2 * rz)[blockIdx.x] = acc[c];
    }
}

template <int K>
void launch_rz(int n, int grid, hipStream_t st, const double* R, const double* Zv, double* s, const int* active, int c0, int rz)
{
    hipLaunchKernelGGL(bic_rz_kernel<K>, dim3(grid), dim3(kThreads), 0, st, n, R, Zv, s, active, c0, rz);
}

template <int K>
void launch_apply(const ehyb_bic* f, hipStream_t st, const double* R, long long ldr, double* Z, long long ldz, const int* active, int astride, int inverted,
                  int c0)
{
    const size_t lds = (size_t)f->max_block * K * sizeof(double);
    hipLaunchKernelGGL(ehyb_bic_apply_kernel<K>, dim3(f->nb), dim3(f->threads), lds, st, f->n, f->d_blocks, f->d_order, f->d_perm, f->d_rounds, f->d_cnt, f->d_meta,
                       f->d_dinv, f->d_cols, f->d_vals, R, ldr, Z, ldz, active, astride, inverted, c0);
}

}  // namespace

// Z = (L L^T)^-1 R -- or (L U)^-1 R: whatever the streams hold -- for k columns, in passes of ehyb_bic_max_k columns
int ehyb::bic_apply_columns(const ehyb_bic* f, void* stream, const double* R, long long ldr, double* Z, long long ldz, int k, const int* active,
                            int astride, bool inverted)
{
    const hipStream_t st = (hipStream_t)stream;
    const int kmax = ehyb_bic_max_k(f);
    for (int c0 = 0; c0 < k; c0 += kmax) {
        switch (std::min(kmax, k - c0)) {
        case 1: launch_apply<1>(f, st, R, ldr, Z, ldz, active, astride, inverted, c0); break;
        case 2: launch_apply<2>(f, st, R, ldr, Z, ldz, active, astride, inverted, c0); break;
        case 3: launch_apply<3>(f, st, R, ldr, Z, ldz, active, astride, inverted, c0); break;
        default: launch_apply<4>(f, st, R, ldr, Z, ldz, active, astride, inverted, c0); break;
        }
    }
    HIP_TRY(hipGetLastError());
    return EHYB_OK;
}

namespace {

template <typename T>
hipError_t to_device(T** d, const T* h, size_t count)
{
    hipError_t e = hipMalloc((void**)d, std::max<size_t>(1, count) * sizeof(T));
    if (e == hipSuccess && count) e = hipMemcpy(*d, h, count * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

}  // namespace

void ehyb::bic_release_device(ehyb_bic* f)
{
    for (void* p : {(void*)f->d_blocks, (void*)f->d_order, (void*)f->d_perm, (void*)f->d_rounds, (void*)f->d_cnt, (void*)f->d_meta, (void*)f->d_dinv, (void*)f->d_cols,
                    (void*)f->d_vals})
        if (p) (void)hipFree(p);
    f->d_blocks = nullptr;
    f->d_order = f->d_perm = nullptr;
    f->d_rounds = f->d_cnt = f->d_meta = nullptr;
    f->d_dinv = f->d_vals = nullptr;
    f->d_cols = nullptr;
    f->uploaded = false;
}

int ehyb::bic_upload_streams(const char* who, ehyb_bic* f, const BicStreams& S)
{
    f->threads = S.threads;
    f->stream_bytes = S.bytes();
    f->stream_entries = S.real_entries;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ehyb_bic_apply_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, kBicLdsBytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(ehyb_bic_apply_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, kBicLdsBytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(ehyb_bic_apply_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize, kBicLdsBytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(ehyb_bic_apply_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, kBicLdsBytes);
    if (e == hipSuccess) e = to_device(&f->d_blocks, S.blocks.data(), S.blocks.size());
    if (e == hipSuccess) e = to_device(&f->d_order, S.launch_order.data(), S.launch_order.size());
    if (e == hipSuccess) e = to_device(&f->d_perm, f->perm.data(), f->perm.size());
    if (e == hipSuccess) e = to_device(&f->d_rounds, S.rounds.data(), S.rounds.size());
    if (e == hipSuccess) e = to_device(&f->d_cnt, S.cnt.data(), S.cnt.size());
    if (e == hipSuccess) e = to_device(&f->d_meta, S.meta.data(), S.meta.size());
    if (e == hipSuccess) e = to_device(&f->d_dinv, S.dinv.data(), S.dinv.size());
    if (e == hipSuccess) e = to_device(&f->d_cols, S.cols.data(), S.cols.size());
    if (e == hipSuccess) e = to_device(&f->d_vals, S.vals.data(), S.vals.size());
    if (e != hipSuccess) {
        bic_release_device(f);
        EHYB_FAIL(EHYB_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    f->uploaded = true;
    return EHYB_OK;
}

namespace {

// in this order: what the plain solver rejects (done by the caller), the object, then the uploads
int bic_args(const char* who, const ehyb_plan* P, const ehyb_bic* f)
{
    if (!f) EHYB_FAIL(EHYB_ERR_ARG, "%s: null bic object", who);
    if (f->n != P->host.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "%s: the bic object has %d rows, the plan %d", who, f->n, P->host.n_cols);
    int rc = solve_uploaded(who, P);
    if (rc != EHYB_OK) return rc;
    if (!f->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: bic object not uploaded", who);
    return EHYB_OK;
}

// The one driver: the loop of pcg_loop.h, one multiply with A per iteration (walks alternating), the two solves and the
// partials of r.z between update and direction.  The arguments are checked.
int bic_solve(const char* who, ehyb_plan* P, ehyb_bic* f, const double* B, int64_t ldb, double* X, int64_t ldx, int k, int max_iter, double rtol,
              int check_every, void* stream, int* iters_done, double* rel_residual)
{
    auto precondition = [&](const PcgState& S, int, int rz) -> int {
        const int rc = bic_apply_columns(f, S.st, S.R, S.n, S.Z, S.n, k, S.active);
        if (rc != EHYB_OK) return rc;
        for_each_group(k, [&](auto K, int c0) { launch_rz<decltype(K)::value>(S.n, S.grid, S.st, S.R, S.Z, S.s, S.active, c0, rz); });
        return EHYB_OK;
    };
    return pcg_solve(
        who, "is the matrix symmetric positive definite?", P, B, ldb, X, ldx, k, max_iter, rtol, check_every, stream, iters_done, rel_residual, {},
        [](const PcgState&) { return EHYB_OK; }, [](int it) { return walk_of(it); }, precondition);
}

}  // namespace

extern "C" int ehyb_bic_upload(ehyb_bic* f)
{
    clear_error();
    if (!f) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_bic_upload: null argument");
    if (f->uploaded) return EHYB_OK;
    BicStreams S;
    bic_build_streams(*f, bic_threads(f->max_block), &S);
    return bic_upload_streams("ehyb_bic_upload", f, S);
}

extern "C" void ehyb_bic_destroy(ehyb_bic* f)
{
    if (!f) return;
    if (f->uploaded) bic_release_device(f);
    delete f;
}

namespace {

// the three entry points both objects have, on the part they share; who: the entry point, what: the object's name in messages
int stream_info_of(const char* who, const char* what, const ehyb_bic* f, int64_t* bytes, int64_t* entries, int* threads)
{
    clear_error();
    if (!f || !bytes || !entries || !threads) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    if (!f->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: %s object not uploaded", who, what);
    *bytes = f->stream_bytes, *entries = f->stream_entries, *threads = f->threads;
    return EHYB_OK;
}

// step: the flags are required
int apply_of(const char* who, const char* what, const ehyb_bic* f, const double* R, int64_t ldr, double* Z, int64_t ldz, int k, bool step, const int* active,
             void* stream)
{
    clear_error();
    if (!f || !R || !Z || (step && !active)) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    if (k < 1 || ldr < f->n || ldz < f->n) EHYB_FAIL(EHYB_ERR_ARG, "%s: k = %d, ldr = %lld, ldz = %lld (k >= 1, both at least n = %d)", who, k, (long long)ldr, (long long)ldz, f->n);
    if (!f->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: %s object not uploaded", who, what);
    return bic_apply_columns(f, stream, R, ldr, Z, ldz, k, active);
}

}  // namespace

extern "C" int ehyb_bic_stream_info(const ehyb_bic* f, int64_t* bytes, int64_t* entries, int* threads)
{
    return stream_info_of("ehyb_bic_stream_info", "bic", f, bytes, entries, threads);
}

extern "C" int ehyb_bic_apply(ehyb_bic* f, const double* R, int64_t ldr, double* Z, int64_t ldz, int k, void* stream)
{
    return apply_of("ehyb_bic_apply", "bic", f, R, ldr, Z, ldz, k, false, nullptr, stream);
}

extern "C" int ehyb_bic_apply_step(ehyb_bic* f, const double* R, int64_t ldr, double* Z, int64_t ldz, int k, const int* active, void* stream)
{
    return apply_of("ehyb_bic_apply_step", "bic", f, R, ldr, Z, ldz, k, true, active, stream);
}

// ------------------------------------------------------------------ ehyb_bilu: the same device side, fed with L and U (bilu.cpp)
extern "C" int ehyb_bilu_upload(ehyb_bilu* f)
{
    clear_error();
    if (!f) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_bilu_upload: null argument");
    if (f->core.uploaded) return EHYB_OK;
    BicTriangle tri[2];
    bilu_triangles(*f, tri);
    BicStreams S;
    bic_build_streams(f->core.n, f->core.nb, f->core.block_ptr.data(), tri, bic_threads(f->core.max_block), &S);
    return bic_upload_streams("ehyb_bilu_upload", &f->core, S);
}

extern "C" void ehyb_bilu_destroy(ehyb_bilu* f)
{
    if (!f) return;
    if (f->core.uploaded) bic_release_device(&f->core);
    delete f;
}

extern "C" int ehyb_bilu_stream_info(const ehyb_bilu* f, int64_t* bytes, int64_t* entries, int* threads)
{
    return stream_info_of("ehyb_bilu_stream_info", "bilu", f ? &f->core : nullptr, bytes, entries, threads);
}

extern "C" int ehyb_bilu_apply(ehyb_bilu* f, const double* R, int64_t ldr, double* Z, int64_t ldz, int k, void* stream)
{
    return apply_of("ehyb_bilu_apply", "bilu", f ? &f->core : nullptr, R, ldr, Z, ldz, k, false, nullptr, stream);
}

extern "C" int ehyb_bilu_apply_step(ehyb_bilu* f, const double* R, int64_t ldr, double* Z, int64_t ldz, int k, const int* active, void* stream)
{
    return apply_of("ehyb_bilu_apply_step", "bilu", f ? &f->core : nullptr, R, ldr, Z, ldz, k, true, active, stream);
}

extern "C" int ehyb_pcg_bic(ehyb_plan* P, ehyb_bic* f, const double* b, double* x, int max_iter, double rtol, int check_every, void* stream,
                            int* iters_done, double* rel_residual)
{
    const char* who = "ehyb_pcg_bic";
    int rc = solve_args(who, P, b && x, max_iter, rtol);
    if (rc != EHYB_OK || (rc = bic_args(who, P, f)) != EHYB_OK) return rc;
    const int n = P->host.n_cols;
    return bic_solve(who, P, f, b, n, x, n, 1, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}

extern "C" int ehyb_pcg_bic_multi(ehyb_plan* P, ehyb_bic* f, const double* B, int64_t ldb, double* X, int64_t ldx, int k, int max_iter, double rtol,
                                  int check_every, void* stream, int* iters_done, double* rel_residual)
{
    const char* who = "ehyb_pcg_bic_multi";
    int rc = multi_args(who, P, ldb, ldx, k);
    if (rc == EHYB_OK) rc = solve_args(who, P, B && X, max_iter, rtol);
    if (rc != EHYB_OK || (rc = bic_args(who, P, f)) != EHYB_OK) return rc;
    return bic_solve(who, P, f, B, ldb, X, ldx, k, max_iter, rtol, check_every, stream, iters_done, rel_residual);
}
