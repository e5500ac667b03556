// The CG loop around a preconditioner that brings kernels of its own (ehyb_cheb.hip, ehyb_coarse.hip): k solves that share
// Q = A P (ehyb_spmm with explicit walks; its pass of width 1 is ehyb_spmv_walk), the dot, update (no preconditioner) and
// direction kernels of ehyb_cg.hip, and between update and direction `precondition`, which leaves Z = M^-1 R for the live
// columns and the partials of r.z in the slot the update kernel would have filled.  Stopping, per-column freezing at check
// points, breakdown and the outputs are stated once, here.  One driver serves one and k right-hand sides, so column j of a
// k-column solve is the one-vector solve of b_j wherever the multiply is (plain storage).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <initializer_list>
#include <vector>

#include "cg_shared.h"
#include "ehyb_internal.h"
#include "solve_loop.h"

namespace {

inline int walk_of(int index) { return (index & 1) ? EHYB_WALK_LAST_TO_FIRST : EHYB_WALK_FIRST_TO_LAST; }

// what the loop owns and a preconditioner may use: k columns of n doubles each (Q is dead between update and the next multiply),
// the slots (A_COUNT per column) and the columns' flags
struct PcgState {
    int n, k, grid;
    hipStream_t st;
    double *R, *Pd, *Q, *Z, *s;
    int* active;
};
// a vector of the preconditioner's own, allocated (and zeroed) with the loop's
struct PcgExtra {
    double** ptr;
    size_t count;
};

// The arguments are checked.  prepare(S) runs once the vectors exist, before the first multiply, on the solve's stream;
// plan_walk(it) is the walk of iteration it's multiply (it = -1: the set-up, whose multiply walks against the first of
// iteration 0, which then starts on what it left in the caches); precondition(S, it, rz) enqueues Z = M^-1 R with the
// partials of r.z in slot number rz.  hint: what the breakdown message asks.
template <typename Prepare, typename Walk, typename Precondition>
int pcg_solve(const char* who, const char* hint, ehyb_plan* P, const double* B, int64_t ldb, double* X, int64_t ldx, int k, int max_iter,
              double rtol, int check_every, void* stream, int* iters_done, double* rel_residual, std::initializer_list<PcgExtra> extra,
              Prepare&& prepare, Walk&& plan_walk, Precondition&& precondition)
{
    using namespace ehyb;
    const int n = P->host.n_cols;
    SolveLoop L(n, check_every);
    const int grid = L.grid;
    double *R, *Pd, *Q, *Z, *s;
    HIP_TRY(L.begin(stream, {&R, &Pd, &Q, &Z}, (size_t)n * k, &s, (size_t)k * A_COUNT, (k + 1) / 2));  // the active flags behind the slots
    for (const PcgExtra& x : extra) HIP_TRY(L.more(x.ptr, x.count));
    int* active = (int*)(s + (size_t)k * A_COUNT * kMaxGrid);
    const hipStream_t st = L.st;
    const PcgState S{n, k, grid, st, R, Pd, Q, Z, s, active};

    int rc;
    if ((rc = prepare(S)) != EHYB_OK) return rc;

    if ((rc = ehyb_spmm(P, X, ldx, Q, n, k, st, plan_walk(-1))) != EHYB_OK) return rc;  // Q = A X0
    for (int j = 0; j < k; ++j)  // r = b - q, p = r; partials of r.r (twice) and b.b
        cg_launch_init(grid, st, n, B + (size_t)j * ldb, Q + (size_t)j * n, nullptr, R + (size_t)j * n, Pd + (size_t)j * n,
                       s + (size_t)j * A_COUNT * kMaxGrid);
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
    // p = z = M^-1 r; a column frozen from the start keeps p = 0 (the multiplies go over it)
    HIP_TRY(hipMemsetAsync(Z, 0, (size_t)n * k * sizeof(double), st));
    for (const PcgExtra& x : extra) HIP_TRY(hipMemsetAsync(*x.ptr, 0, x.count * sizeof(double), st));
    if ((rc = precondition(S, -1, 0)) != EHYB_OK) return rc;
    HIP_TRY(hipMemcpyAsync(Pd, Z, (size_t)n * k * sizeof(double), hipMemcpyDeviceToDevice, st));

    int it = 0;
    rc = L.run(
        P, max_iter, it, [&] { return n_live > 0; },
        [&](int cur, bool) -> int {
            // the plain launches (cfg.graphs = 2, the odd last iteration) are the captured ones
            int e = ehyb_spmm(P, Pd, n, Q, n, k, st, plan_walk(cur));  // Q = A P, frozen columns included (their q is not read)
            if (e != EHYB_OK) return e;
            for_each_group(k, [&](auto K, int c0) {
                cg_launch_dot(decltype(K)::value, grid, st, n, Pd, Q, s, active, c0);
                cg_launch_update(decltype(K)::value, grid, st, n, Pd, Q, nullptr, X, ldx, R, s, active, c0, cur);
            });
            if ((e = precondition(S, cur, cur ^ 1)) != EHYB_OK) return e;
            for_each_group(k, [&](auto K, int c0) { cg_launch_direction(decltype(K)::value, grid, st, n, Z, nullptr, Pd, s, active, c0, cur); });
            return EHYB_OK;
        },
        [&](int cur) -> int {
            bool changed = false;
            for (int j = 0; j < k; ++j) {
                if (!live[j]) continue;
                rs[j] = L.sum(j * A_COUNT + A_RR);
                const double rz = L.sum(j * A_COUNT + A_RZ0 + 2 * cur);
                // breakdown of this column (frozen, the others go on): a NaN, or -- short of convergence -- an r.z that is
                // not positive: the preconditioner was not positive definite
                if (!(rs[j] == rs[j]) || !(rz == rz) || (std::sqrt(rs[j] / bb[j]) > rtol && !(rz > 0))) rs[j] = NAN;
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
    if (broke) EHYB_FAIL(EHYB_ERR_ARG, "%s: breakdown%s (%s)", who, k > 1 ? " in a column" : "", hint);
    return EHYB_OK;
}

}  // namespace
