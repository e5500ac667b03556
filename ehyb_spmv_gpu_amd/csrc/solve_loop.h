// The host side of the device-resident solvers (ehyb_cg.hip, ehyb_bicgstab.hip, ehyb_refine.hip): the checks a solve or a
// *_step building block starts with, the split of k columns into launches, what a solve owns, and the loop that issues its
// iterations in bursts between check points.  A solver keeps its recurrences (one iteration of parity cur), its slot layout,
// and what it reads and decides at a check point.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "ehyb_internal.h"
#include "hip_try.h"
#include "vec_reduce.h"

namespace {

// in this order: the arguments (args_ok: the solver's own pointers), a plan over all rows, the upload; who: the entry point.
// solve_args is the part that returns EHYB_ERR_ARG: a solver with argument checks of its own runs them between the two.
inline int solve_args(const char* who, const ehyb_plan* P, bool args_ok, int max_iter, double rtol)
{
    ::ehyb::clear_error();
    if (!P || !args_ok) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    if (max_iter < 0 || !(rtol >= 0)) EHYB_FAIL(EHYB_ERR_ARG, "%s: max_iter %d, rtol %g", who, max_iter, rtol);
    if (P->host.row_begin != 0 || P->host.row_end != P->host.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "%s: needs a plan over all rows", who);
    return EHYB_OK;
}
inline int solve_uploaded(const char* who, const ehyb_plan* P)
{
    if (!P->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: plan not uploaded (no CPU fallback exists)", who);
    return EHYB_OK;
}
inline int solve_prologue(const char* who, const ehyb_plan* P, bool args_ok, int max_iter, double rtol)
{
    const int rc = solve_args(who, P, args_ok, max_iter, rtol);
    return rc != EHYB_OK ? rc : solve_uploaded(who, P);
}

// a k-column solve: k first, then the leading dimensions, then solve_prologue
inline int multi_args(const char* who, const ehyb_plan* P, int64_t ldb, int64_t ldx, int k)
{
    if (k < 1) EHYB_FAIL(EHYB_ERR_ARG, "%s: k = %d right-hand sides (at least 1)", who, k);
    if (P && (ldb < P->host.n_cols || ldx < P->host.n_cols))
        EHYB_FAIL(EHYB_ERR_ARG, "%s: ldb %lld, ldx %lld < %d rows", who, (long long)ldb, (long long)ldx, P->host.n_cols);
    return EHYB_OK;
}
inline int multi_prologue(const char* who, const ehyb_plan* P, bool args_ok, int64_t ldb, int64_t ldx, int k, int max_iter, double rtol)
{
    const int rc = multi_args(who, P, ldb, ldx, k);
    return rc != EHYB_OK ? rc : solve_prologue(who, P, args_ok, max_iter, rtol);
}

// a *_step building block: n and every pointer it requires (an optional one, dinv, is not listed)
inline int check_step(const char* who, int n, std::initializer_list<const void*> required)
{
    bool ok = n >= 0;
    for (const void* a : required) ok = ok && a;
    if (!ok) EHYB_FAIL(EHYB_ERR_ARG, "%s: bad arguments", who);
    return EHYB_OK;
}

constexpr int kMultiMaxK = 4;  // columns per vector-kernel launch

// f(K as an integral constant, c0) for k columns in groups of at most kMultiMaxK, as even as they come (k = 5: 3 + 2)
template <typename F>
void for_each_group(int k, F&& f)
{
    const int groups = (k + kMultiMaxK - 1) / kMultiMaxK;
    for (int g = 0, c0 = 0; g < groups; ++g) {
        const int w = k / groups + (g < k % groups ? 1 : 0);
        switch (w) {
        case 1: f(std::integral_constant<int, 1>{}, c0); break;
        case 2: f(std::integral_constant<int, 2>{}, c0); break;
        case 3: f(std::integral_constant<int, 3>{}, c0); break;
        default: f(std::integral_constant<int, 4>{}, c0); break;
        }
        c0 += w;
    }
}

// what a solve owns, released on every way out, and the loop that drives it
class SolveLoop {
public:
    // two workgroups per CU for every vector kernel: 115.7 us per CG iteration on the audikw_1-like matrix against 118-120 with
    // 1024 workgroups (twice the partials to re-add) and 126 with 256
    const int grid;
    hipStream_t st = nullptr;  // the caller's stream, or a private one (begin)
    std::vector<double> h;     // the slots as read() copied them last

    SolveLoop(int n, int check_every)
        : grid(std::max(1, std::min((n + kThreads - 1) / kThreads, kMaxGrid / 2))),
          every_(check_every <= 0 ? 10 : check_every + (check_every & 1))  // iterations are issued in even/odd pairs
    {
    }
    ~SolveLoop()
    {
        if (exec_) (void)hipGraphExecDestroy(exec_);
        if (graph_) (void)hipGraphDestroy(graph_);
        if (own_) (void)hipStreamDestroy(own_);
        for (void* a : bufs_) (void)hipFree(a);
    }

    // The stream -- a private (blocking) one if the caller passed none: the legacy default stream cannot be captured --, the
    // vectors (`count` doubles each), and the partial slots: `slots` of kMaxGrid doubles, `extra` doubles behind them for the
    // solver's flags.
    hipError_t begin(void* stream, std::initializer_list<double**> vectors, size_t count, double** s, size_t slots, size_t extra = 0)
    {
        hipError_t e = (st = (hipStream_t)stream) ? hipSuccess : hipStreamCreate(&own_);
        if (!st) st = own_;
        h.resize(slots * kMaxGrid + extra);
        for (double** a : vectors)
            if (e == hipSuccess) e = alloc(a, std::max<size_t>(1, count));
        if (e == hipSuccess && (e = alloc(s, h.size())) == hipSuccess) s_ = *s;
        return e;
    }
    // one more vector of the solve's, of a length of its own
    hipError_t more(double** p, size_t count) { return alloc(p, std::max<size_t>(1, count)); }

    // every launch so far checked, the slots copied into h, the stream drained
    hipError_t read()
    {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h.data(), s_, h.size() * sizeof(double), hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    }

    double sum(size_t slot) const  // of h, in the fixed order of the device
    {
        double t = 0.0;
        for (int i = 0; i < grid; ++i) t += h[slot * kMaxGrid + i];
        return t;
    }

    // Iterations while it < max_iter and live(), in bursts of check_every, each followed by a read() and check(cur): cur is the
    // parity of the iteration that would come next, whose alternating slots hold the latest values.  enqueue(cur, captured)
    // issues one iteration of parity cur.  An even and an odd iteration are captured once and replayed: one submission per two
    // iterations.  cfg.graphs = 2 keeps the plain launches (A/B, debugging), and so does a capture that fails.
    template <typename Live, typename Enqueue, typename Check>
    int run(const ehyb_plan* P, int max_iter, int& it, Live&& live, Enqueue&& enqueue, Check&& check)
    {
        if (P->cfg.graphs != 2 && max_iter >= 2 && live() && hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            int erc = enqueue(0, true);
            if (erc == EHYB_OK) erc = enqueue(1, true);
            const hipError_t eend = hipStreamEndCapture(st, &graph_);
            if (erc != EHYB_OK || eend != hipSuccess || hipGraphInstantiate(&exec_, graph_, nullptr, nullptr, 0) != hipSuccess)
                exec_ = nullptr;
            (void)hipGetLastError();
        }
        int rc;
        for (it = 0; it < max_iter && live();) {
            const int burst = std::min(every_, max_iter - it);  // even, except possibly the very last one
            int k = 0;
            for (; k + 2 <= burst; k += 2) {
                if (exec_)
                    HIP_TRY(hipGraphLaunch(exec_, st));
                else if ((rc = enqueue(0, false)) != EHYB_OK || (rc = enqueue(1, false)) != EHYB_OK)
                    return rc;
            }
            if (k < burst && (rc = enqueue(0, false)) != EHYB_OK) return rc;
            it += burst;
            HIP_TRY(read());
            if ((rc = check(burst & 1)) != EHYB_OK) return rc;
        }
        return EHYB_OK;
    }

private:
    hipError_t alloc(double** p, size_t count)
    {
        const hipError_t e = hipMalloc((void**)p, count * sizeof(double));
        if (e == hipSuccess) bufs_.push_back(*p);
        return e;
    }

    const int every_;
    std::vector<void*> bufs_;
    double* s_ = nullptr;
    hipStream_t own_ = nullptr;
    hipGraph_t graph_ = nullptr;
    hipGraphExec_t exec_ = nullptr;
};

}  // namespace
