// What the drivers on the pair A / A^T share on the host (ehyb_lsqr.hip, ehyb_svds.hip): the checks of (plan, plan_t) in the order
// of include/ehyb.h, and the transposed multiply.  plan_t is a plan of A^T in the numbering of plan, plan itself (the caller's
// statement that A is symmetric) or NULL: then every A^T multiply is ehyb_spmv_t on the plan of A.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "ehyb_internal.h"
#include "solve_loop.h"

namespace {

// EHYB_ERR_ARG: a plan not over all rows; a plan_t of another dimension or not over all rows; with plan_t NULL what
// ehyb_spmv_t_supported refuses (the form is named in ehyb_last_error)
inline int pair_args(const char* who, const ehyb_plan* P, const ehyb_plan* PT)
{
    if (P->host.row_begin != 0 || P->host.row_end != P->host.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "%s: needs a plan over all rows", who);
    if (PT && PT->host.n_cols != P->host.n_cols)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: plan_t has %d rows, plan %d (pad a rectangular matrix to square)", who, PT->host.n_cols, P->host.n_cols);
    if (PT && (PT->host.row_begin != 0 || PT->host.row_end != PT->host.n_cols))
        EHYB_FAIL(EHYB_ERR_ARG, "%s: needs a plan_t over all rows", who);
    if (!PT) return ehyb_spmv_t_supported(P);
    return EHYB_OK;
}

// EHYB_ERR_STATE for a plan, then a plan_t, never uploaded
inline int pair_uploaded(const char* who, const ehyb_plan* P, const ehyb_plan* PT)
{
    const int rc = solve_uploaded(who, P);
    if (rc != EHYB_OK) return rc;
    if (PT && !PT->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: plan_t not uploaded (no CPU fallback exists)", who);
    return EHYB_OK;
}

// out = A^T in for k columns of leading dimension n: one ehyb_spmm on the plan of A^T, or column by column on the plan of A
inline int multiply_t(ehyb_plan* P, ehyb_plan* PT, const double* in, double* out, int n, int k, hipStream_t st, int walk)
{
    if (PT) return ehyb_spmm(PT, in, n, out, n, k, st, walk);
    for (int j = 0; j < k; ++j) {
        const int e = ehyb_spmv_t(P, in + (size_t)j * n, out + (size_t)j * n, st);
        if (e != EHYB_OK) return e;
    }
    return EHYB_OK;
}

}  // namespace
