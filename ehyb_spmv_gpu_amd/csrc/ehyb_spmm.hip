// Y = A X for k columns per pass over the matrix (ehyb_spmm, include/ehyb.h).  The value stream, the column words, the lane maps
// and the slab records are read ONCE per pass for up to k_max columns; a multiply moves about matrix + k (x + y) bytes instead of
// k (matrix + x + y).  A pass of width 2..4 is one launch of the window kernel and, unless the residual rides inline, one of the
// CSR-segment residual, both K columns wide (ell_device.h, launched by ehyb_hip.hip); on a plan whose residual is in panel form,
// the window launch (if the plan kept windows) and the two panel passes, K wide; a pass of width 1 is ehyb_spmv_walk itself.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ehyb_internal.h"
#include "ell_device.h"

using namespace ehyb;

// (ehyb_spmm_max_k is host arithmetic: plan.cpp)

int ehyb_spmm(ehyb_plan* P, const double* X, int64_t ldx, double* Y, int64_t ldy, int k, void* stream, int walk)
{
    clear_error();
    if (!P || !X || !Y) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm: null argument");
    if (k < 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm: k = %d columns (at least 1)", k);
    const HostLayout& H = P->host;
    if (ldx < H.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm: ldx %lld < %d columns of the matrix", (long long)ldx, H.n_cols);
    if (ldy < H.row_end) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm: ldy %lld < %d rows", (long long)ldy, H.row_end);
    if (walk < -1 || walk > 1) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_spmm: walk %d (EHYB_WALK_AUTO, _FIRST_TO_LAST, _LAST_TO_FIRST)", walk);
    if (!P->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "ehyb_spmm: plan not uploaded (no CPU fallback exists)");
    hipStream_t st = (hipStream_t)stream;
    // ceil(k / k_max) passes over the matrix, as even as they come (k = 5 on a plan of k_max 4: 3 + 2)
    const int kmax = plan_spmm_width(P), passes = (k + kmax - 1) / kmax;
    int j0 = 0;
    for (int p = 0; p < passes; ++p) {
        const int w = k / passes + (p < k % passes ? 1 : 0);
        const double* Xp = X + (int64_t)j0 * ldx;
        double* Yp = Y + (int64_t)j0 * ldy;
        int rc;
        if (w == 1) {
            rc = ehyb_spmv_walk(P, Xp, Yp, stream, walk);  // the one-vector launch sequence
        } else {
            rc = launch_window(P, Xp, ldx, Yp, ldy, w, st, H.inline_er, walk);
            if (rc == EHYB_OK && H.er_panel) rc = launch_panel_k(P, Xp, ldx, Yp, ldy, w, st, walk);  // (never inline; no window launch where no partition kept one)
            else if (rc == EHYB_OK && !H.inline_er) rc = launch_er_csr(P, Xp, ldx, Yp, ldy, w, st);
        }
        if (rc != EHYB_OK) return rc;
        j0 += w;
    }
    return EHYB_OK;
}
