// The object behind ehyb_bilu (include/ehyb.h): the block ILU(0) preconditioner of ehyb_gmres_bilu and ehyb_bicgstab_bilu.
// bilu.cpp builds the host side (the blocks and local order of ehyb_bic, the ILU(0) factor of every diagonal block, the levels
// of the two solves; no GPU needed).  The device side is ehyb_bic's: the same streams, the same apply kernel, the same upload and
// release (ehyb_bic.hip), fed with L and ones for the forward solve and U and 1 / u_ii for the backward one.
#pragma once
#include <cstdint>
#include <vector>

#include "bic.h"
#include "ehyb_internal.h"

struct ehyb_bilu {
    // n, nb, order, max_block, counts, block_ptr, perm, shift as in ehyb_bic; row_ptr / cols / vals: the strictly lower part of the
    // unit lower L; dinv: ones (the forward solve's multiplier); level_f from L, level_b from U; and the device side
    ehyb_bic core;
    std::vector<int64_t> u_row_ptr;  // [n + 1] U in CSR form in position order, strictly upper part
    std::vector<int32_t> u_cols;     // [nnz(U)] block-local positions, rising in a row
    std::vector<double> u_vals;      // [nnz(U)]
    std::vector<double> u_dinv;      // [n] 1 / u_ii
};

namespace ehyb {
// the two triangles of f as the stream builder takes them
inline void bilu_triangles(const ehyb_bilu& f, BicTriangle (&tri)[2])
{
    tri[0] = {f.core.row_ptr.data(), f.core.cols.data(), f.core.vals.data(), f.core.dinv.data(), f.core.level_f.data()};
    tri[1] = {f.u_row_ptr.data(), f.u_cols.data(), f.u_vals.data(), f.u_dinv.data(), f.core.level_b.data()};
}

// what a *_bilu solver checks after what its Jacobi counterpart rejects, in this order: the factor, then the uploads
inline int bilu_solver_args(const char* who, const ehyb_plan* P, const ehyb_bilu* f)
{
    if (!f) EHYB_FAIL(EHYB_ERR_ARG, "%s: null bilu object", who);
    if (f->core.n != P->host.n_cols) EHYB_FAIL(EHYB_ERR_ARG, "%s: the bilu object has %d rows, the plan %d", who, f->core.n, P->host.n_cols);
    if (!P->uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: plan not uploaded (no CPU fallback exists)", who);
    if (!f->core.uploaded) EHYB_FAIL(EHYB_ERR_STATE, "%s: bilu object not uploaded", who);
    return EHYB_OK;
}
}  // namespace ehyb
