// The object behind ehyb_fsai (include/ehyb.h): the factorised sparse approximate inverse G of ehyb_pcg_fsai.  fsai.cpp builds the
// host side (pattern, values, the plans of G and G^T; no GPU needed), ehyb_fsai.hip uploads it, repeats the numeric phase on the
// device, applies it and releases it.
#pragma once
#include <cstdint>
#include <vector>

#include "ehyb.h"

struct ehyb_fsai {
    int n = 0;        // rows of the matrix
    int row_cap = 0;  // longest row of G allowed (1 .. EHYB_FSAI_MAX_ROW)
    int max_row = 0;  // longest row of G there is: sizes the factor kernel's LDS
    int transpose_mode = 0;
    int64_t counts[2] = {0, 0};  // capped rows, fallback rows (EHYB_FSAI_COUNTS)
    std::vector<int64_t> row_ptr;  // [n + 1] G in CSR form, the columns of a row rising, the diagonal last
    std::vector<int32_t> cols;     // [nnz(G)]
    std::vector<double> vals;      // [nnz(G)]
    std::vector<int32_t> order_t;  // [nnz(G)] entry k of G^T (CSR order) is entry order_t[k] of G: the entry order of plan_t
    std::vector<int32_t> a_ptr;    // [n + 1] the pattern of A, for the numeric phase on the device
    std::vector<int32_t> a_cols;   // [nnz(A)]
    ehyb_plan* plan_g = nullptr;   // G, on the matrix's partitions
    ehyb_plan* plan_t = nullptr;   // G^T (transpose_mode 0), else null: ehyb_spmv_t on plan_g
    bool uploaded = false;
    int32_t* d_a_ptr = nullptr;
    int32_t* d_a_cols = nullptr;
    int64_t* d_row_ptr = nullptr;
    int32_t* d_cols = nullptr;
    int32_t* d_order_t = nullptr;
    double* d_vals = nullptr;  // [nnz(G)] what the factor kernel writes and ehyb_plan_set_values gathers from
    double* d_t = nullptr;     // [n] t = G r of ehyb_fsai_apply: one apply at a time per object
    int* d_count = nullptr;    // [4] fallback rows, rows whose a_ii is not positive and finite, entry_order values out of range
};

namespace ehyb {

// One row of G from its dense block, by the rules of include/ehyb.h.  S: the lower triangle of A[J, J], packed by rows
// (S[r (r + 1) / 2 + c], c <= r), overwritten by its Cholesky factor; g: m values out.  false: a pivot is not a positive finite
// number (g untouched).  The order of every sum is stated in include/ehyb.h; the factor kernel follows the same one.
bool fsai_row(double* S, int m, double* g);

}  // namespace ehyb
