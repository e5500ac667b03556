// The host side of the block ILU(0) preconditioner (ehyb_gmres_bilu, ehyb_bicgstab_bilu): the blocks and the local order of
// ehyb_bic (bic.cpp: the same code), the ILU(0) factor L U ~ A_b of every diagonal block with the pivot rule and the shift
// ladder, and the levels of the two triangular solves.  No GPU is needed here.  A block depends on nothing but the matrix:
// OpenMP threads share out whole blocks, never the terms of a sum, and every sum runs in the order include/ehyb.h states, so the
// result does not depend on the number of threads.  The device streams are bic_build_streams's, fed with the two triangles.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>

#include "bilu.h"
#include "ehyb_internal.h"

using namespace ehyb;

namespace {

// A_b in local order, duplicates summed, the diagonal always present: CSR over the block's positions, columns rising
struct BlockPattern {
    std::vector<int64_t> rp;       // [rows + 1]
    std::vector<int32_t> cols;     // block-local
    std::vector<double> a;         // the values of A_b
    std::vector<int64_t> diag_at;  // [rows] the diagonal's entry
    std::vector<double> s;         // [rows] sum_j |a_ij|, rising j
};

// what one block leaves: both triangles in CSR form over its positions, 1 / u_ii, the alpha
struct BlockFactor {
    std::vector<int64_t> lrp, urp;
    std::vector<int32_t> lcols, ucols;
    std::vector<double> lvals, uvals, udinv;
    double shift = 0.0;
};

constexpr double kPivotFloor = 0x1p-26;

// row-wise IKJ ILU(0) of A_b + alpha diag(s) in place in w (w = a on entry, but for the diagonal): k rising, j rising.  where:
// rows ints of -1, left so.  false: a pivot that is not finite or not above 2^-26 s_i.
bool factor_block(int rows, const BlockPattern& B, double alpha, double* w, int32_t* where)
{
    std::memcpy(w, B.a.data(), B.a.size() * sizeof(double));
    if (alpha != 0)
        for (int i = 0; i < rows; ++i) w[B.diag_at[i]] = B.a[B.diag_at[i]] + alpha * B.s[i];
    for (int i = 0; i < rows; ++i) {
        const int64_t lo = B.rp[i], hi = B.rp[i + 1], di = B.diag_at[i];
        for (int64_t e = lo; e < hi; ++e) where[B.cols[e]] = (int32_t)(e - lo);
        for (int64_t e = lo; e < di; ++e) {
            const int k = B.cols[e];
            const double lik = w[e] / w[B.diag_at[k]];
            w[e] = lik;
            for (int64_t q = B.diag_at[k] + 1; q < B.rp[k + 1]; ++q) {
                const int32_t at = where[B.cols[q]];
                if (at >= 0) w[lo + at] = w[lo + at] - lik * w[q];
            }
        }
        for (int64_t e = lo; e < hi; ++e) where[B.cols[e]] = -1;
        const double u = w[di];
        if (!std::isfinite(u) || !(std::fabs(u) > kPivotFloor * B.s[i])) return false;
    }
    return true;
}

// LEVEL_F from L's rows, LEVEL_B from U's, and the most levels of any block
void compute_levels(ehyb_bilu* f)
{
    ehyb_bic& c = f->core;
    const int n = c.n;
    c.level_f.assign((size_t)n, 0);
    c.level_b.assign((size_t)n, 0);
    int most = 0;
    for (int b = 0; b < c.nb; ++b) {
        const int r0 = c.block_ptr[b], r1 = c.block_ptr[b + 1];
        for (int p = r0; p < r1; ++p) {
            int lv = 0;
            for (int64_t e = c.row_ptr[p]; e < c.row_ptr[p + 1]; ++e) lv = std::max(lv, c.level_f[(size_t)r0 + c.cols[e]] + 1);
            c.level_f[p] = lv;
            most = std::max(most, lv + 1);
        }
        for (int p = r1 - 1; p >= r0; --p) {
            int lv = 0;
            for (int64_t e = f->u_row_ptr[p]; e < f->u_row_ptr[p + 1]; ++e) lv = std::max(lv, c.level_b[(size_t)r0 + f->u_cols[e]] + 1);
            c.level_b[p] = lv;
            most = std::max(most, lv + 1);
        }
    }
    c.counts[3] = n ? most : 0;
}

}  // namespace

extern "C" int ehyb_bilu_create_host(const matrixCOO* m, int block_rows, int order, ehyb_bilu** out)
{
    const char* who = "ehyb_bilu_create_host";
    clear_error();
    if (!m || !m->rowIdx || !m->J || !m->V || m->dimension < 1 || !out) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    const int rc = bic_check_matrix(who, m, block_rows, order);
    if (rc != EHYB_OK) return rc;
    const int n = m->dimension;
    std::unique_ptr<ehyb_bilu> f(new (std::nothrow) ehyb_bilu);
    if (!f) EHYB_FAIL(EHYB_ERR_ALLOC, "%s: out of memory", who);
    ehyb_bic& c = f->core;
    c.n = n;
    c.order = order;
    const int threads = bic_host_threads();
    bic_cut_blocks(m, block_rows, &c);
    const int nb = c.nb;
    c.perm.resize((size_t)n);
    c.shift.assign((size_t)nb, 0.0);
    std::vector<int32_t> pos((size_t)n);  // block-local position of a row
    std::vector<BlockFactor> parts((size_t)nb);
    int64_t n_shifted = 0, n_fallback = 0;

#pragma omp parallel for schedule(dynamic, 1) num_threads(threads) reduction(+ : n_shifted, n_fallback)
    for (int b = 0; b < nb; ++b) {
        const int r0 = c.block_ptr[b], r1 = c.block_ptr[b + 1], rows = r1 - r0;
        bic_block_order(m, r0, r1, order, true, c.perm.data(), pos.data());
        // ---- A_b: the rows in position order, a row's in-block entries by rising column, equal columns summed in stored order
        BlockPattern B;
        B.rp.assign((size_t)rows + 1, 0);
        B.diag_at.resize((size_t)rows);
        B.s.resize((size_t)rows);
        std::vector<std::pair<int32_t, double>> row;
        for (int p = 0; p < rows; ++p) {
            const int i = c.perm[(size_t)r0 + p];
            row.clear();
            for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e)
                if (m->J[e] >= r0 && m->J[e] < r1) row.emplace_back(pos[m->J[e]], m->V[e]);
            std::stable_sort(row.begin(), row.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
            bool has_diag = false;
            double s = 0.0;
            const size_t first = B.cols.size();
            for (size_t q = 0; q < row.size();) {
                double v = row[q].second;
                size_t q1 = q + 1;
                for (; q1 < row.size() && row[q1].first == row[q].first; ++q1) v = v + row[q1].second;
                if (!has_diag && row[q].first > p) {  // no diagonal stored: a zero in its place
                    B.diag_at[p] = (int64_t)B.cols.size();
                    B.cols.push_back(p), B.a.push_back(0.0);
                    has_diag = true;
                }
                if (row[q].first == p) B.diag_at[p] = (int64_t)B.cols.size(), has_diag = true;
                B.cols.push_back(row[q].first), B.a.push_back(v);
                q = q1;
            }
            if (!has_diag) {
                B.diag_at[p] = (int64_t)B.cols.size();
                B.cols.push_back(p), B.a.push_back(0.0);
            }
            for (size_t q = first; q < B.cols.size(); ++q) s = s + std::fabs(B.a[q]);
            B.s[p] = s;
            B.rp[(size_t)p + 1] = (int64_t)B.cols.size();
        }
        // ---- the factor: as it stands, then up the ladder
        std::vector<double> w(B.a.size());
        std::vector<int32_t> where((size_t)rows, -1);
        bool done = factor_block(rows, B, 0.0, w.data(), where.data());
        double alpha = 0.0;
        if (!done) {
            for (int k = -10; k <= 10 && !done; k += 2) {
                alpha = std::ldexp(1.0, k);
                done = factor_block(rows, B, alpha, w.data(), where.data());
            }
            if (done) ++n_shifted;
        }
        BlockFactor& F = parts[b];
        F.lrp.assign((size_t)rows + 1, 0);
        F.urp.assign((size_t)rows + 1, 0);
        F.udinv.resize((size_t)rows);
        if (!done) {  // the Jacobi form: no entries
            ++n_fallback;
            alpha = -1.0;
            for (int p = 0; p < rows; ++p) {
                const double a = B.a[B.diag_at[p]];
                F.udinv[p] = a != 0 && std::isfinite(a) ? 1.0 / a : 1.0;
            }
        } else {
            for (int p = 0; p < rows; ++p) {
                const int64_t di = B.diag_at[p];
                F.lcols.insert(F.lcols.end(), B.cols.begin() + B.rp[p], B.cols.begin() + di);
                F.lvals.insert(F.lvals.end(), w.begin() + B.rp[p], w.begin() + di);
                F.ucols.insert(F.ucols.end(), B.cols.begin() + di + 1, B.cols.begin() + B.rp[p + 1]);
                F.uvals.insert(F.uvals.end(), w.begin() + di + 1, w.begin() + B.rp[p + 1]);
                F.udinv[p] = 1.0 / w[di];
                F.lrp[(size_t)p + 1] = (int64_t)F.lcols.size();
                F.urp[(size_t)p + 1] = (int64_t)F.ucols.size();
            }
        }
        F.shift = alpha;
    }

    // ---- the blocks' pieces behind one another
    c.row_ptr.assign((size_t)n + 1, 0);
    f->u_row_ptr.assign((size_t)n + 1, 0);
    for (int b = 0; b < nb; ++b) {
        const int r0 = c.block_ptr[b], rows = c.block_ptr[b + 1] - r0;
        for (int p = 0; p < rows; ++p) {
            c.row_ptr[(size_t)r0 + p + 1] = c.row_ptr[r0] + parts[b].lrp[(size_t)p + 1];
            f->u_row_ptr[(size_t)r0 + p + 1] = f->u_row_ptr[r0] + parts[b].urp[(size_t)p + 1];
        }
        c.shift[b] = parts[b].shift;
    }
    c.cols.resize((size_t)c.row_ptr[n]);
    c.vals.resize((size_t)c.row_ptr[n]);
    f->u_cols.resize((size_t)f->u_row_ptr[n]);
    f->u_vals.resize((size_t)f->u_row_ptr[n]);
    c.dinv.assign((size_t)n, 1.0);
    f->u_dinv.resize((size_t)n);
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (int b = 0; b < nb; ++b) {
        const int r0 = c.block_ptr[b];
        const BlockFactor& F = parts[b];
        std::copy(F.lcols.begin(), F.lcols.end(), c.cols.begin() + c.row_ptr[r0]);
        std::copy(F.lvals.begin(), F.lvals.end(), c.vals.begin() + c.row_ptr[r0]);
        std::copy(F.ucols.begin(), F.ucols.end(), f->u_cols.begin() + f->u_row_ptr[r0]);
        std::copy(F.uvals.begin(), F.uvals.end(), f->u_vals.begin() + f->u_row_ptr[r0]);
        std::copy(F.udinv.begin(), F.udinv.end(), f->u_dinv.begin() + r0);
    }
    c.counts[0] = nb, c.counts[1] = n_shifted, c.counts[2] = n_fallback;
    compute_levels(f.get());
    *out = f.release();
    return EHYB_OK;
}

extern "C" int ehyb_bilu_create_raw(int n, int nb, const int32_t* block_ptr, const int64_t* l_row_ptr, const int32_t* l_cols, const double* l_vals,
                                    const int64_t* u_row_ptr, const int32_t* u_cols, const double* u_vals, const double* u_dinv, ehyb_bilu** out)
{
    const char* who = "ehyb_bilu_create_raw";
    clear_error();
    if (n < 1 || nb < 1 || !block_ptr || !l_row_ptr || !u_row_ptr || !u_dinv || !out) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (block_ptr[0] != 0 || block_ptr[nb] != n || l_row_ptr[0] != 0 || u_row_ptr[0] != 0)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the blocks do not cover rows 0 .. %d, or a pointer does not start at 0", who, n);
    for (int b = 0; b < nb; ++b) {
        const int64_t rows = (int64_t)block_ptr[b + 1] - block_ptr[b];
        if (rows < 1 || rows > EHYB_BIC_MAX_BLOCK || block_ptr[b] < 0 || block_ptr[b + 1] > n)
            EHYB_FAIL(EHYB_ERR_ARG, "%s: block %d has %lld rows (1 .. %d)", who, b, (long long)rows, EHYB_BIC_MAX_BLOCK);
    }
    for (int i = 0; i < n; ++i)
        if (l_row_ptr[i + 1] < l_row_ptr[i] || u_row_ptr[i + 1] < u_row_ptr[i]) EHYB_FAIL(EHYB_ERR_ARG, "%s: a row pointer falls at row %d", who, i);
    if ((l_row_ptr[n] > 0 && (!l_cols || !l_vals)) || (u_row_ptr[n] > 0 && (!u_cols || !u_vals))) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    for (int b = 0; b < nb; ++b)
        for (int i = block_ptr[b]; i < block_ptr[b + 1]; ++i) {
            const int p = i - block_ptr[b], rows = block_ptr[b + 1] - block_ptr[b];
            for (int64_t e = l_row_ptr[i]; e < l_row_ptr[i + 1]; ++e) {
                if (l_cols[e] < 0 || l_cols[e] >= p)
                    EHYB_FAIL(EHYB_ERR_ARG, "%s: row %d (position %d of block %d) of L holds column %d: not strictly lower, or outside the block", who, i, p, b,
                              l_cols[e]);
                if (e > l_row_ptr[i] && l_cols[e] <= l_cols[e - 1]) EHYB_FAIL(EHYB_ERR_ARG, "%s: the columns of row %d of L do not rise (unsorted)", who, i);
            }
            for (int64_t e = u_row_ptr[i]; e < u_row_ptr[i + 1]; ++e) {
                if (u_cols[e] <= p || u_cols[e] >= rows)
                    EHYB_FAIL(EHYB_ERR_ARG, "%s: row %d (position %d of block %d) of U holds column %d: not strictly upper, or outside the block", who, i, p, b,
                              u_cols[e]);
                if (e > u_row_ptr[i] && u_cols[e] <= u_cols[e - 1]) EHYB_FAIL(EHYB_ERR_ARG, "%s: the columns of row %d of U do not rise (unsorted)", who, i);
            }
        }
    std::unique_ptr<ehyb_bilu> f(new (std::nothrow) ehyb_bilu);
    if (!f) EHYB_FAIL(EHYB_ERR_ALLOC, "%s: out of memory", who);
    ehyb_bic& c = f->core;
    c.n = n, c.nb = nb;
    c.block_ptr.assign(block_ptr, block_ptr + nb + 1);
    for (int b = 0; b < nb; ++b) c.max_block = std::max(c.max_block, block_ptr[b + 1] - block_ptr[b]);
    c.perm.resize((size_t)n);
    std::iota(c.perm.begin(), c.perm.end(), 0);
    c.row_ptr.assign(l_row_ptr, l_row_ptr + n + 1);
    c.cols.assign(l_cols, l_cols + l_row_ptr[n]);
    c.vals.assign(l_vals, l_vals + l_row_ptr[n]);
    c.dinv.assign((size_t)n, 1.0);
    f->u_row_ptr.assign(u_row_ptr, u_row_ptr + n + 1);
    f->u_cols.assign(u_cols, u_cols + u_row_ptr[n]);
    f->u_vals.assign(u_vals, u_vals + u_row_ptr[n]);
    f->u_dinv.assign(u_dinv, u_dinv + n);
    c.shift.assign((size_t)nb, 0.0);
    c.counts[0] = nb;
    compute_levels(f.get());
    *out = f.release();
    return EHYB_OK;
}

extern "C" int ehyb_bilu_host_array(const ehyb_bilu* f, int which, const void** ptr, int64_t* count)
{
    clear_error();
    if (!f || !ptr || !count) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_bilu_host_array: null argument");
    const ehyb_bic& c = f->core;
    switch (which) {
    case EHYB_BILU_BLOCK_PTR: *ptr = c.block_ptr.data(), *count = (int64_t)c.block_ptr.size(); break;
    case EHYB_BILU_PERM: *ptr = c.perm.data(), *count = (int64_t)c.perm.size(); break;
    case EHYB_BILU_L_ROW_PTR: *ptr = c.row_ptr.data(), *count = (int64_t)c.row_ptr.size(); break;
    case EHYB_BILU_L_COLS: *ptr = c.cols.data(), *count = (int64_t)c.cols.size(); break;
    case EHYB_BILU_L_VALS: *ptr = c.vals.data(), *count = (int64_t)c.vals.size(); break;
    case EHYB_BILU_U_ROW_PTR: *ptr = f->u_row_ptr.data(), *count = (int64_t)f->u_row_ptr.size(); break;
    case EHYB_BILU_U_COLS: *ptr = f->u_cols.data(), *count = (int64_t)f->u_cols.size(); break;
    case EHYB_BILU_U_VALS: *ptr = f->u_vals.data(), *count = (int64_t)f->u_vals.size(); break;
    case EHYB_BILU_U_DINV: *ptr = f->u_dinv.data(), *count = (int64_t)f->u_dinv.size(); break;
    case EHYB_BILU_LEVEL_F: *ptr = c.level_f.data(), *count = (int64_t)c.level_f.size(); break;
    case EHYB_BILU_LEVEL_B: *ptr = c.level_b.data(), *count = (int64_t)c.level_b.size(); break;
    case EHYB_BILU_SHIFT: *ptr = c.shift.data(), *count = (int64_t)c.shift.size(); break;
    case EHYB_BILU_COUNTS: *ptr = c.counts, *count = 4; break;
    default: EHYB_FAIL(EHYB_ERR_ARG, "ehyb_bilu_host_array: no array %d", which);
    }
    return EHYB_OK;
}

extern "C" int ehyb_bilu_max_k(const ehyb_bilu* f)
{
    clear_error();
    return f ? ehyb_bic_max_k(&f->core) : 0;
}
