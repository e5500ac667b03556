// The host side of the factorised sparse approximate inverse (ehyb_pcg_fsai): the pattern of G from the lower triangle of the
// reordered matrix, one small dense Cholesky solve per row for its values, G as a matrix on the partitions of A and the plans of
// G and G^T.  No GPU is needed here.  A row of G depends on nothing but the matrix: OpenMP threads share out whole rows, never
// the terms of a sum, and every sum of a row runs in the order include/ehyb.h states, so the result does not depend on the
// number of threads.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "ehyb_internal.h"
#include "fsai.h"

using namespace ehyb;

namespace {

// the calling thread's OpenMP setting, but never more than the CPUs the process owns
int fsai_threads() { return std::max(1, std::min(omp_get_max_threads(), default_host_threads())); }

inline bool positive_finite(double v) { return v > 0 && std::isfinite(v); }

// The columns of row i of G, rising, the diagonal last: the stored columns j < i of row i -- the cap - 1 of largest |a_ij| where
// there are more, ties to the lower column -- and i.  *capped: the row lost columns.  scratch is the caller's.
void select_row(const matrixCOO* m, int i, int cap, std::vector<int32_t>& out, std::vector<std::pair<double, int32_t>>& scratch, bool* capped)
{
    scratch.clear();
    for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e)
        if (m->J[e] >= 0 && m->J[e] < i) scratch.emplace_back(std::fabs(m->V[e]), m->J[e]);
    // a column stored twice counts once, with its first value
    std::stable_sort(scratch.begin(), scratch.end(), [](const auto& a, const auto& b) { return a.second < b.second; });
    scratch.erase(std::unique(scratch.begin(), scratch.end(), [](const auto& a, const auto& b) { return a.second == b.second; }), scratch.end());
    *capped = (int)scratch.size() > cap - 1;
    if (*capped) {
        // (columns rise here: a stable sort by falling magnitude leaves equal magnitudes in rising order; NaN sorts as the smallest)
        std::stable_sort(scratch.begin(), scratch.end(), [](const auto& a, const auto& b) { return a.first > b.first || (a.first == a.first && b.first != b.first); });
        scratch.resize(cap - 1);
        std::sort(scratch.begin(), scratch.end(), [](const auto& a, const auto& b) { return a.second < b.second; });
    }
    out.clear();
    for (const auto& s : scratch) out.push_back(s.second);
    out.push_back(i);
}

// S = the lower triangle of A[J, J], packed by rows: row k takes the stored entries of row J[k] of A whose column is one of
// J[0 .. k]; what is not stored is 0
void assemble(const matrixCOO* m, const int32_t* J, int mm, double* S)
{
    std::fill(S, S + (size_t)mm * (mm + 1) / 2, 0.0);
    for (int k = 0; k < mm; ++k) {
        const int r = J[k];
        double* Sk = S + (size_t)k * (k + 1) / 2;
        for (int e = m->rowIdx[r]; e < m->rowIdx[r + 1]; ++e) {
            const int32_t* at = std::lower_bound(J, J + k + 1, m->J[e]);
            if (at != J + k + 1 && *at == m->J[e]) Sk[at - J] = m->V[e];
        }
    }
}

int check_matrix(const char* who, const matrixCOO* m)
{
    if (!m || !m->rowIdx || !m->J || !m->V || m->dimension < 1) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    return EHYB_OK;
}

}  // namespace

bool ehyb::fsai_row(double* S, int m, double* g)
{
    auto at = [&](int r, int c) -> double& { return S[(size_t)r * (r + 1) / 2 + c]; };
    // S = L L^T, right-looking: column j is scaled by the root of its pivot, then every S[r][c], j < c <= r, loses L[r][j] L[c][j]
    for (int j = 0; j < m; ++j) {
        const double d = at(j, j);
        if (!positive_finite(d)) return false;
        const double ljj = std::sqrt(d);
        at(j, j) = ljj;
        for (int r = j + 1; r < m; ++r) at(r, j) = at(r, j) / ljj;
        for (int r = j + 1; r < m; ++r) {
            const double lrj = at(r, j);
            for (int c = j + 1; c <= r; ++c) at(r, c) = at(r, c) - lrj * at(c, j);
        }
    }
    // L^T g = e_m, from the last unknown up: g[r] = (e[r] - sum over c = m - 1 down to r + 1 of L[c][r] g[c]) / L[r][r]
    for (int r = m - 1; r >= 0; --r) {
        double v = r == m - 1 ? 1.0 : 0.0;
        for (int c = m - 1; c > r; --c) v = v - at(c, r) * g[c];
        g[r] = v / at(r, r);
    }
    return true;
}

extern "C" int ehyb_fsai_create_host(const matrixCOO* m, int row_cap, const ehyb_config* plan_cfg, int transpose_mode, ehyb_fsai** out)
{
    const char* who = "ehyb_fsai_create_host";
    clear_error();
    int rc = check_matrix(who, m);
    if (rc != EHYB_OK) return rc;
    if (!out) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (row_cap > EHYB_FSAI_MAX_ROW) EHYB_FAIL(EHYB_ERR_ARG, "%s: row_cap %d (1 .. %d, <= 0: %d)", who, row_cap, EHYB_FSAI_MAX_ROW, EHYB_FSAI_MAX_ROW);
    if (transpose_mode != 0 && transpose_mode != 1) EHYB_FAIL(EHYB_ERR_ARG, "%s: transpose_mode %d (0 or 1)", who, transpose_mode);
    const int n = m->dimension;
    if (!m->partBoundary || m->nParts < 1 || m->partBoundary[0] != 0 || m->partBoundary[m->nParts] != n)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the matrix has no partition data (call ehyb_matrix_reorder first)", who);
    const int cap = row_cap <= 0 ? EHYB_FSAI_MAX_ROW : row_cap;
    std::unique_ptr<ehyb_fsai, void (*)(ehyb_fsai*)> f(new (std::nothrow) ehyb_fsai, [](ehyb_fsai* p) {
        if (!p) return;
        if (p->plan_g) ehyb_plan_destroy(p->plan_g);
        if (p->plan_t) ehyb_plan_destroy(p->plan_t);
        delete p;
    });
    if (!f) EHYB_FAIL(EHYB_ERR_ALLOC, "%s: out of memory", who);
    f->n = n;
    f->row_cap = cap;
    f->transpose_mode = transpose_mode;
    const int threads = fsai_threads();

    // ---- the pattern: the lengths, their prefix sums, the columns
    f->row_ptr.assign((size_t)n + 1, 0);
    int64_t n_capped = 0;
    int max_row = 0;
#pragma omp parallel num_threads(threads) reduction(+ : n_capped) reduction(max : max_row)
    {
        std::vector<int32_t> J;
        std::vector<std::pair<double, int32_t>> scratch;
#pragma omp for schedule(dynamic, 256)
        for (int i = 0; i < n; ++i) {
            bool capped;
            select_row(m, i, cap, J, scratch, &capped);
            f->row_ptr[(size_t)i + 1] = (int64_t)J.size();
            n_capped += capped;
            max_row = std::max(max_row, (int)J.size());
        }
    }
    for (int i = 0; i < n; ++i) f->row_ptr[(size_t)i + 1] += f->row_ptr[i];
    const int64_t nnz = f->row_ptr[n];
    if (nnz > INT32_MAX) EHYB_FAIL(EHYB_ERR_ARG, "%s: %lld entries in G", who, (long long)nnz);
    f->counts[0] = n_capped;
    f->max_row = max_row;
    f->cols.resize((size_t)nnz);
    f->vals.resize((size_t)nnz);

    // ---- the values, row by row
    int64_t n_fallback = 0;
    int bad_row = n;
#pragma omp parallel num_threads(threads) reduction(+ : n_fallback) reduction(min : bad_row)
    {
        std::vector<int32_t> J;
        std::vector<std::pair<double, int32_t>> scratch;
        std::vector<double> S((size_t)cap * (cap + 1) / 2);
#pragma omp for schedule(dynamic, 256)
        for (int i = 0; i < n; ++i) {
            bool capped;
            select_row(m, i, cap, J, scratch, &capped);
            const int mm = (int)J.size();
            int32_t* Ji = &f->cols[(size_t)f->row_ptr[i]];
            double* g = &f->vals[(size_t)f->row_ptr[i]];
            std::copy(J.begin(), J.end(), Ji);
            assemble(m, Ji, mm, S.data());
            const double aii = S[(size_t)mm * (mm + 1) / 2 - 1];
            if (!positive_finite(aii)) {
                bad_row = std::min(bad_row, i);
                continue;
            }
            if (!fsai_row(S.data(), mm, g)) {  // the Jacobi form of the row
                std::fill(g, g + mm, 0.0);
                g[mm - 1] = 1.0 / std::sqrt(aii);
                ++n_fallback;
            }
        }
    }
    if (bad_row < n)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the matrix is not positive definite (the diagonal entry of row %d is missing or not a positive finite number)", who, bad_row);
    f->counts[1] = n_fallback;

    // ---- G as a matrix on the partitions of A, and its plan(s)
    ehyb_config cfg;
    if (plan_cfg)
        cfg = *plan_cfg;
    else
        ehyb_config_default(&cfg);
    cfg.sym_pairs = 2;
    cfg.value_map = 1;
    std::vector<int> rp((size_t)n + 1);
    for (int i = 0; i <= n; ++i) rp[i] = (int)f->row_ptr[i];
    matrixCOO G;
    memset(&G, 0, sizeof G);
    G.totalNum = (int)nnz;
    G.dimension = n;
    G.maxCol = max_row;
    G.nParts = m->nParts;
    G.vectorCacheSize = m->vectorCacheSize;
    G.kernelPerPart = m->kernelPerPart;
    G.rowIdx = rp.data();
    G.J = f->cols.data();
    G.V = f->vals.data();
    G.partBoundary = m->partBoundary;
    if ((rc = ehyb_plan_create_host(&G, 0, n, &cfg, &f->plan_g)) != EHYB_OK) return rc;
    if (transpose_mode == 1) {
        if ((rc = ehyb_spmv_t_supported(f->plan_g)) != EHYB_OK) {
            const std::string why = ehyb_last_error();
            EHYB_FAIL(rc, "%s: transpose_mode 1: %s", who, why.c_str());
        }
    } else {
        // G^T in CSR form: the rows of G in rising order deal their entries to the columns, so a row of G^T rises too
        std::vector<int> tp((size_t)n + 1, 0);
        for (int64_t k = 0; k < nnz; ++k) ++tp[(size_t)f->cols[k] + 1];
        for (int i = 0; i < n; ++i) tp[i + 1] += tp[i];
        std::vector<int> at(tp.begin(), tp.end() - 1);
        std::vector<int32_t> tcols((size_t)nnz);
        std::vector<double> tvals((size_t)nnz);
        f->order_t.resize((size_t)nnz);
        for (int i = 0; i < n; ++i)
            for (int64_t k = f->row_ptr[i]; k < f->row_ptr[i + 1]; ++k) {
                const int q = at[f->cols[k]]++;
                tcols[q] = i;
                tvals[q] = f->vals[k];
                f->order_t[q] = (int32_t)k;
            }
        G.rowIdx = tp.data();
        G.J = tcols.data();
        G.V = tvals.data();
        if ((rc = ehyb_plan_create_host(&G, 0, n, &cfg, &f->plan_t)) != EHYB_OK) return rc;
    }
    // ---- what the numeric phase on the device reads of A
    f->a_ptr.assign(m->rowIdx, m->rowIdx + n + 1);
    f->a_cols.assign(m->J, m->J + m->rowIdx[n]);
    *out = f.release();
    return EHYB_OK;
}

extern "C" int ehyb_fsai_host_array(const ehyb_fsai* f, int which, const void** ptr, int64_t* count)
{
    clear_error();
    if (!f || !ptr || !count) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_fsai_host_array: null argument");
    switch (which) {
    case EHYB_FSAI_ROW_PTR: *ptr = f->row_ptr.data(), *count = (int64_t)f->row_ptr.size(); break;
    case EHYB_FSAI_COLS: *ptr = f->cols.data(), *count = (int64_t)f->cols.size(); break;
    case EHYB_FSAI_VALS: *ptr = f->vals.data(), *count = (int64_t)f->vals.size(); break;
    case EHYB_FSAI_COUNTS: *ptr = f->counts, *count = 2; break;
    default: EHYB_FAIL(EHYB_ERR_ARG, "ehyb_fsai_host_array: no array %d", which);
    }
    return EHYB_OK;
}

extern "C" int ehyb_fsai_plans(const ehyb_fsai* f, ehyb_plan** plan_g, ehyb_plan** plan_t)
{
    clear_error();
    if (!f || !plan_g || !plan_t) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_fsai_plans: null argument");
    *plan_g = f->plan_g;
    *plan_t = f->plan_t;
    return EHYB_OK;
}
