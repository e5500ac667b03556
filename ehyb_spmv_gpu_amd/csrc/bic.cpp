// The host side of the block incomplete Cholesky preconditioner (ehyb_pcg_bic): the blocks from the partitions of the reordered
// matrix, the local order of every block (as stored, or by greedy colouring), the IC(0) factor of every diagonal block with the
// shift rule, the levels of the two triangular solves, and the two device streams as host arrays.  No GPU is needed here.  A
// block depends on nothing but the matrix: OpenMP threads share out whole blocks, never the terms of a sum, and every sum runs
// in the order include/ehyb.h states, so the result does not depend on the number of threads.
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>

#include "bic.h"
#include "ehyb_internal.h"

using namespace ehyb;

int ehyb::bic_host_threads() { return std::max(1, std::min(omp_get_max_threads(), default_host_threads())); }

namespace {

inline bool positive_finite(double v) { return v > 0 && std::isfinite(v); }

// L L^T ~ A_b + alpha diag(A_b) on the pattern of one block: rp the block's rows in the object's arrays (entries rp[i] ..
// rp[i + 1] of the object; cols / a / l the block's own), columns rising.  false: a pivot is not a positive finite number.
bool factor_block(int rows, const int64_t* rp, const int32_t* cols, const double* a, const double* adiag, double alpha, double* l, double* ldiag)
{
    const int64_t o = rp[0];  // cols, a and l are the block's own: entry e of the object sits at e - o
    for (int i = 0; i < rows; ++i) {
        for (int64_t e = rp[i] - o; e < rp[i + 1] - o; ++e) {
            const int c = cols[e];
            double s = a[e];
            int64_t ei = rp[i] - o, ec = rp[c] - o;
            const int64_t end_c = rp[c + 1] - o;
            while (ei < e && ec < end_c) {  // the k < c present in both rows, rising
                if (cols[ei] == cols[ec]) {
                    s = s - l[ei] * l[ec];
                    ++ei, ++ec;
                } else if (cols[ei] < cols[ec]) {
                    ++ei;
                } else {
                    ++ec;
                }
            }
            l[e] = s / ldiag[c];
        }
        double d = adiag[i] + alpha * adiag[i];
        for (int64_t e = rp[i] - o; e < rp[i + 1] - o; ++e) d = d - l[e] * l[e];
        if (!positive_finite(d)) return false;
        ldiag[i] = std::sqrt(d);
    }
    return true;
}

// LEVEL_F, LEVEL_B and the most levels of any block, from the pattern
void compute_levels(ehyb_bic* f)
{
    const int n = f->n;
    f->level_f.assign((size_t)n, 0);
    f->level_b.assign((size_t)n, 0);
    int most = 0;
    for (int b = 0; b < f->nb; ++b) {
        const int r0 = f->block_ptr[b], r1 = f->block_ptr[b + 1];
        for (int p = r0; p < r1; ++p) {
            int lv = 0;
            for (int64_t e = f->row_ptr[p]; e < f->row_ptr[p + 1]; ++e) lv = std::max(lv, f->level_f[(size_t)r0 + f->cols[e]] + 1);
            f->level_f[p] = lv;
            most = std::max(most, lv + 1);
        }
        for (int q = r1 - 1; q >= r0; --q) {  // level_b[q] is final: every row behind q has been through
            most = std::max(most, f->level_b[q] + 1);
            for (int64_t e = f->row_ptr[q]; e < f->row_ptr[q + 1]; ++e) {
                int32_t& lp = f->level_b[(size_t)r0 + f->cols[e]];
                lp = std::max(lp, f->level_b[q] + 1);
            }
        }
    }
    f->counts[3] = n ? most : 0;
}

}  // namespace

// ------------------------------------------------------------------ the device streams
int ehyb::bic_threads(int longest_block)
{
    // a quarter of the longest block's rows, in whole waves: the staging loops take four trips, and a level of a coloured block
    // (a third or a quarter of its rows) one or two rounds
    const int want = (longest_block + 3) / 4;
    return std::min(1024, std::max(64, (want + 63) / 64 * 64));
}

int ehyb::bic_group_log2(int threads, int w, int64_t entries)
{
    // the widest power of two g <= 64 with  w g <= threads  (the level in one round: lanes that would idle share rows instead)
    // and  g <= mean row length / 2  (a row then takes at least two passes of its group, so the padding of its last pass is
    // under half of what it streams, and rows of two or three entries keep one lane each)
    if (w < 1 || entries < 1) return 0;
    const int64_t mean = entries / w;
    int gl = 0;
    while (gl < 6 && (int64_t)w << (gl + 1) <= threads && (int64_t)2 << (gl + 1) <= mean) ++gl;
    return gl;
}

// IC: L as stored, L^T -- the rows of L in rising order deal their entries to the columns, so a row of L^T rises too; a block's
// entries of L^T lie where its entries of L do --, 1 / l_ii in both directions
void ehyb::bic_build_streams(const ehyb_bic& f, int threads, BicStreams* out)
{
    const int n = f.n, nb = f.nb;
    std::vector<int64_t> tp((size_t)n + 1, 0);
    std::vector<int32_t> tcols(f.cols.size());
    std::vector<double> tvals(f.vals.size());
#pragma omp parallel for schedule(dynamic, 1) num_threads(bic_host_threads())
    for (int b = 0; b < nb; ++b) {
        const int r0 = f.block_ptr[b], rows = f.block_ptr[b + 1] - r0;
        int64_t* t = &tp[r0];  // t[p + 1]: the length of row p of L^T, then the row's end
        for (int p = 0; p < rows; ++p)
            for (int64_t e = f.row_ptr[(size_t)r0 + p]; e < f.row_ptr[(size_t)r0 + p + 1]; ++e) ++t[(size_t)f.cols[e] + 1];
        std::vector<int64_t> at((size_t)rows);
        int64_t run = f.row_ptr[r0];
        for (int p = 0; p < rows; ++p) {
            at[p] = run;
            run += t[(size_t)p + 1];
            t[(size_t)p + 1] = run;
        }
        for (int p = 0; p < rows; ++p)
            for (int64_t e = f.row_ptr[(size_t)r0 + p]; e < f.row_ptr[(size_t)r0 + p + 1]; ++e) {
                const int64_t q = at[f.cols[e]]++;
                tcols[q] = p;
                tvals[q] = f.vals[e];
            }
    }
    const BicTriangle tri[2] = {{f.row_ptr.data(), f.cols.data(), f.vals.data(), f.dinv.data(), f.level_f.data()},
                                {tp.data(), tcols.data(), tvals.data(), f.dinv.data(), f.level_b.data()}};
    bic_build_streams(n, nb, f.block_ptr.data(), tri, threads, out);
}

void ehyb::bic_build_streams(int n, int nb, const int32_t* block_ptr, const BicTriangle (&tri)[2], int threads, BicStreams* out)
{
    out->threads = threads;
    out->blocks.assign((size_t)nb, BicBlock{});
    out->meta.assign((size_t)2 * n, 0);
    out->dinv.assign((size_t)2 * n, 0.0);
    struct Part {
        std::vector<uint32_t> rounds[2], cnt[2];
        std::vector<uint16_t> cols[2];
        std::vector<double> vals[2];
        int64_t real = 0, cost = 0;
    };
    std::vector<Part> parts((size_t)nb);
#pragma omp parallel for schedule(dynamic, 1) num_threads(bic_host_threads())
    for (int b = 0; b < nb; ++b) {
        const int r0 = block_ptr[b], rows = block_ptr[b + 1] - r0;
        Part& P = parts[b];
        BicBlock& B = out->blocks[b];
        B.row0 = r0, B.rows = rows;
        for (int dir = 0; dir < 2; ++dir) {
            const int64_t* rp = tri[dir].row_ptr + r0;
            const int32_t* cl = tri[dir].cols;
            const double* vl = tri[dir].vals;
            const int32_t* level = tri[dir].level + r0;
            int nlev = 0;
            for (int p = 0; p < rows; ++p) nlev = std::max(nlev, level[p] + 1);
            B.nlev[dir] = nlev;
            // the block's rows by (level, falling length, rising row)
            std::vector<int32_t> ord((size_t)rows);
            std::iota(ord.begin(), ord.end(), 0);
            auto len_of = [&](int p) { return rp[p + 1] - rp[p]; };
            std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) {
                if (level[x] != level[y]) return level[x] < level[y];
                return len_of(x) > len_of(y);
            });
            size_t slot = (size_t)dir * n + r0;
            int at = 0;
            for (int lv = 0; lv < nlev; ++lv) {
                int w = 0;
                int64_t entries = 0;
                while (at + w < rows && level[ord[at + w]] == lv) entries += len_of(ord[at + w]), ++w;
                const int gl = bic_group_log2(threads, w, entries), g = 1 << gl, G = threads >> gl;
                for (int s0 = 0; s0 < w; s0 += G) {
                    const int nr = std::min(G, w - s0);
                    const int64_t longest = len_of(ord[at + s0]);
                    const int64_t passes = (longest + g - 1) >> gl;
                    P.rounds[dir].push_back((uint32_t)nr | (uint32_t)gl << 11 | (uint32_t)(s0 + G >= w ? 1 : 0) << 14 | (uint32_t)passes << 15);
                    for (int64_t pass = 0; pass < passes; ++pass) {
                        int live = 0;  // the rows fall in length: the rows that reach this pass are the first `live`
                        while (live < nr && len_of(ord[at + s0 + live]) > pass * g) ++live;
                        P.cnt[dir].push_back((uint32_t)live);
                        const size_t first = P.cols[dir].size();
                        P.cols[dir].resize(first + (size_t)live * g, kBicNoEntry);
                        P.vals[dir].resize(first + (size_t)live * g, 0.0);
                        for (int r = 0; r < live; ++r) {
                            const int p = ord[at + s0 + r];
                            const int64_t len = len_of(p);
                            for (int64_t q = pass * g; q < std::min(len, (pass + 1) * g); ++q) {
                                P.cols[dir][first + (size_t)r * g + (size_t)(q - pass * g)] = (uint16_t)cl[rp[p] + q];
                                P.vals[dir][first + (size_t)r * g + (size_t)(q - pass * g)] = vl[rp[p] + q];
                                ++P.real;
                            }
                        }
                        P.cost += (live * g + 63) / 64;
                    }
                    P.cost += 2;
                }
                for (int r = 0; r < w; ++r) {
                    const int p = ord[at + r];
                    out->meta[slot + r] = (uint32_t)p | (uint32_t)len_of(p) << 16;
                    out->dinv[slot + r] = tri[dir].dinv[(size_t)r0 + p];
                }
                slot += w, at += w;
                P.cost += 8;  // a barrier, a few waves' worth of passes
            }
        }
        P.cost += rows / 16;
    }
    // ---- the blocks' pieces behind one another, direction 1 behind direction 0 of the same block
    out->real_entries = 0;
    int64_t n_ent = 0;
    for (int b = 0; b < nb; ++b)
        for (int dir = 0; dir < 2; ++dir) n_ent += (int64_t)parts[b].cols[dir].size();
    out->rounds.clear(), out->cnt.clear(), out->cols.clear(), out->vals.clear();
    out->cols.reserve((size_t)n_ent), out->vals.reserve((size_t)n_ent);
    for (int b = 0; b < nb; ++b) {
        Part& P = parts[b];
        for (int dir = 0; dir < 2; ++dir) {
            out->blocks[b].rnd0[dir] = (int32_t)out->rounds.size();
            out->blocks[b].nround[dir] = (int32_t)P.rounds[dir].size();
            out->blocks[b].cnt0[dir] = (int64_t)out->cnt.size();
            out->blocks[b].ent0[dir] = (int64_t)out->cols.size();
            out->rounds.insert(out->rounds.end(), P.rounds[dir].begin(), P.rounds[dir].end());
            out->cnt.insert(out->cnt.end(), P.cnt[dir].begin(), P.cnt[dir].end());
            out->cols.insert(out->cols.end(), P.cols[dir].begin(), P.cols[dir].end());
            out->vals.insert(out->vals.end(), P.vals[dir].begin(), P.vals[dir].end());
        }
        out->real_entries += P.real;
    }
    out->launch_order.resize((size_t)nb);
    std::iota(out->launch_order.begin(), out->launch_order.end(), 0);
    std::stable_sort(out->launch_order.begin(), out->launch_order.end(), [&](int x, int y) { return parts[x].cost > parts[y].cost; });
}

// ------------------------------------------------------------------ the object
// the checks of *_create_host on the matrix, after the null pointers
int ehyb::bic_check_matrix(const char* who, const matrixCOO* m, int block_rows, int order)
{
    if (block_rows < 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: block_rows %d (0: whole partitions)", who, block_rows);
    if (order != EHYB_BIC_ORDER_STORED && order != EHYB_BIC_ORDER_COLOUR) EHYB_FAIL(EHYB_ERR_ARG, "%s: order %d (0 or 1)", who, order);
    const int n = m->dimension;
    if (!m->partBoundary || m->nParts < 1 || m->partBoundary[0] != 0 || m->partBoundary[m->nParts] != n)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the matrix has no partition data (call ehyb_matrix_reorder first)", who);
    for (int p = 0; p < m->nParts; ++p)
        if (m->partBoundary[p + 1] < m->partBoundary[p]) EHYB_FAIL(EHYB_ERR_ARG, "%s: the partition boundaries do not rise", who);
    if (m->rowIdx[0] != 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: the row pointer does not start at 0", who);
    for (int i = 0; i < n; ++i) {
        if (m->rowIdx[i + 1] < m->rowIdx[i]) EHYB_FAIL(EHYB_ERR_ARG, "%s: the row pointer falls at row %d", who, i);
        for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e)
            if (m->J[e] < 0 || m->J[e] >= n) EHYB_FAIL(EHYB_ERR_ARG, "%s: row %d holds column %d, outside the matrix", who, i, m->J[e]);
    }
    return EHYB_OK;
}

// blocks: every partition in ceil(rows / cap) runs of nearly equal length, the first runs one longer
void ehyb::bic_cut_blocks(const matrixCOO* m, int block_rows, ehyb_bic* f)
{
    const int cap = block_rows > 0 ? std::min(block_rows, EHYB_BIC_MAX_BLOCK) : EHYB_BIC_MAX_BLOCK;
    f->block_ptr.assign(1, 0);
    for (int p = 0; p < m->nParts; ++p) {
        const int rows = m->partBoundary[p + 1] - m->partBoundary[p];
        if (rows < 1) continue;
        const int runs = (rows + cap - 1) / cap, base = rows / runs, longer = rows % runs;
        for (int r = 0; r < runs; ++r) f->block_ptr.push_back(f->block_ptr.back() + base + (r < longer ? 1 : 0));
    }
    f->nb = (int)f->block_ptr.size() - 1;
    f->max_block = 0;
    for (int b = 0; b < f->nb; ++b) f->max_block = std::max(f->max_block, f->block_ptr[b + 1] - f->block_ptr[b]);
}

// the local order of the block of rows r0 .. r1 - 1
void ehyb::bic_block_order(const matrixCOO* m, int r0, int r1, int order, bool both_triangles, int32_t* perm, int32_t* pos)
{
    const int rows = r1 - r0;
    if (order == EHYB_BIC_ORDER_STORED) {
        for (int i = r0; i < r1; ++i) perm[i] = i, pos[i] = i - r0;
        return;
    }
    // the block's graph, every edge both ways -- from the lower triangle, or from both (an edge stored in both is then listed
    // twice, which the colouring does not see); rows in rising order take the smallest colour no coloured neighbour holds
    const auto edge = [&](int i, int j) { return j >= r0 && (both_triangles ? j < r1 && j != i : j < i); };
    std::vector<int32_t> deg((size_t)rows + 1, 0);
    for (int i = r0; i < r1; ++i)
        for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e)
            if (edge(i, m->J[e])) ++deg[(size_t)(i - r0) + 1], ++deg[(size_t)(m->J[e] - r0) + 1];
    for (int p = 0; p < rows; ++p) deg[(size_t)p + 1] += deg[p];
    std::vector<int32_t> adj((size_t)deg[rows]), at(deg.begin(), deg.end() - 1);
    for (int i = r0; i < r1; ++i)
        for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e)
            if (edge(i, m->J[e])) adj[at[i - r0]++] = m->J[e] - r0, adj[at[m->J[e] - r0]++] = i - r0;
    // (a row may have more neighbours than the block has rows when edges are listed twice: colours stay below rows all the same)
    std::vector<int32_t> colour((size_t)rows, -1), mark((size_t)rows + 1, -1), count;
    for (int p = 0; p < rows; ++p) {
        for (int e = deg[p]; e < deg[p + 1]; ++e)
            if (colour[adj[e]] >= 0) mark[colour[adj[e]]] = p;
        int c = 0;
        while (mark[c] == p) ++c;
        colour[p] = c;
        if (c >= (int)count.size()) count.resize((size_t)c + 1, 0);
        ++count[c];
    }
    std::vector<int32_t> start(count.size() + 1, 0);
    for (size_t c = 0; c < count.size(); ++c) start[c + 1] = start[c] + count[c];
    for (int p = 0; p < rows; ++p) {  // positions by (colour, row)
        const int to = start[colour[p]]++;
        perm[(size_t)r0 + to] = r0 + p;
        pos[(size_t)r0 + p] = to;
    }
}

extern "C" int ehyb_bic_create_host(const matrixCOO* m, int block_rows, int order, ehyb_bic** out)
{
    const char* who = "ehyb_bic_create_host";
    clear_error();
    if (!m || !m->rowIdx || !m->J || !m->V || m->dimension < 1 || !out) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    const int rc = bic_check_matrix(who, m, block_rows, order);
    if (rc != EHYB_OK) return rc;
    const int n = m->dimension;
    std::unique_ptr<ehyb_bic> f(new (std::nothrow) ehyb_bic);
    if (!f) EHYB_FAIL(EHYB_ERR_ALLOC, "%s: out of memory", who);
    f->n = n;
    f->order = order;
    const int threads = bic_host_threads();
    bic_cut_blocks(m, block_rows, f.get());
    const int nb = f->nb;

    // ---- the local order and the lengths of the rows of tril(A_b) in it
    f->perm.resize((size_t)n);
    std::vector<int32_t> pos((size_t)n);  // block-local position of a row
    f->row_ptr.assign((size_t)n + 1, 0);
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
    for (int b = 0; b < nb; ++b) {
        const int r0 = f->block_ptr[b], r1 = f->block_ptr[b + 1];
        bic_block_order(m, r0, r1, order, false, f->perm.data(), pos.data());
        for (int i = r0; i < r1; ++i)
            for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e)
                if (m->J[e] >= r0 && m->J[e] < i) ++f->row_ptr[(size_t)r0 + std::max(pos[i], pos[m->J[e]]) + 1];
    }
    for (int i = 0; i < n; ++i) f->row_ptr[(size_t)i + 1] += f->row_ptr[i];
    const int64_t nnz = f->row_ptr[n];
    f->cols.resize((size_t)nnz);
    f->vals.resize((size_t)nnz);
    f->dinv.assign((size_t)n, 0.0);
    f->shift.assign((size_t)nb, 0.0);

    // ---- pattern, values of A_b, factor
    int64_t n_shifted = 0, n_fallback = 0;
    int bad_row = n;
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads) reduction(+ : n_shifted, n_fallback) reduction(min : bad_row)
    for (int b = 0; b < nb; ++b) {
        const int r0 = f->block_ptr[b], r1 = f->block_ptr[b + 1], rows = r1 - r0;
        const int64_t* rp = &f->row_ptr[r0];
        const int64_t e0 = rp[0], e1 = rp[rows];
        std::vector<int64_t> at(rp, rp + rows);
        std::vector<double> adiag((size_t)rows, NAN), ldiag((size_t)rows), a((size_t)(e1 - e0));
        for (int i = r0; i < r1; ++i)
            for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e) {
                const int j = m->J[e];
                if (j == i) {
                    if (adiag[pos[i]] != adiag[pos[i]]) adiag[pos[i]] = m->V[e];  // (a column stored twice counts once, with its first value)
                } else if (j >= r0 && j < i) {
                    const int row = std::max(pos[i], pos[j]);
                    const int64_t to = at[row]++;
                    f->cols[to] = std::min(pos[i], pos[j]);
                    a[to - e0] = m->V[e];
                }
            }
        bool bad = false;
        for (int p = 0; p < rows; ++p)
            if (!positive_finite(adiag[p])) bad = true, bad_row = std::min(bad_row, f->perm[(size_t)r0 + p]);
        if (bad) continue;
        // the columns of every row rising (the colour order mixes them; stored order: they rise already)
        std::vector<std::pair<int32_t, double>> row;
        for (int p = 0; p < rows; ++p) {
            const int64_t lo = rp[p], hi = rp[p + 1];
            if (std::is_sorted(f->cols.data() + lo, f->cols.data() + hi)) continue;
            row.clear();
            for (int64_t e = lo; e < hi; ++e) row.emplace_back(f->cols[e], a[e - e0]);
            std::stable_sort(row.begin(), row.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
            for (int64_t e = lo; e < hi; ++e) f->cols[e] = row[e - lo].first, a[e - e0] = row[e - lo].second;
        }
        double* l = f->vals.data() + e0;
        const int32_t* cl = f->cols.data() + e0;
        bool done = factor_block(rows, rp, cl, a.data(), adiag.data(), 0.0, l, ldiag.data());
        double alpha = 0.0;
        if (!done) {
            for (int k = -10; k <= 10 && !done; ++k) {
                alpha = std::ldexp(1.0, k);
                done = factor_block(rows, rp, cl, a.data(), adiag.data(), alpha, l, ldiag.data());
            }
            if (done) ++n_shifted;
        }
        if (!done) {  // the Jacobi form: the pattern stays, its values are zero
            ++n_fallback;
            alpha = -1.0;
            std::fill(l, l + (e1 - e0), 0.0);
            for (int p = 0; p < rows; ++p) ldiag[p] = std::sqrt(adiag[p]);
        }
        f->shift[b] = alpha;
        for (int p = 0; p < rows; ++p) f->dinv[(size_t)r0 + p] = 1.0 / ldiag[p];
    }
    if (bad_row < n)
        EHYB_FAIL(EHYB_ERR_ARG, "%s: the matrix is not positive definite (the diagonal entry of row %d is missing or not a positive finite number)", who, bad_row);
    f->counts[0] = nb, f->counts[1] = n_shifted, f->counts[2] = n_fallback;
    compute_levels(f.get());
    *out = f.release();
    return EHYB_OK;
}

extern "C" int ehyb_bic_create_raw(int n, int nb, const int32_t* block_ptr, const int64_t* row_ptr, const int32_t* cols, const double* vals,
                                   const double* dinv, ehyb_bic** out)
{
    const char* who = "ehyb_bic_create_raw";
    clear_error();
    if (n < 1 || nb < 1 || !block_ptr || !row_ptr || !dinv || !out) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    *out = nullptr;
    if (block_ptr[0] != 0 || block_ptr[nb] != n || row_ptr[0] != 0) EHYB_FAIL(EHYB_ERR_ARG, "%s: the blocks do not cover rows 0 .. %d, or a pointer does not start at 0", who, n);
    for (int b = 0; b < nb; ++b) {
        const int64_t rows = (int64_t)block_ptr[b + 1] - block_ptr[b];
        if (rows < 1 || rows > EHYB_BIC_MAX_BLOCK || block_ptr[b] < 0 || block_ptr[b + 1] > n)
            EHYB_FAIL(EHYB_ERR_ARG, "%s: block %d has %lld rows (1 .. %d)", who, b, (long long)rows, EHYB_BIC_MAX_BLOCK);
    }
    for (int i = 0; i < n; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) EHYB_FAIL(EHYB_ERR_ARG, "%s: the row pointer falls at row %d", who, i);
    if (row_ptr[n] > 0 && (!cols || !vals)) EHYB_FAIL(EHYB_ERR_ARG, "%s: null argument", who);
    for (int b = 0; b < nb; ++b)
        for (int i = block_ptr[b]; i < block_ptr[b + 1]; ++i)
            for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
                if (cols[e] < 0 || cols[e] >= i - block_ptr[b])
                    EHYB_FAIL(EHYB_ERR_ARG, "%s: row %d (position %d of block %d) holds column %d: not strictly lower, or outside the block", who, i,
                              i - block_ptr[b], b, cols[e]);
                if (e > row_ptr[i] && cols[e] <= cols[e - 1]) EHYB_FAIL(EHYB_ERR_ARG, "%s: the columns of row %d do not rise (unsorted)", who, i);
            }
    std::unique_ptr<ehyb_bic> f(new (std::nothrow) ehyb_bic);
    if (!f) EHYB_FAIL(EHYB_ERR_ALLOC, "%s: out of memory", who);
    f->n = n, f->nb = nb;
    f->block_ptr.assign(block_ptr, block_ptr + nb + 1);
    for (int b = 0; b < nb; ++b) f->max_block = std::max(f->max_block, block_ptr[b + 1] - block_ptr[b]);
    f->perm.resize((size_t)n);
    std::iota(f->perm.begin(), f->perm.end(), 0);
    f->row_ptr.assign(row_ptr, row_ptr + n + 1);
    f->cols.assign(cols, cols + row_ptr[n]);
    f->vals.assign(vals, vals + row_ptr[n]);
    f->dinv.assign(dinv, dinv + n);
    f->shift.assign((size_t)nb, 0.0);
    f->counts[0] = nb;
    compute_levels(f.get());
    *out = f.release();
    return EHYB_OK;
}

extern "C" int ehyb_bic_host_array(const ehyb_bic* f, int which, const void** ptr, int64_t* count)
{
    clear_error();
    if (!f || !ptr || !count) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_bic_host_array: null argument");
    switch (which) {
    case EHYB_BIC_BLOCK_PTR: *ptr = f->block_ptr.data(), *count = (int64_t)f->block_ptr.size(); break;
    case EHYB_BIC_PERM: *ptr = f->perm.data(), *count = (int64_t)f->perm.size(); break;
    case EHYB_BIC_ROW_PTR: *ptr = f->row_ptr.data(), *count = (int64_t)f->row_ptr.size(); break;
    case EHYB_BIC_COLS: *ptr = f->cols.data(), *count = (int64_t)f->cols.size(); break;
    case EHYB_BIC_VALS: *ptr = f->vals.data(), *count = (int64_t)f->vals.size(); break;
    case EHYB_BIC_DINV: *ptr = f->dinv.data(), *count = (int64_t)f->dinv.size(); break;
    case EHYB_BIC_LEVEL_F: *ptr = f->level_f.data(), *count = (int64_t)f->level_f.size(); break;
    case EHYB_BIC_LEVEL_B: *ptr = f->level_b.data(), *count = (int64_t)f->level_b.size(); break;
    case EHYB_BIC_SHIFT: *ptr = f->shift.data(), *count = (int64_t)f->shift.size(); break;
    case EHYB_BIC_COUNTS: *ptr = f->counts, *count = 4; break;
    default: EHYB_FAIL(EHYB_ERR_ARG, "ehyb_bic_host_array: no array %d", which);
    }
    return EHYB_OK;
}

extern "C" int ehyb_bic_max_k(const ehyb_bic* f)
{
    clear_error();
    if (!f || f->max_block < 1) return 0;
    return std::min(4, EHYB_BIC_MAX_BLOCK / f->max_block);
}
