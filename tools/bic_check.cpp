// Stand-alone check of the host side of the block incomplete Cholesky preconditioner (csrc/bic.cpp) for sanitizer builds: its own
// main, the host builder and bic.cpp, no HIP.  It builds reordered SPD matrices and the host object in both orders and for
// several block_rows, holds the factor to L L^T = A_b on its own pattern, compares one and three OpenMP threads bit for bit,
// tries the shift, the fallback and the refusals, and walks the two device streams of bic_build_streams exactly as
// ehyb_bic_apply_kernel does -- thread by thread on the host, every index held against the length of its array -- against a
// plain substitution on dyadic data, where both are exact.  tools/asan_bic.sh builds it with -fsanitize=address,undefined and
// runs it.
#include <omp.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bic.h"
#include "ehyb_internal.h"

// the symbols of the HIP side that host-only plans need (none is reached here)
namespace ehyb {
int materialize_panel_host(ehyb_plan*) { return EHYB_ERR_STATE; }
}
extern "C" void ehyb_plan_destroy(ehyb_plan* p) { delete p; }
extern "C" int ehyb_spmv_t_supported(const ehyb_plan* p) { return p ? EHYB_OK : EHYB_ERR_ARG; }

using namespace ehyb;

namespace {

uint64_t rng_state = 88172645463325252ull;
uint32_t rnd(uint32_t below)
{
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 33) % below);
}

// SPD on a grid of nx x ny points (5-point): off-diagonals -(1 + (i + j) % 3), the diagonal the row's sum of magnitudes + 0.5;
// then `extra`, a dense symmetric block of ne rows, as one more component
int make_matrix(int nx, int ny, const double* extra, int ne, const ehyb_config* cfg, matrixCOO* m)
{
    const int ng = nx * ny, n = ng + ne;
    std::vector<int64_t> rp(1, 0);
    std::vector<int> col;
    std::vector<double> val;
    for (int i = 0; i < ng; ++i) {
        std::vector<int> nb;
        const int x = i % nx, y = i / nx;
        if (y > 0) nb.push_back(i - nx);
        if (x > 0) nb.push_back(i - 1);
        nb.push_back(i);
        if (x + 1 < nx) nb.push_back(i + 1);
        if (y + 1 < ny) nb.push_back(i + nx);
        double sum = 0.5;
        for (int j : nb)
            if (j != i) sum += 1.0 + (i + j) % 3;
        for (int j : nb) col.push_back(j), val.push_back(j == i ? sum : -(1.0 + (i + j) % 3));
        rp.push_back((int64_t)col.size());
    }
    for (int i = 0; i < ne; ++i) {
        for (int j = 0; j < ne; ++j)
            if (extra[i * ne + j] != 0.0) col.push_back(ng + j), val.push_back(extra[i * ne + j]);
        rp.push_back((int64_t)col.size());
    }
    int rc = ehyb_matrix_from_csr(n, rp.data(), col.data(), val.data(), cfg, m);
    if (rc != EHYB_OK) return rc;
    ehyb_config rcfg = *cfg;
    rcfg.part_boundary_cap = n + 1;
    return ehyb_matrix_reorder(m, 1, &rcfg);
}

double entry(const matrixCOO* m, int i, int j)
{
    for (int e = m->rowIdx[i]; e < m->rowIdx[i + 1]; ++e)
        if (m->J[e] == j) return m->V[e];
    return 0.0;
}

// the structure of an object, and (L L^T)_pq = (A_b + alpha diag)_pq on the pattern of L
int check_object(const char* name, const matrixCOO* m, const ehyb_bic* f)
{
    const int n = f->n;
    if ((int)f->block_ptr.size() != f->nb + 1 || f->block_ptr[0] != 0 || f->block_ptr[f->nb] != n) return printf("%s: the blocks\n", name), 1;
    std::vector<char> seen((size_t)n, 0);
    for (int b = 0; b < f->nb; ++b) {
        const int r0 = f->block_ptr[b], r1 = f->block_ptr[b + 1];
        if (r1 <= r0 || r1 - r0 > EHYB_BIC_MAX_BLOCK) return printf("%s: block %d is empty or too long\n", name, b), 1;
        for (int p = r0; p < r1; ++p) {
            const int row = f->perm[p];
            if (row < r0 || row >= r1 || seen[row]++) return printf("%s: PERM leaves block %d\n", name, b), 1;
            const double alpha = f->shift[b];
            if (alpha < 0) continue;  // (a block in its Jacobi form)
            double norm = 0, worst = 0;
            for (int64_t e = f->row_ptr[p]; e <= f->row_ptr[p + 1]; ++e) {  // (the last trip: the diagonal)
                const bool diag = e == f->row_ptr[p + 1];
                const int c = diag ? p - r0 : f->cols[e];
                if (c < 0 || c > p - r0 || (!diag && c == p - r0)) return printf("%s: row %d holds column %d\n", name, p, c), 1;
                if (!diag && e > f->row_ptr[p] && f->cols[e] <= f->cols[e - 1]) return printf("%s: row %d does not rise\n", name, p), 1;
                if (!diag && f->level_f[(size_t)r0 + c] >= f->level_f[p]) return printf("%s: LEVEL_F at row %d\n", name, p), 1;
                if (!diag && f->level_b[(size_t)r0 + c] <= f->level_b[p]) return printf("%s: LEVEL_B at row %d\n", name, p), 1;
                // row p of L times row c of L (both rise): the k present in both
                double sum = 0, mag = 0;
                int64_t ep = f->row_ptr[p], ec = f->row_ptr[(size_t)r0 + c];
                const int64_t end_p = f->row_ptr[p + 1], end_c = f->row_ptr[(size_t)r0 + c + 1];
                while (ep < end_p && ec < end_c) {
                    if (f->cols[ep] == f->cols[ec])
                        sum += f->vals[ep] * f->vals[ec], mag += std::fabs(f->vals[ep] * f->vals[ec]), ++ep, ++ec;
                    else if (f->cols[ep] < f->cols[ec])
                        ++ep;
                    else
                        ++ec;
                }
                const double lcc = 1.0 / f->dinv[(size_t)r0 + c];
                const double lpc = diag ? lcc : f->vals[e];
                sum += lpc * lcc, mag += std::fabs(lpc * lcc);
                double a = entry(m, std::max(row, f->perm[(size_t)r0 + c]), std::min(row, f->perm[(size_t)r0 + c]));
                if (diag) a += alpha * a;
                worst = std::max(worst, std::fabs(sum - a));
                norm = std::max(norm, mag + std::fabs(a));
            }
            if (!(worst <= 64 * std::ldexp(1.0, -53) * norm)) return printf("%s: row %d: L L^T misses A_b by %g\n", name, p, worst), 1;
        }
    }
    return 0;
}

bool same_bits(const ehyb_bic* a, const ehyb_bic* b)
{
    auto eq = [](const auto& x, const auto& y) { return x.size() == y.size() && (x.empty() || memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0); };
    return eq(a->block_ptr, b->block_ptr) && eq(a->perm, b->perm) && eq(a->row_ptr, b->row_ptr) && eq(a->cols, b->cols) && eq(a->vals, b->vals) &&
           eq(a->dinv, b->dinv) && eq(a->level_f, b->level_f) && eq(a->level_b, b->level_b) && eq(a->shift, b->shift) &&
           memcmp(a->counts, b->counts, sizeof a->counts) == 0;
}

// ---- the apply kernel's walk of the streams, on the host: T threads, K = 1
#define HOLD(index, array) \
    if ((size_t)(index) >= (array).size()) return printf("%s: index %lld outside %s (%zu)\n", name, (long long)(index), #array, (array).size()), 1

int walk_streams(const char* name, const ehyb_bic* f, int T, const std::vector<double>& r, std::vector<double>* z)
{
    BicStreams S;
    bic_build_streams(*f, T, &S);
    const int n = f->n;
    if ((int)S.blocks.size() != f->nb || S.meta.size() != (size_t)2 * n || S.dinv.size() != (size_t)2 * n || S.cols.size() != S.vals.size())
        return printf("%s: the sizes of the streams\n", name), 1;
    if (S.real_entries != 2 * (int64_t)f->cols.size()) return printf("%s: %lld entries in the streams\n", name, (long long)S.real_entries), 1;
    std::vector<char> launched((size_t)f->nb, 0);
    std::vector<char> read(S.cols.size(), 0);
    z->assign((size_t)n, NAN);
    for (int wg = 0; wg < f->nb; ++wg) {
        HOLD(wg, S.launch_order);
        const int b = S.launch_order[wg];
        HOLD(b, launched);
        if (launched[b]++) return printf("%s: block %d launched twice\n", name, b), 1;
        const BicBlock B = S.blocks[b];
        const int rows = B.rows;
        if (B.row0 != f->block_ptr[b] || rows != f->block_ptr[b + 1] - B.row0) return printf("%s: the record of block %d\n", name, b), 1;
        std::vector<double> xs((size_t)rows);
        for (int i = 0; i < rows; ++i) {
            HOLD(B.row0 + i, f->perm);
            HOLD(f->perm[B.row0 + i], r);
            xs[i] = r[f->perm[B.row0 + i]];
        }
        for (int dir = 0; dir < 2; ++dir) {
            size_t slot = (size_t)dir * n + B.row0;
            long long ent = B.ent0[dir];
            long long ci = B.cnt0[dir];
            int barriers = 0;
            for (int r = 0; r < B.nround[dir]; ++r) {
                HOLD(B.rnd0[dir] + r, S.rounds);
                const uint32_t word = S.rounds[B.rnd0[dir] + r];
                const int nr = (int)(word & 0x7FF), gl = (int)(word >> 11 & 7), g = 1 << gl, passes = (int)(word >> 15);
                const bool last = (word >> 14 & 1) != 0;
                if (gl > 6 || nr < 1 || (nr << gl) > T) return printf("%s: round word %u\n", name, word), 1;
                std::vector<double> acc((size_t)T, 0.0);
                for (int p = 0; p < passes; ++p) {
                    HOLD(ci + p, S.cnt);
                    const int live = (int)S.cnt[ci + p];
                    if (live < 1 || live > nr) return printf("%s: a pass of %d rows in a round of %d\n", name, live, nr), 1;
                    for (int t = 0; t < T; ++t) {
                        if ((t >> gl) >= live) continue;
                        const long long e = ent + t;
                        HOLD(e, S.cols);
                        if (read[e]++) return printf("%s: entry %lld read twice\n", name, e), 1;
                        HOLD(slot + (t >> gl), S.meta);
                        const int len = (int)(S.meta[slot + (t >> gl)] >> 16), q = p * g + (t & (g - 1));
                        if ((S.cols[e] == kBicNoEntry) != (q >= len)) return printf("%s: entry %lld: padding where the row has an entry, or the reverse\n", name, e), 1;
                        if (S.cols[e] == kBicNoEntry) continue;
                        HOLD(S.cols[e], xs);
                        acc[t] = std::fma(S.vals[e], xs[S.cols[e]], acc[t]);
                    }
                    ent += (long long)live << gl;
                }
                ci += passes;
                for (int off = g >> 1; off > 0; off >>= 1) {
                    std::vector<double> got(acc);
                    for (int t = 0; t < T; ++t) acc[t] = got[t] + got[t ^ off];  // (t ^ off < T: g divides T)
                }
                std::vector<std::pair<int, double>> stores;  // a level's rows read nothing the level writes: order is free
                for (int t = 0; t < T; ++t) {
                    if ((t >> gl) >= nr || (t & (g - 1))) continue;
                    HOLD(slot + (t >> gl), S.meta);
                    const uint32_t mw = S.meta[slot + (t >> gl)];
                    const int row = (int)(mw & 0xFFFF);
                    HOLD(row, xs);
                    if ((int)(mw >> 16) > passes * g) return printf("%s: a row longer than its round's head\n", name), 1;
                    stores.emplace_back(row, (xs[row] - acc[t]) * S.dinv[slot + (t >> gl)]);
                }
                for (const auto& st : stores) xs[st.first] = st.second;
                slot += nr;
                barriers += last;
            }
            if (barriers != B.nlev[dir]) return printf("%s: block %d, direction %d: %d barriers for %d levels\n", name, b, dir, barriers, B.nlev[dir]), 1;
            if (slot != (size_t)dir * n + B.row0 + rows) return printf("%s: block %d, direction %d: %zu rows served\n", name, b, dir, slot), 1;
        }
        for (int i = 0; i < rows; ++i) (*z)[f->perm[B.row0 + i]] = xs[i];
    }
    for (size_t e = 0; e < read.size(); ++e)
        if (!read[e]) return printf("%s: entry %zu never read\n", name, e), 1;
    return 0;
}

// z = P^T (L L^T)^-1 P r by plain substitution
void substitute(const ehyb_bic* f, const std::vector<double>& r, std::vector<double>* z)
{
    const int n = f->n;
    std::vector<double> x((size_t)n);
    for (int p = 0; p < n; ++p) x[p] = r[f->perm[p]];
    for (int b = 0; b < f->nb; ++b) {
        const int r0 = f->block_ptr[b], r1 = f->block_ptr[b + 1];
        for (int p = r0; p < r1; ++p) {
            double s = 0;
            for (int64_t e = f->row_ptr[p]; e < f->row_ptr[p + 1]; ++e) s += f->vals[e] * x[(size_t)r0 + f->cols[e]];
            x[p] = (x[p] - s) * f->dinv[p];
        }
        std::vector<double> sums((size_t)(r1 - r0), 0.0);
        for (int q = r1 - 1; q >= r0; --q) {
            x[q] = (x[q] - sums[q - r0]) * f->dinv[q];
            for (int64_t e = f->row_ptr[q]; e < f->row_ptr[q + 1]; ++e) sums[f->cols[e]] += f->vals[e] * x[q];
        }
    }
    z->assign((size_t)n, 0.0);
    for (int p = 0; p < n; ++p) (*z)[f->perm[p]] = x[p];
}

// a raw dyadic object: blocks of the given lengths; kind 0: rows take up to two columns among the earlier positions q of the
// block with q % 5 < p % 5 (at most five levels); 1: a bidiagonal chain; 2: independent rows and a last row that holds them all
int run_raw(const char* name, const std::vector<int>& lengths, int kind)
{
    std::vector<int32_t> bp(1, 0), cols;
    std::vector<int64_t> rp(1, 0);
    std::vector<double> vals, dinv;
    for (int rows : lengths) {
        for (int p = 0; p < rows; ++p) {
            if (kind == 0) {
                std::vector<int> take;
                for (int tries = 0; tries < 2 && p > 0; ++tries) {
                    const int q = p - 1 - (int)rnd((uint32_t)std::min(p, 40));
                    if (q % 5 < p % 5 && (take.empty() || take[0] != q)) take.push_back(q);
                }
                std::sort(take.begin(), take.end());
                for (int q : take) cols.push_back(q), vals.push_back(rnd(2) ? 1.0 + rnd(2) : -1.0 - rnd(2));
            } else if (kind == 1) {
                if (p > 0) cols.push_back(p - 1), vals.push_back(rnd(2) ? 1.0 : -1.0);
            } else if (p == rows - 1) {
                for (int q = 0; q < p; ++q) cols.push_back(q), vals.push_back(rnd(2) ? 1.0 : -1.0);
            }
            rp.push_back((int64_t)cols.size());
            dinv.push_back(kind == 1 ? 1.0 : std::ldexp(1.0, (int)rnd(3) - 1));
        }
        bp.push_back(bp.back() + rows);
    }
    const int n = bp.back();
    ehyb_bic* f = nullptr;
    if (ehyb_bic_create_raw(n, (int)lengths.size(), bp.data(), rp.data(), cols.data(), vals.data(), dinv.data(), &f) != EHYB_OK)
        return printf("%s: create_raw failed: %s\n", name, ehyb_last_error()), 1;
    std::vector<double> r((size_t)n), want, got;
    for (double& v : r) v = (double)rnd(33) - 16.0;
    substitute(f, r, &want);
    int bad = 0;
    for (int T : {64, 256, 1024, bic_threads(f->max_block)}) {
        if (bad) break;
        bad = walk_streams(name, f, T, r, &got);
        if (!bad && memcmp(want.data(), got.data(), (size_t)n * sizeof(double)) != 0) bad = printf("%s: %d threads: the streams give another z\n", name, T);
    }
    printf("%-44s n=%d blocks=%d levels=%lld max_k=%d %s\n", name, n, f->nb, (long long)f->counts[3], ehyb_bic_max_k(f), bad ? "FAILED" : "ok");
    delete f;
    return bad ? 1 : 0;
}

int run_case(const char* name, int nx, int ny, int block_rows, int order)
{
    ehyb_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.lds_doubles = 1024;
    matrixCOO m;
    memset(&m, 0, sizeof m);
    if (make_matrix(nx, ny, nullptr, 0, &cfg, &m) != EHYB_OK) return printf("%s: matrix failed: %s\n", name, ehyb_last_error()), 1;
    ehyb_bic *f = nullptr, *f3 = nullptr;
    omp_set_num_threads(1);
    if (ehyb_bic_create_host(&m, block_rows, order, &f) != EHYB_OK) return printf("%s: create failed: %s\n", name, ehyb_last_error()), 1;
    omp_set_num_threads(3);
    if (ehyb_bic_create_host(&m, block_rows, order, &f3) != EHYB_OK) return printf("%s: second create failed: %s\n", name, ehyb_last_error()), 1;
    int bad = check_object(name, &m, f);
    if (!bad && !same_bits(f, f3)) bad = printf("%s: one and three threads differ\n", name);
    if (!bad && (f->counts[1] || f->counts[2])) bad = printf("%s: shifted or fallen back\n", name);
    // the streams against the substitution (rounded sums: the two may differ in their last bits)
    std::vector<double> r((size_t)f->n), want, got;
    for (double& v : r) v = (double)rnd(2001) / 1000.0 - 1.0;
    substitute(f, r, &want);
    if (!bad) bad = walk_streams(name, f, bic_threads(f->max_block), r, &got);
    for (int i = 0; i < f->n && !bad; ++i)
        if (!(std::fabs(want[i] - got[i]) <= 1e-9 * (1.0 + std::fabs(want[i])))) bad = printf("%s: z[%d] = %g, the substitution gives %g\n", name, i, got[i], want[i]);
    const void* p;
    int64_t cnt;
    if (!bad && (ehyb_bic_host_array(f, EHYB_BIC_COUNTS, &p, &cnt) != EHYB_OK || cnt != 4 || ehyb_bic_host_array(f, 10, &p, &cnt) != EHYB_ERR_ARG)) bad = printf("%s: host_array\n", name);
    printf("%-44s n=%d blocks=%d nnz(L)=%zu levels=%lld %s\n", name, f->n, f->nb, f->cols.size(), (long long)f->counts[3], bad ? "FAILED" : "ok");
    delete f;
    delete f3;
    ehyb_matrix_free(&m);
    return bad ? 1 : 0;
}

int run_shift_fallback_and_refusals()
{
    ehyb_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.lds_doubles = 1024;
    int bad = 0;
    // Kershaw's matrix: IC(0) in the stored order breaks down, a shift repairs it
    const double kershaw[16] = {3, -2, 0, 2, -2, 3, -2, 0, 0, -2, 3, -2, 2, 0, -2, 3};
    const double beyond[4] = {1, 1e6, 1e6, 1};
    for (int which = 0; which < 2; ++which) {
        matrixCOO m;
        memset(&m, 0, sizeof m);
        if (make_matrix(12, 10, which ? beyond : kershaw, which ? 2 : 4, &cfg, &m) != EHYB_OK) return printf("matrix failed\n"), 1;
        ehyb_bic* f = nullptr;
        if (ehyb_bic_create_host(&m, 0, EHYB_BIC_ORDER_STORED, &f) != EHYB_OK) return printf("create failed: %s\n", ehyb_last_error()), 1;
        if (which == 0 && (f->counts[1] != 1 || f->counts[2] != 0)) bad = printf("Kershaw's block: %lld shifted, %lld fallen back\n", (long long)f->counts[1], (long long)f->counts[2]);
        if (which == 1 && (f->counts[1] != 0 || f->counts[2] != 1)) bad = printf("the block beyond every shift: %lld shifted, %lld fallen back\n", (long long)f->counts[1], (long long)f->counts[2]);
        if (!bad) bad = check_object(which ? "fallback" : "shift", &m, f);
        delete f;
        ehyb_matrix_free(&m);
    }
    matrixCOO m;
    memset(&m, 0, sizeof m);
    if (make_matrix(12, 10, nullptr, 0, &cfg, &m) != EHYB_OK) return 1;
    ehyb_bic* f = nullptr;
    if (ehyb_bic_create_host(nullptr, 0, 0, &f) != EHYB_ERR_ARG || ehyb_bic_create_host(&m, 0, 0, nullptr) != EHYB_ERR_ARG) bad = printf("null\n");
    if (ehyb_bic_create_host(&m, -1, 0, &f) != EHYB_ERR_ARG || f) bad = printf("block_rows -1 was not refused\n");
    if (ehyb_bic_create_host(&m, 0, 2, &f) != EHYB_ERR_ARG || f) bad = printf("order 2 was not refused\n");
    const int keep = m.J[3];
    m.J[3] = m.dimension;
    if (ehyb_bic_create_host(&m, 0, 0, &f) != EHYB_ERR_ARG || f || !strstr(ehyb_last_error(), "outside the matrix")) bad = printf("a column outside the matrix was not refused\n");
    m.J[3] = keep;
    for (int e = m.rowIdx[3]; e < m.rowIdx[4]; ++e)
        if (m.J[e] == 3) m.V[e] = -1.0;
    if (ehyb_bic_create_host(&m, 0, 1, &f) != EHYB_ERR_ARG || f || !strstr(ehyb_last_error(), "not positive definite")) bad = printf("a negative diagonal was not refused\n");
    m.nParts = 0;
    if (ehyb_bic_create_host(&m, 0, 0, &f) != EHYB_ERR_ARG || f || !strstr(ehyb_last_error(), "partition")) bad = printf("no partitions: not refused\n");
    // raw objects: a column on the diagonal, an unsorted row, an empty block
    const int32_t bp[3] = {0, 2, 4}, bp_empty[3] = {0, 4, 4};
    const int64_t rp[5] = {0, 0, 1, 1, 2}, rp2[5] = {0, 0, 0, 0, 2};
    const int32_t good[2] = {0, 0}, diag[2] = {1, 0}, unsorted[2] = {1, 0};
    const double v[2] = {1, 1}, d[4] = {1, 1, 1, 1};
    if (ehyb_bic_create_raw(4, 2, bp, rp, good, v, d, &f) != EHYB_OK) bad = printf("a good raw object was refused: %s\n", ehyb_last_error());
    delete f;
    f = nullptr;
    if (ehyb_bic_create_raw(4, 2, bp, rp, diag, v, d, &f) != EHYB_ERR_ARG || f) bad = printf("a diagonal column was not refused\n");
    const int32_t one[2] = {0, 4};
    if (ehyb_bic_create_raw(4, 1, one, rp2, unsorted, v, d, &f) != EHYB_ERR_ARG || f || !strstr(ehyb_last_error(), "unsorted")) bad = printf("an unsorted row was not refused\n");
    if (ehyb_bic_create_raw(4, 2, bp_empty, rp, good, v, d, &f) != EHYB_ERR_ARG || f) bad = printf("an empty block was not refused\n");
    printf("%-44s %s\n", "shift, fallback and refusals", bad ? "FAILED" : "ok");
    ehyb_matrix_free(&m);
    return bad ? 1 : 0;
}

}  // namespace

int main()
{
    int bad = 0;
    bad += run_case("grid 48x40, stored", 48, 40, 0, EHYB_BIC_ORDER_STORED);
    bad += run_case("grid 48x40, colour", 48, 40, 0, EHYB_BIC_ORDER_COLOUR);
    bad += run_case("grid 48x40, stored, block_rows 64", 48, 40, 64, EHYB_BIC_ORDER_STORED);
    bad += run_case("grid 48x40, colour, block_rows 100", 48, 40, 100, EHYB_BIC_ORDER_COLOUR);
    bad += run_case("grid 48x40, block_rows 1", 48, 40, 1, EHYB_BIC_ORDER_COLOUR);
    bad += run_case("one row", 1, 1, 0, EHYB_BIC_ORDER_STORED);
    bad += run_raw("raw: blocks of 1, 63, 64, 65, 1025", {1, 63, 64, 65, 1025}, 0);
    bad += run_raw("raw: a chain of 300", {300}, 1);
    bad += run_raw("raw: 2500 rows and one that holds them", {7, 2501, 3}, 2);
    bad += run_raw("raw: 5121 rows beside 77", {5121, 77}, 0);
    bad += run_raw("raw: 20480 rows, a chain", {20480}, 1);
    bad += run_shift_fallback_and_refusals();
    printf(bad ? "bic_check: %d FAILED\n" : "bic_check: all ok\n", bad);
    return bad ? 1 : 0;
}
