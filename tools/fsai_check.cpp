// Stand-alone check of the host side of the FSAI preconditioner (csrc/fsai.cpp) for sanitizer builds: its own main, the host
// builder and fsai.cpp, no HIP.  For every case it builds a reordered SPD matrix, the host object (patterns with and without a row
// cap, one plan and two), and holds every row of G to S g = e_m / g_m on the dense block assembled here from the matrix; then
// the fallback of an indefinite block, the refusals, and the same bits on one and three OpenMP threads.
// tools/asan_fsai.sh builds it with -fsanitize=address,undefined and runs it.
#include <omp.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ehyb_internal.h"
#include "fsai.h"

// the symbols of the HIP side that host-only plans and objects need: a plan's destructor (nothing on a device to free), the
// download of a device-built panel form, which no plan here has, and the rule of the transposed multiply (mode 1 asks it)
namespace ehyb {
int materialize_panel_host(ehyb_plan*) { return EHYB_ERR_STATE; }
}
extern "C" void ehyb_plan_destroy(ehyb_plan* p) { delete p; }
extern "C" int ehyb_spmv_t_supported(const ehyb_plan* p) { return p && p->cfg.val_f32 != 1 ? EHYB_OK : EHYB_ERR_ARG; }

namespace {

void destroy(ehyb_fsai* f)
{
    if (!f) return;
    ehyb_plan_destroy(f->plan_g);
    ehyb_plan_destroy(f->plan_t);
    delete f;
}

// SPD on a pattern: a grid of nx x ny points (5-point), or dense diagonal blocks of `block` rows (nx = n, ny = 0);
// off-diagonals -(1 + (i + j) % 3), the diagonal the row's sum of magnitudes + 0.5
int make_matrix(int nx, int ny, int block, const ehyb_config* cfg, matrixCOO* m)
{
    const int n = ny ? nx * ny : nx;
    std::vector<int64_t> rp(1, 0);
    std::vector<int> col;
    std::vector<double> val;
    for (int i = 0; i < n; ++i) {
        std::vector<int> nb;
        if (ny) {
            const int x = i % nx, y = i / nx;
            if (y > 0) nb.push_back(i - nx);
            if (x > 0) nb.push_back(i - 1);
            nb.push_back(i);
            if (x + 1 < nx) nb.push_back(i + 1);
            if (y + 1 < ny) nb.push_back(i + nx);
        } else {
            for (int j = i / block * block; j < std::min(n, (i / block + 1) * block); ++j) nb.push_back(j);
        }
        double sum = 0.5;
        for (int j : nb)
            if (j != i) sum += 1.0 + (i + j) % 3;
        for (int j : nb) col.push_back(j), val.push_back(j == i ? sum : -(1.0 + (i + j) % 3));
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

// every row: the columns rise and end in the diagonal, and || S g - e_m / g_m ||_inf <= 8 m eps ||S||_inf ||g||_inf
int check_rows(const char* name, const matrixCOO* m, const ehyb_fsai* f, int cap)
{
    const double eps = std::ldexp(1.0, -53);
    for (int i = 0; i < f->n; ++i) {
        const int64_t lo = f->row_ptr[i], mm = f->row_ptr[i + 1] - lo;
        if (mm < 1 || mm > cap || f->cols[lo + mm - 1] != i) return printf("%s: row %d has %lld columns\n", name, i, (long long)mm), 1;
        for (int64_t k = 1; k < mm; ++k)
            if (f->cols[lo + k] <= f->cols[lo + k - 1]) return printf("%s: row %d does not rise\n", name, i), 1;
        double s_norm = 0, g_norm = 0, worst = 0;
        for (int64_t r = 0; r < mm; ++r) {
            double sum = 0, mag = 0;
            for (int64_t c = 0; c < mm; ++c) {
                const int a = f->cols[lo + std::max(r, c)], b = f->cols[lo + std::min(r, c)];
                const double s = entry(m, a, b);  // the lower triangle, mirrored
                sum += s * f->vals[lo + c];
                mag += std::fabs(s);
            }
            if (r == mm - 1) sum -= 1.0 / f->vals[lo + mm - 1];
            worst = std::max(worst, std::fabs(sum));
            s_norm = std::max(s_norm, mag);
            g_norm = std::max(g_norm, std::fabs(f->vals[lo + r]));
        }
        if (!(worst <= 8 * mm * eps * s_norm * g_norm)) return printf("%s: row %d misses the bound (%g)\n", name, i, worst), 1;
    }
    return 0;
}

int run_case(const char* name, int nx, int ny, int block, int cap, int mode, int f32)
{
    ehyb_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.lds_doubles = 1024, cfg.sym_pairs = 1, cfg.val_f32 = f32;  // (sym_pairs is forced off for G)
    matrixCOO m;
    memset(&m, 0, sizeof m);
    if (make_matrix(nx, ny, block, &cfg, &m) != EHYB_OK) return printf("%s: matrix failed: %s\n", name, ehyb_last_error()), 1;
    ehyb_fsai *f = nullptr, *f3 = nullptr;
    omp_set_num_threads(1);
    int rc = ehyb_fsai_create_host(&m, cap, &cfg, mode, &f);
    if (mode == 1 && f32) {  // refused with the words of the transposed multiply's rule
        ehyb_matrix_free(&m);
        return rc == EHYB_ERR_ARG && !f ? 0 : (printf("%s: mode 1 with fp32 values was not refused\n", name), 1);
    }
    if (rc != EHYB_OK) return printf("%s: create failed: %s\n", name, ehyb_last_error()), 1;
    omp_set_num_threads(3);
    if (ehyb_fsai_create_host(&m, cap, &cfg, mode, &f3) != EHYB_OK) return printf("%s: second create failed: %s\n", name, ehyb_last_error()), 1;
    int bad = check_rows(name, &m, f, cap <= 0 ? EHYB_FSAI_MAX_ROW : cap);
    if (!bad && (f->row_ptr != f3->row_ptr || f->cols != f3->cols || f->counts[0] != f3->counts[0] ||
                 memcmp(f->vals.data(), f3->vals.data(), f->vals.size() * sizeof(double)) != 0))
        bad = printf("%s: one and three threads differ\n", name);
    if (!bad && ((mode == 0) != (f->plan_t != nullptr) || !f->plan_g || f->plan_g->host.sym)) bad = printf("%s: the plans\n", name);
    ehyb_stats st;
    if (!bad && (ehyb_plan_stats(f->plan_g, &st) != EHYB_OK || st.nnz != (int64_t)f->cols.size())) bad = printf("%s: the plan of G holds %lld entries\n", name, (long long)st.nnz);
    const void* p;
    int64_t cnt;
    if (!bad && (ehyb_fsai_host_array(f, EHYB_FSAI_COUNTS, &p, &cnt) != EHYB_OK || cnt != 2 || ehyb_fsai_host_array(f, 9, &p, &cnt) != EHYB_ERR_ARG)) bad = printf("%s: host_array\n", name);
    printf("%-28s n=%d nnz(G)=%zu longest row %d capped %lld fallback %lld %s\n", name, f->n, f->cols.size(), f->max_row, (long long)f->counts[0],
           (long long)f->counts[1], bad ? "FAILED" : "ok");
    destroy(f);
    destroy(f3);
    ehyb_matrix_free(&m);
    return bad ? 1 : 0;
}

int run_fallback_and_refusals()
{
    ehyb_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.lds_doubles = 1024;
    matrixCOO m;
    memset(&m, 0, sizeof m);
    if (make_matrix(12, 10, 0, &cfg, &m) != EHYB_OK) return 1;
    ehyb_fsai* f = nullptr;
    int bad = 0;
    if (ehyb_fsai_create_host(&m, EHYB_FSAI_MAX_ROW + 1, &cfg, 0, &f) != EHYB_ERR_ARG || f) bad = printf("row_cap 65 was not refused\n");
    if (ehyb_fsai_create_host(nullptr, 0, &cfg, 0, &f) != EHYB_ERR_ARG || ehyb_fsai_create_host(&m, 0, &cfg, 0, nullptr) != EHYB_ERR_ARG) bad = printf("null\n");
    // an off-diagonal pair beyond the diagonal: the block of the later row is indefinite, the row falls back
    int i = -1, at_ij = -1;
    for (int r = m.dimension - 1; r > 0 && i < 0; --r)
        for (int e = m.rowIdx[r]; e < m.rowIdx[r + 1]; ++e)
            if (m.J[e] < r) i = r, at_ij = e;
    const int j = m.J[at_ij];
    const double big = -10.0 * entry(&m, i, i);
    m.V[at_ij] = big;
    for (int e = m.rowIdx[j]; e < m.rowIdx[j + 1]; ++e)
        if (m.J[e] == i) m.V[e] = big;
    if (ehyb_fsai_create_host(&m, 0, &cfg, 0, &f) != EHYB_OK || f->counts[1] != 1) bad = printf("fallback: %s\n", ehyb_last_error());
    if (f) {
        const int64_t lo = f->row_ptr[i], hi = f->row_ptr[i + 1];
        for (int64_t k = lo; k < hi; ++k)
            if (f->vals[k] != (k == hi - 1 ? 1.0 / std::sqrt(entry(&m, i, i)) : 0.0)) bad = printf("fallback row %d, entry %lld\n", i, (long long)(k - lo));
        destroy(f);
        f = nullptr;
    }
    // a diagonal entry that is not positive, and no partition data
    for (int e = m.rowIdx[3]; e < m.rowIdx[4]; ++e)
        if (m.J[e] == 3) m.V[e] = -1.0;
    if (ehyb_fsai_create_host(&m, 0, &cfg, 0, &f) != EHYB_ERR_ARG || f || !strstr(ehyb_last_error(), "not positive definite")) bad = printf("a negative diagonal was not refused\n");
    m.nParts = 0;
    if (ehyb_fsai_create_host(&m, 0, &cfg, 0, &f) != EHYB_ERR_ARG || f || !strstr(ehyb_last_error(), "partition")) bad = printf("no partitions: not refused\n");
    printf("%-28s %s\n", "fallback and refusals", bad ? "FAILED" : "ok");
    ehyb_matrix_free(&m);
    return bad ? 1 : 0;
}

}  // namespace

int main()
{
    int bad = 0;
    bad += run_case("grid 48x40", 48, 40, 0, 0, 0, 0);
    bad += run_case("grid 48x40, cap 2", 48, 40, 0, 2, 0, 0);
    bad += run_case("grid 48x40, one plan", 48, 40, 0, 0, 1, 0);
    bad += run_case("grid 48x40, fp32 values", 48, 40, 0, 0, 0, 1);
    bad += run_case("grid, one plan, fp32", 48, 40, 0, 0, 1, 1);
    bad += run_case("blocks of 96", 192, 0, 96, 0, 0, 0);
    bad += run_case("blocks of 96, cap 8", 192, 0, 96, 8, 0, 0);
    bad += run_case("blocks of 96, cap 1", 192, 0, 96, 1, 1, 0);
    bad += run_case("one row", 1, 0, 1, 0, 0, 0);
    bad += run_fallback_and_refusals();
    printf(bad ? "fsai_check: %d FAILED\n" : "fsai_check: all ok\n", bad);
    return bad ? 1 : 0;
}
