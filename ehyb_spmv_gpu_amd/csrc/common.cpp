// Error text, configuration defaults, the sizing heuristic and the small vector helpers.
#include "ehyb_internal.h"

#include <sys/mman.h>

#include <omp.h>
#include <sched.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <cmath>

namespace ehyb {

// Threads for the host builder when the caller names none: what OpenMP would take, but no more than
// the CPUs this process may really use -- its affinity mask and its cgroup CPU quota.  A container
// that sees 128 hardware threads and owns 16 ran the pre-step of a 30,000-row matrix in 5.9 s on 128
// OpenMP threads (spinning at every barrier of the multilevel partitioner) against 1 s on 8.
int default_host_threads()
{
    static int cached = 0;
    if (cached > 0) return cached;
    long t = omp_get_max_threads();  // honours OMP_NUM_THREADS
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) t = std::min<long>(t, CPU_COUNT(&set));
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota|max> <period>"
        char quota[32];
        long period = 0;
        if (fscanf(f, "%31s %ld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0)
            t = std::min(t, std::max(1L, (atol(quota) + period - 1) / period));
        fclose(f);
    } else {  // cgroup v1
        long quota = -1, period = 0;
        if (FILE* q = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
            if (fscanf(q, "%ld", &quota) != 1) quota = -1;
            fclose(q);
        }
        if (FILE* q = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (fscanf(q, "%ld", &period) != 1) period = 0;
            fclose(q);
        }
        if (quota > 0 && period > 0) t = std::min(t, std::max(1L, (quota + period - 1) / period));
    }
    cached = (int)std::max(1L, t);
    return cached;
}

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
void clear_error() { g_err[0] = '\0'; }

double wall_seconds()
{
    using namespace std::chrono;
    return duration<double>(steady_clock::now().time_since_epoch()).count();
}

// Fresh pages of a large array that is about to be filled: mapped in by the kernel in one sweep (madvise MADV_POPULATE_WRITE,
// Linux 5.14+) instead of one page-fault trap per 4 KiB on first touch.  Measured on the build container (8 CPUs): filling a fresh
// 620 MB array 0.33 s -> 0.026 s of populate + 0.014 s of fill; the permuted I / J / V of the bench matrix (1.24 GB) were 0.74 s of
// the reorder step, nearly all of it these traps.  (Transparent huge pages were tried first -- MADV_HUGEPAGE -- and made it WORSE,
// 0.74 -> 1.99 s: with defrag = madvise every huge-page fault compacts memory synchronously.)  A hint: an older kernel answers
// EINVAL and the first touch pays as before.
void release_big(void* p, size_t bytes)
{
    if (!p) return;
    if (bytes >= (size_t(64) << 20)) {
        try {
            std::thread(free, p).detach();   // (the helper outlives nothing it needs: free() of a block nobody refers to any more)
            return;
        } catch (...) {
            // no thread to be had: in line, as below
        }
    }
    free(p);
}

void prefault(void* p, size_t bytes)
{
#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif
    if (!p || bytes < (size_t(8) << 20)) return;
    const uintptr_t lo = ((uintptr_t)p + 4095) & ~uintptr_t(4095), hi = ((uintptr_t)p + bytes) & ~uintptr_t(4095);
    if (hi <= lo) return;
    const size_t slice = size_t(16) << 20;
    const int64_t n = (int64_t)((hi - lo + slice - 1) / slice);
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t i = 0; i < n; ++i) {
        const uintptr_t a = lo + (uintptr_t)i * slice, b = std::min<uintptr_t>(hi, a + slice);
        (void)madvise((void*)a, (size_t)(b - a), MADV_POPULATE_WRITE);
    }
}

OmpScope::OmpScope(int want)
{
    const int dflt = default_host_threads();  // reads the caller's setting the first time: before it is changed
    saved = omp_get_max_threads();
    omp_set_num_threads(want > 0 ? want : dflt);
}
OmpScope::~OmpScope() { omp_set_num_threads(saved); }

void device_values_f32(const double* src, size_t n, float* dst)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) dst[i] = (float)src[i];  // cvtsd2ss: nearest-even, +-inf beyond the range, subnormals kept
}

static int round_down(int v, int m) { return v / m * m; }

Config resolve_config(const ehyb_config* in)
{
    ehyb_config z;
    memset(&z, 0, sizeof z);
    if (in) z = *in;
    Config c;
    c.window_mode = z.window_mode == EHYB_WINDOW_REFERENCE ? EHYB_WINDOW_REFERENCE : EHYB_WINDOW_HALO;
    c.n_top = z.n_top > 1 ? z.n_top : 1;
    // Symmetric pair storage: the window also holds one accumulator per own row, so a partition gets
    // at most 30 % of the budget as rows (x: own + halo, y: own), and one workgroup owns a partition.
    // Measured best (tools/sweep.py --sym 1): 256 partitions, one 1024-thread workgroup per CU; two per CU
    // (80 KiB, 512 partitions) is 7 % slower.  One workgroup per CU leaves the whole 160 KiB of LDS to it, so
    // the budget is all of it (until the end of round 2: 112 KiB, which is what 256 partitions of the bench
    // matrix need): matrices that take several rounds of workgroups get fewer, larger partitions -- KKT 110^3
    // 768 -> 511 partitions, 96.6 -> 91.5 us; 200^3 4087 -> 2816, 538 -> 518 us -- and the row-limited
    // partitions of a graded mesh are bisected less often (304 -> 257 items, 107.8 -> 100.5 us); the bench
    // matrix and a 120 k-row one are unchanged (same partitions).
    c.sym_pairs = (z.sym_pairs == 1 && c.window_mode == EHYB_WINDOW_HALO) ? 1 : 2;
    // Plain storage: the whole 160 KiB of a CU as one window, one workgroup per CU, 256 equal-cost work
    // items -- fewer, larger partitions mean fewer halo columns to stage and less padding (audikw_1-like:
    // 136 us against 153 us with two 80 KiB workgroups per CU on the same box; banded +4 %, KKT and
    // R-MAT unchanged).
    c.lds_doubles = z.lds_doubles > 0 ? std::min(z.lds_doubles, EHYB_LDS_MAX_DOUBLES) : EHYB_LDS_MAX_DOUBLES;
    c.lds_doubles = std::max(kSlabRows, round_down(c.lds_doubles, 2));
    // Rows per partition: the whole window in reference mode (convert.c:247 tests against
    // partStart + vectorCacheSize); 55 % of it in halo mode (measured best), the rest holds gathered columns.
    int dflt_rows = c.window_mode == EHYB_WINDOW_REFERENCE ? c.lds_doubles : c.lds_doubles * 11 / 20;
    c.part_rows = z.part_rows > 0 ? std::min(z.part_rows, c.lds_doubles) : dflt_rows;
    c.part_rows = std::max(kSlabRows, round_down(c.part_rows, kSlabRows));
    c.threads = z.threads > 0 ? z.threads : 1024;  // 16 waves per workgroup
    c.threads = std::min(1024, std::max(64, round_down(c.threads, 64)));
    // As many work items per CU as workgroups are resident there (LDS and thread limits): exactly one
    // resident round.  Measured: one or two whole rounds are good, one and a half loses up to 12 %.
    const int resident = std::max(1, std::min(EHYB_LDS_MAX_DOUBLES / c.lds_doubles, 2048 / c.threads));
    c.items_per_cu = z.items_per_cu > 0 ? z.items_per_cu : resident;
    c.partitioner = z.partitioner;
    c.er_seg_len = z.er_seg_len > 0 ? std::max(64, z.er_seg_len) : 4096;
    c.host_threads = z.host_threads > 0 ? z.host_threads : default_host_threads();
    c.verbose = z.verbose;
    c.seed = z.seed;
    c.er_threads = z.er_threads > 0 ? std::min(1024, std::max(64, round_down(z.er_threads, 64))) : 256;
    c.ell_variant = z.ell_variant == 3 ? 3 : 1;
    c.col_sharing = z.col_sharing == 2 ? 2 : 1;
    // residual inside the ELL launch (inline pairs) or as its own launch: 0 = the layout builder decides
    // (inline iff it holds < 0.2 % of the entries and its padded slices < 1 %: layout.cpp)
    c.fuse_er = (z.fuse_er == 1 || z.fuse_er == 2) ? z.fuse_er : 0;
    c.cap_split = z.cap_split == 2 ? 2 : 1;
    c.hub_rule = z.hub_rule == 2 ? 2 : 1;
    c.part_boundary_cap = z.part_boundary_cap > 0 ? z.part_boundary_cap : 0;
    c.er_mode = (z.er_mode == 1 || z.er_mode == 2) ? z.er_mode : 0;
    // default 16,384 columns = 128 KiB of x per panel, one 1024-thread workgroup per CU: with the degree order and the
    // equal-cost items of round 3 the wider panel wins at every size measured (R-MAT 2^24: 544 us against 567-660 us for
    // 8,192 columns, 2^22: 149 against 147 us; fewer partial sums: 46.1 M against 55.2 M).  Round 2's default was 8,192.
    c.er_panel_cols = z.er_panel_cols > 0 ? std::min(16384, std::max(256, round_down(z.er_panel_cols, 64))) : 16384;
    c.er_block_rows = z.er_block_rows > 0 ? std::min(16384, std::max(64, z.er_block_rows)) : 2048;  // measured best on R-MAT 2^22 (1024-4096 level, 8192 25 % slower)
    c.direct = (z.direct == 1 || z.direct == 2) ? z.direct : 0;
    c.ell_prune = z.ell_prune == 2 ? 2 : 1;
    c.value_map = z.value_map == 1 ? 1 : 0;
    c.prune_pct = z.prune_pct > 0 ? z.prune_pct : 110;
    c.er_units1 = z.er_units1 > 0 ? z.er_units1 : 0;  // 0: from the residual's size (er_panel.cpp)
    c.er_units2 = z.er_units2 > 0 ? z.er_units2 : 2048;
    c.graph_compress = (z.graph_compress >= 1 && z.graph_compress <= 3) ? z.graph_compress : 0;
    c.balance = (z.balance == 1 || z.balance == 2) ? z.balance : 0;
    c.req_margin = z.req_margin;
    c.sym_slack_permille = z.sym_slack_permille > 0 ? z.sym_slack_permille : 30;
    c.xcd_map = z.xcd_map == 2 ? 2 : 1;
    c.graphs = z.graphs == 2 ? 2 : 1;
    c.er_sums = z.er_sums == 2 ? 2 : 1;
    c.er_panel_threads = (z.er_panel_threads == 512 || z.er_panel_threads == 1024) ? z.er_panel_threads : 0;
    c.symbolic = z.symbolic == 1 ? 1 : 2;
    c.cg_fused_dot = z.cg_fused_dot == 2 ? 2 : 1;
    c.ell_alternate = (z.ell_alternate == 1 || z.ell_alternate == 2) ? z.ell_alternate : 0;  // 0: by the size of the stream (launch_ell)
    c.row_split = z.row_split > 0 ? z.row_split : 0;
    c.col_map = z.col_map == 2 ? 2 : 1;
    c.er_nt = (z.er_nt == 1 || z.er_nt == 2) ? z.er_nt : 0;
    c.ell_nt = (z.ell_nt >= 1 && z.ell_nt <= 5) ? z.ell_nt : 4;  // 4: a fixed set of slabs stays in the Infinity Cache (ell_keep_rule)
    c.ell_keep = std::min(1000, std::max(0, z.ell_keep));  // 0: by the size of the Infinity Cache (ell_keep_rule)
    c.ell_triples = z.ell_triples == 2 ? 2 : 1;
    c.val_f32 = z.val_f32 == 1 ? 1 : 0;
    c.er_queue = (z.er_queue == 1 || z.er_queue == 2) ? z.er_queue : 0;  // 0: by the number of items per resident workgroup (launch_panel_scale)
    // the automatic choice of the direct shape is for callers that left the window sizing alone: a caller
    // that names a window (lds_doubles / part_rows other than the defaults) gets that window
    if (c.direct == 0 && (c.lds_doubles != EHYB_LDS_MAX_DOUBLES || c.part_rows != round_down(EHYB_LDS_MAX_DOUBLES * 11 / 20, kSlabRows) ||
                          c.window_mode == EHYB_WINDOW_REFERENCE || c.sym_pairs == 1))
        c.direct = 2;
    // symmetric pairs: whole rows may not leave the ELL part (a residual row cannot scatter): no hub rule
    if (c.sym_pairs == 1) {
        c.part_rows = std::max(kSlabRows, std::min(c.part_rows, round_down(c.lds_doubles * 3 / 10, kSlabRows)));
        c.hub_rule = 2;
    }
    return c;
}

}  // namespace ehyb

using namespace ehyb;

extern "C" {

const char* ehyb_last_error(void) { return g_err; }
int ehyb_host_threads(void) { return ehyb::default_host_threads(); }

const char* ehyb_version(void) { return "ehyb-mi355x 0.1.0 gfx950"; }

// Every "0 = default" field of *in replaced by the value the library will use, given the other
// fields (the window and partition sizes depend on window_mode and sym_pairs).  in == NULL: all defaults.
void ehyb_config_resolve(const ehyb_config* in, ehyb_config* out)
{
    if (!out) return;
    const Config c = resolve_config(in);
    ehyb_config r;
    memset(&r, 0, sizeof r);
    r.lds_doubles = c.lds_doubles;
    r.part_rows = c.part_rows;
    r.threads = c.threads;
    r.window_mode = c.window_mode;
    r.items_per_cu = c.items_per_cu;
    r.partitioner = c.partitioner;
    r.er_seg_len = c.er_seg_len;
    r.host_threads = c.host_threads;
    r.verbose = c.verbose;
    r.seed = c.seed;
    r.n_top = c.n_top;
    r.er_threads = c.er_threads;
    r.ell_variant = c.ell_variant;
    r.col_sharing = c.col_sharing;
    r.fuse_er = c.fuse_er;
    r.cap_split = c.cap_split;
    r.hub_rule = c.hub_rule;
    r.sym_pairs = c.sym_pairs;
    r.part_boundary_cap = c.part_boundary_cap;
    r.er_mode = c.er_mode;
    r.er_panel_cols = c.er_panel_cols;
    r.er_block_rows = c.er_block_rows;
    r.direct = c.direct;
    r.ell_prune = c.ell_prune;
    r.value_map = c.value_map;
    r.prune_pct = c.prune_pct;
    r.er_units1 = c.er_units1;
    r.er_units2 = c.er_units2;
    r.graph_compress = c.graph_compress;
    r.balance = c.balance;
    r.req_margin = c.req_margin;
    r.sym_slack_permille = c.sym_slack_permille;
    r.xcd_map = c.xcd_map;
    r.graphs = c.graphs;
    r.er_sums = c.er_sums;
    r.er_panel_threads = c.er_panel_threads;
    r.er_queue = c.er_queue;
    r.symbolic = c.symbolic;
    r.cg_fused_dot = c.cg_fused_dot;
    r.ell_alternate = c.ell_alternate;
    r.row_split = c.row_split;
    r.col_map = c.col_map;
    r.er_nt = c.er_nt;
    r.ell_nt = c.ell_nt;
    r.ell_keep = c.ell_keep;
    r.ell_triples = c.ell_triples;
    r.val_f32 = c.val_f32;
    *out = r;
}

void ehyb_config_default(ehyb_config* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof *cfg);
    Config c = resolve_config(nullptr);
    cfg->lds_doubles = c.lds_doubles;
    cfg->part_rows = c.part_rows;
    cfg->threads = c.threads;
    cfg->window_mode = c.window_mode;
    cfg->items_per_cu = c.items_per_cu;
    cfg->partitioner = EHYB_PART_AUTO;
    cfg->er_seg_len = c.er_seg_len;
    cfg->er_threads = c.er_threads;
    cfg->n_top = 1;
}

// Re-derivation of solver_test.c:53-77 / 158-182 for 256 CUs x 160 KiB LDS:
//   reference: cache = ceil(n/(pf*82*1024))*1024 with the smallest pf whose window fits
//              93 KiB; small matrices get kernelPerPart blocks per partition.
//   here:      the window size is a tuning knob (cfg.part_rows), nParts follows from it
//              with 3 % slack for the partitioner's balance, and kernelPerPart is the
//              number of ELL work items one partition is cut into.
int ehyb_sizing(int dimension, const ehyb_config* cfg, int* nParts, int* vectorCacheSize,
                int* kernelPerPart)
{
    if (dimension <= 0) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_sizing: dimension %d", dimension);
    Config c = resolve_config(cfg);
    int cache = c.part_rows;
    // Plain storage, halo window, default sizing: a matrix of a few hundred thousand rows has fewer
    // full-size partitions than there are work items (256), so several items re-stage the same 160 KiB
    // window.  About 160 partitions are the better trade between restaging and halo columns
    // (round 2 sweep, NOTEBOOK.md 2: us per SpMV with 11,264-row partitions against the best size: 196 k rows
    // 45.3 -> 30.0 at 2048 rows, 393 k rows 65.9 -> 53.2 at 2048, 943 k rows 148.5 -> 136.2 at 5632; from
    // 2.7 M rows on the full-size partitions are as good as any).
    if (c.sym_pairs != 1 && c.window_mode == EHYB_WINDOW_HALO && c.lds_doubles == EHYB_LDS_MAX_DOUBLES &&
        c.part_rows == round_down(EHYB_LDS_MAX_DOUBLES * 11 / 20, kSlabRows)) {
        const int64_t want = ((int64_t)dimension / 160 + kSlabRows - 1) / kSlabRows * kSlabRows;
        cache = (int)std::min<int64_t>(cache, std::max<int64_t>(2048, want));
        // Below ~160 k rows 2048-row partitions are fewer than 80 and every one is cut into three to five work items
        // that stage the same window: about 160 partitions of >= 768 rows there (round 3 sweep, profiles/r03_a_midsize_sweep.jsonl, two
        // generators: KKT 128 k rows 9.0 -> 6.6 us, FEM 120 k rows 22.0 -> 21.2 us; at 195 k rows both are as good or
        // better on the 2048-row partitions -- FEM 30.2 against 34.3 us, KKT 13.8 against 13.4 us -- which stay).
        if ((int64_t)dimension < 80 * (int64_t)cache) {
            const int64_t small = ((int64_t)dimension / 160 + kSlabRows - 1) / kSlabRows * kSlabRows;
            cache = (int)std::min<int64_t>(cache, std::max<int64_t>(768, small));
        }
    }
    // the graph partitioner needs slack to balance; contiguous blocks are cut exactly
    int64_t usable = c.partitioner == EHYB_PART_CONTIGUOUS ? cache : std::max<int64_t>(kSlabRows, (int64_t)(cache * 0.97));
    int64_t parts = (dimension + usable - 1) / usable;
    if (c.n_top > 1) parts = (parts + c.n_top - 1) / c.n_top * c.n_top;
    if (parts < 1) parts = 1;
    if (c.sym_pairs == 1 && parts <= kNumCU / 2) {
        // small matrix, one workgroup per partition: more, smaller partitions (>= 512 rows) keep more CUs busy
        parts = std::max<int64_t>(parts, std::min<int64_t>(kNumCU, dimension / 512));
        cache = (int)std::min<int64_t>(cache, (int64_t)((double)dimension / parts * 1.05) + kSlabRows);
    } else if (c.sym_pairs == 1) {
        // one workgroup per partition, all of equal size: whole rounds of 256 workgroups, and a cap
        // just above the mean so that the partitioner keeps them equal
        parts = (parts + kNumCU - 1) / kNumCU * kNumCU;
        const double slack = c.sym_slack_permille / 1000.0;
        cache = (int)std::min<int64_t>(cache, (int64_t)((double)dimension / parts * (1.0 + slack)) + 2);
    }
    int64_t items = (int64_t)c.items_per_cu * kNumCU;
    int kpp = (int)std::max<int64_t>(1, (items + parts - 1) / parts);
    if (nParts) *nParts = (int)parts;
    if (vectorCacheSize) *vectorCacheSize = cache;
    if (kernelPerPart) *kernelPerPart = std::min(kpp, 32767);
    return EHYB_OK;
}

void ehyb_vector_reorder(int dimension, const double* v_in, double* v_rodr, const int* list)
{
    for (int i = 0; i < dimension; ++i) v_rodr[list[i]] = v_in[i];
}

void ehyb_vector_recover(int dimension, const double* v_rodr, double* v, const int* list)
{
    // The reference inverts the list and scatters (reordering.c:386-391); gathering through
    // the forward list gives the same vector without the temporary.
    for (int i = 0; i < dimension; ++i) v[i] = v_rodr[list[i]];
}

void ehyb_x_glibc(int n, double* x)
{
    for (int i = 0; i < n; ++i) {
        srand((unsigned)i);
        x[i] = (double)(rand() % 200 - 100) / 1000;
    }
}

void ehyb_matrix_free(matrixCOO* m)
{
    if (!m) return;
    free(m->rowIdx);
    free(m->numInRow);
    free(m->numInRow2);
    free(m->I);
    free(m->J);
    free(m->V);
    free(m->diag);
    free(m->partBoundary);
    free(m->reorderList);
    memset(m, 0, sizeof *m);
}

// The eigenpairs of a dense symmetric matrix by cyclic Jacobi (the projected problem of ehyb_eigsh): sweeps over p < q in a fixed
// order, the rotation that annihilates a_pq in Rutishauser's form (t the smaller root, so every angle is at most 45 degrees), an
// entry dropped once it no longer changes either diagonal neighbour in fp64.  No square of an entry is formed -- theta is a
// ratio --, so a matrix scaled by 2^200 or 2^-200 goes through like the unscaled one.  The order of operations is fixed: the same
// input gives the same bits.
int ehyb_sym_eig(int m, const double* T, int ldt, double* evals, double* Y)
{
    clear_error();
    if (m < 1 || m > EHYB_EIGSH_MAX_BASIS + 1 || !T || ldt < m || !evals || !Y)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_sym_eig: bad arguments (m %d, 1 .. %d; ldt %d)", m, EHYB_EIGSH_MAX_BASIS + 1, ldt);
    std::vector<double> A((size_t)m * m), Q((size_t)m * m, 0.0);
    for (int j = 0; j < m; ++j)
        for (int i = 0; i <= j; ++i) {
            const double v = T[(size_t)j * ldt + i];
            if (!std::isfinite(v)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_sym_eig: entry (%d, %d) is not finite", i, j);
            A[(size_t)j * m + i] = A[(size_t)i * m + j] = v;
        }
    for (int i = 0; i < m; ++i) Q[(size_t)i * m + i] = 1.0;
    auto a = [&](int i, int j) -> double& { return A[(size_t)j * m + i]; };
    for (int sweep = 0; sweep < 100; ++sweep) {
        bool rotated = false;
        for (int p = 0; p + 1 < m; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = a(p, q);
                if (apq == 0.0) continue;
                const double app = a(p, p), aqq = a(q, q), g = std::fabs(apq);
                if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
                    a(p, q) = a(q, p) = 0.0;
                    continue;
                }
                const double theta = (aqq - app) / (2.0 * apq), tt = theta * theta;
                const double t = std::isfinite(tt) ? (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(tt + 1.0)) : 0.5 / theta;
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                a(p, p) = app - t * apq;
                a(q, q) = aqq + t * apq;
                a(p, q) = a(q, p) = 0.0;
                for (int k = 0; k < m; ++k) {
                    if (k != p && k != q) {
                        const double akp = a(k, p), akq = a(k, q);
                        a(k, p) = a(p, k) = c * akp - s * akq;
                        a(k, q) = a(q, k) = s * akp + c * akq;
                    }
                    const double qkp = Q[(size_t)p * m + k], qkq = Q[(size_t)q * m + k];
                    Q[(size_t)p * m + k] = c * qkp - s * qkq;
                    Q[(size_t)q * m + k] = s * qkp + c * qkq;
                }
                rotated = true;
            }
        if (!rotated) break;
    }
    std::vector<int> order(m);
    for (int i = 0; i < m; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a(x, x) < a(y, y); });
    for (int i = 0; i < m; ++i) {
        evals[i] = a(order[i], order[i]);
        memcpy(Y + (size_t)i * m, &Q[(size_t)order[i] * m], (size_t)m * sizeof(double));
    }
    return EHYB_OK;
}

// The singular value decomposition of a small dense matrix by one-sided (Hestenes) cyclic Jacobi (the projected problem of
// ehyb_svds): sweeps over the column pairs p < q in a fixed order, each pair rotated until a_p . a_q is at most rows 2^-53 |a_p| |a_q|;
// the rotations accumulate in Y, the column norms are sigma and the normalised columns X.  The matrix itself is rotated, never
// M^T M: a small sigma keeps the digits its column has.  The entries are first scaled by a power of two (exactly) so that the
// largest is near one and no square over- or underflows.  Both factors are polished by one Newton-Schulz step at the end.  A fixed
// sweep limit and a fixed order: the same input gives the same bits.
int ehyb_small_svd(int rows, int cols, const double* M, int ldm, double* sigma, double* X, double* Y)
{
    clear_error();
    constexpr int kMax = EHYB_SVDS_MAX_BASIS + 1;
    if (cols < 1 || rows < cols || rows > kMax || !M || ldm < rows || !sigma || !X || !Y)
        EHYB_FAIL(EHYB_ERR_ARG, "ehyb_small_svd: bad arguments (rows %d, cols %d, 1 <= cols <= rows <= %d; ldm %d)", rows, cols, kMax, ldm);
    std::vector<double> A((size_t)rows * cols), V((size_t)cols * cols, 0.0);
    double big = 0.0;
    for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) {
            const double v = M[(size_t)j * ldm + i];
            if (!std::isfinite(v)) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_small_svd: entry (%d, %d) is not finite", i, j);
            A[(size_t)j * rows + i] = v;
            big = std::max(big, std::fabs(v));
        }
    const int shift = big > 0 ? std::ilogb(big) : 0;
    for (double& v : A) v = std::scalbn(v, -shift);
    for (int i = 0; i < cols; ++i) V[(size_t)i * cols + i] = 1.0;
    auto dot = [&](const double* a, const double* b, int len) {
        double t = 0.0;
        for (int i = 0; i < len; ++i) t += a[i] * b[i];
        return t;
    };
    // the rounding of a_p . a_q itself is of this size: a tighter test would go on rotating noise, and every needless rotation
    // costs Y an ulp of orthogonality -- which a restart of ehyb_svds hands on to the kept vectors
    const double tol = rows * 0x1p-53;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p + 1 < cols; ++p)
            for (int q = p + 1; q < cols; ++q) {
                double *ap = &A[(size_t)p * rows], *aq = &A[(size_t)q * rows];
                const double app = dot(ap, ap, rows), aqq = dot(aq, aq, rows), apq = dot(ap, aq, rows);
                if (apq == 0.0 || std::fabs(apq) <= tol * std::sqrt(app) * std::sqrt(aqq)) continue;
                const double zeta = (aqq - app) / (2.0 * apq);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(zeta * zeta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int i = 0; i < rows; ++i) {
                    const double x = ap[i], y = aq[i];
                    ap[i] = c * x - s * y;
                    aq[i] = s * x + c * y;
                }
                double *vp = &V[(size_t)p * cols], *vq = &V[(size_t)q * cols];
                for (int i = 0; i < cols; ++i) {
                    const double x = vp[i], y = vq[i];
                    vp[i] = c * x - s * y;
                    vq[i] = s * x + c * y;
                }
                rotated = true;
            }
        if (!rotated) break;
    }
    std::vector<double> norm(cols);
    std::vector<int> order(cols);
    for (int j = 0; j < cols; ++j) {
        norm[j] = std::sqrt(dot(&A[(size_t)j * rows], &A[(size_t)j * rows], rows));
        order[j] = j;
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return norm[x] > norm[y]; });
    for (int j = 0; j < cols; ++j) {
        const int o = order[j];
        sigma[j] = std::scalbn(norm[o], shift);
        memcpy(Y + (size_t)j * cols, &V[(size_t)o * cols], (size_t)cols * sizeof(double));
        for (int i = 0; i < rows; ++i) X[(size_t)j * rows + i] = norm[o] > 0 ? A[(size_t)o * rows + i] / norm[o] : 0.0;
    }
    // a zero sigma: the unit vector that the columns set so far leave most of, orthogonalised twice against them
    for (int j = 0; j < cols; ++j) {
        if (sigma[j] > 0) continue;
        std::vector<double> best(rows), e(rows);
        double best_norm = -1.0;
        for (int k = 0; k < rows; ++k) {
            std::fill(e.begin(), e.end(), 0.0);
            e[k] = 1.0;
            for (int pass = 0; pass < 2; ++pass)
                for (int l = 0; l < cols; ++l) {
                    if (l >= j && !(sigma[l] > 0)) continue;  // not set yet (those before j have been completed)
                    const double* xl = X + (size_t)l * rows;
                    const double d = dot(xl, e.data(), rows);
                    for (int i = 0; i < rows; ++i) e[i] -= d * xl[i];
                }
            const double en = std::sqrt(dot(e.data(), e.data(), rows));
            if (en > best_norm) {
                best_norm = en;
                best = e;
            }
        }
        for (int i = 0; i < rows; ++i) X[(size_t)j * rows + i] = best[i] / best_norm;
    }
    // The rotations leave X^T X and Y^T Y off the identity by some rows 2^-52, and a restart of ehyb_svds hands that on to the kept
    // vectors, restart after restart.  One Newton-Schulz step, Z += Z (I - Z^T Z) / 2, moves Z by half its defect -- below what
    // the residuals can see -- to the nearest orthonormal columns, and leaves a defect of a few ulps.
    auto polish = [&](double* Z, int r, int c) {
        std::vector<double> E((size_t)c * c), Zn((size_t)r * c);
        for (int a = 0; a < c; ++a)
            for (int b = 0; b < c; ++b) E[(size_t)b * c + a] = 0.5 * ((a == b ? 1.0 : 0.0) - dot(Z + (size_t)a * r, Z + (size_t)b * r, r));
        for (int b = 0; b < c; ++b)
            for (int i = 0; i < r; ++i) {
                double t = 0.0;
                for (int a = 0; a < c; ++a) t += Z[(size_t)a * r + i] * E[(size_t)b * c + a];
                Zn[(size_t)b * r + i] = Z[(size_t)b * r + i] + t;
            }
        memcpy(Z, Zn.data(), Zn.size() * sizeof(double));
    };
    polish(X, rows, cols);
    polish(Y, cols, cols);
    return EHYB_OK;
}

}  // extern "C"

// C++-linkage names of reordering.h (reference reordering.h:6-10).
#include "reordering.h"
void vectorReorder(const int dimension, const double* v_in, double* v_rodr, const int* rodr_list)
{
    ehyb_vector_reorder(dimension, v_in, v_rodr, rodr_list);
}
void vectorRecover(const int dimension, const double* v_rodr, double* v, const int* rodr_list)
{
    ehyb_vector_recover(dimension, v_rodr, v, rodr_list);
}
// The reference driver sizes nParts / vectorCacheSize for its 82-SM target (solver_test.c:53-77,
// 158-182: audikw_1 -> 164 partitions of <= 6144 rows).  Those are hints here: the partition count is
// re-derived for 256 CUs x 160 KiB of LDS (ehyb_sizing) and written back into the struct, like the
// reference's own reorder step rewrites the arrays it is handed.  matrixReorder is only ever called
// for matrices read from a symmetric file (solver_test.c:369-370), so it sizes the partitions for
// symmetric pair storage (from EHYB_SYM_MIN_ROWS rows up) -- spmvGPuEHYB then recognises them.
// partBoundary: allocated HERE, as the reference's own matrixReorder[_unsym] does (reordering.c:44,234: malloc of
// `dimension` ints over whatever the caller left in the field -- its driver's calloc, solver_test.c:43,144, is simply
// dropped; NULL is legal).  The partition count written back may exceed the caller's nParts, so the caller's own
// array, whatever its size, is never written to.  dimension + 1 ints: room for one partition per row.
static void reorder_dropin(matrixCOO* m, int symmetric, const char* who)
{
    if (!m || m->dimension <= 0) {
        fprintf(stderr, "%s: null or empty matrix\n", who);
        exit(1);
    }
    m->partBoundary = (int*)malloc(sizeof(int) * ((size_t)m->dimension + 1));
    if (!m->partBoundary) {
        fprintf(stderr, "%s: out of memory\n", who);
        exit(1);
    }
    ehyb_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.sym_pairs = (symmetric && m->dimension >= EHYB_SYM_MIN_ROWS) ? 1 : 0;
    cfg.part_boundary_cap = m->dimension + 1;
    int np = 1, cache = 0, kpp = 1;
    int rc = ehyb_sizing(m->dimension, &cfg, &np, &cache, &kpp);
    if (rc == EHYB_OK) {
        m->nParts = std::min(np, m->dimension);
        m->vectorCacheSize = (uint16_t)std::min(cache, 65535);
        m->kernelPerPart = (int16_t)kpp;
        rc = ehyb_matrix_reorder(m, symmetric, &cfg);
    }
    if (rc != EHYB_OK) {
        fprintf(stderr, "%s: %s\n", who, ehyb_last_error());
        exit(1);
    }
}
void matrixReorder(matrixCOO* m) { reorder_dropin(m, 1, "matrixReorder"); }
void matrixReorder_unsym(matrixCOO* m) { reorder_dropin(m, 0, "matrixReorder_unsym"); }
