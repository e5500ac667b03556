// Stand-alone check of the device form of the column words (csrc/col_triples.cpp) for sanitizer builds: its own main, the host
// builder and the transcoder, no HIP.  For every case it builds a host plan, asks for the device arrays (ehyb_plan_device_cols) and
// decodes them slab by slab against EHYB_ARR_ELL_COL with a decoder of its own; a padding triple may read columns 1 and 2 where
// the host form reads 0.  tools/asan_col_triples.sh builds it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ehyb_internal.h"

// the two symbols of the HIP side that a host-only plan needs: its destructor (nothing on a device to free), and the download
// of a device-built panel form, which no plan here has
namespace ehyb {
int materialize_panel_host(ehyb_plan*) { return EHYB_ERR_STATE; }
}
extern "C" void ehyb_plan_destroy(ehyb_plan* p) { delete p; }

namespace {

struct Case {
    const char* name;
    int kind;  // 0 fem3d, 1 banded, 2 rmat, 3 nodes (below)
    int a[7];
    int lds, sym, fuse, direct, triples;
    int parts;       // > 0: partitions the reorder step is asked for, in place of the sizing's own count (and no capacity split)
    int want_inline; // 1: the plan must hold slabs with inline pairs
    int want_coded;  // 1: the plan must hold triple-coded slabs, -1: none
};

// n_nodes nodes of three unknowns: the first half couple to themselves only (3 entries per row: slabs of 2 pairs), the second half
// to the nodes i-1 .. i+2 of their half (12 entries: 6 pairs; 9 at the end: 5 pairs) -- the short slabs no generator gives
int gen_nodes(int n_nodes, const ehyb_config* cfg, matrixCOO* m)
{
    const int half = n_nodes / 2;
    std::vector<int64_t> rp(1, 0);
    std::vector<int> col;
    std::vector<double> val;
    for (int i = 0; i < n_nodes; ++i)
        for (int d = 0; d < 3; ++d) {
            for (int j = (i < half ? i : i - 1); j <= (i < half ? i : i + 2); ++j)
                if (i < half || (j >= half && j < n_nodes))
                    for (int e = 0; e < 3; ++e) col.push_back(3 * j + e), val.push_back(0.5 + (double)((col.size() * 2654435761u) % 1000) / 1000.0);
            rp.push_back((int64_t)col.size());
        }
    return ehyb_matrix_from_csr(3 * n_nodes, rp.data(), col.data(), val.data(), cfg, m);
}

template <class T>
const T* view(const ehyb_plan* p, int which, int64_t* n)
{
    const void* ptr = nullptr;
    if (ehyb_plan_host_array(p, which, &ptr, n) != EHYB_OK) exit(2);
    return static_cast<const T*>(ptr);
}

int check(const Case& c)
{
    ehyb_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.lds_doubles = c.lds, cfg.sym_pairs = c.sym, cfg.fuse_er = c.fuse, cfg.direct = c.direct, cfg.ell_triples = c.triples;
    if (c.parts > 0) cfg.cap_split = 2;
    matrixCOO m;
    memset(&m, 0, sizeof m);
    int rc = c.kind == 0   ? ehyb_gen_fem3d(c.a[0], c.a[1], c.a[2], c.a[3], c.a[4], c.a[5], (uint64_t)c.a[6], &cfg, &m)
             : c.kind == 1 ? ehyb_gen_banded(c.a[0], c.a[1], c.a[2], &cfg, &m)
             : c.kind == 2 ? ehyb_gen_rmat(c.a[0], (int64_t)c.a[1], (uint64_t)c.a[2], &cfg, &m)
                           : gen_nodes(c.a[0], &cfg, &m);
    if (rc != EHYB_OK) return printf("%s: generator failed: %s\n", c.name, ehyb_last_error()), 1;
    ehyb_config rcfg = cfg;
    rcfg.part_boundary_cap = m.dimension + 1;
    if (c.parts > 0) m.nParts = c.parts;
    if (ehyb_matrix_reorder(&m, c.kind == 0 || c.kind == 1, &rcfg) != EHYB_OK) return printf("%s: reorder failed: %s\n", c.name, ehyb_last_error()), 1;
    ehyb_plan* p = nullptr;
    if (ehyb_plan_create_host(&m, 0, m.dimension, &cfg, &p) != EHYB_OK) return printf("%s: plan failed: %s\n", c.name, ehyb_last_error()), 1;
    int64_t n_col = 0, n_meta = 0, n_val = 0, n_lg = 0, n_segs = 0;
    const uint32_t* col = view<uint32_t>(p, EHYB_ARR_ELL_COL, &n_col);
    const uint32_t* meta = view<uint32_t>(p, EHYB_ARR_SLAB_META, &n_meta);
    const double* val = view<double>(p, EHYB_ARR_ELL_VAL, &n_val);
    const uint8_t* lg = view<uint8_t>(p, EHYB_ARR_LANE_GROUP, &n_lg);
    const int32_t* segs = view<int32_t>(p, EHYB_ARR_SEGS, &n_segs);
    const int64_t nslabs = n_meta / 4, n_words = ehyb_plan_device_col_words(p);
    std::vector<uint32_t> words((size_t)n_words + 1), dmeta((size_t)n_meta + 1);
    if (ehyb_plan_device_cols(p, words.data(), dmeta.data()) != EHYB_OK) return printf("%s: device_cols failed\n", c.name), 1;
    std::vector<int64_t> slots((size_t)nslabs, 0);
    for (int64_t g = 0; g + 8 <= n_segs; g += 8)
        for (int64_t s = segs[g + 1]; s < segs[g + 2]; ++s) slots[(size_t)s] = segs[g + 6] + (segs[g + 4] & 1) + segs[g + 3];
    int64_t at = 0, coded = 0, inl = 0, bad = 0;
    for (int64_t s = 0; s < nslabs && !bad; ++s) {
        const uint32_t* h = meta + 4 * s;
        const uint32_t* d = dmeta.data() + 4 * s;
        const uint32_t np = h[3] >> 16, ner = (h[3] >> 8) & 0xff, G = (h[3] & 0x3f) + 1;
        if (d[0] != h[0] || d[2] != h[2] || (d[3] & ~0x40u) != h[3] || d[1] != (uint32_t)at) bad = 1;
        inl += ner > 0;
        if (!(d[3] & 0x40u)) {
            const int64_t hw = (int64_t)np * G + (int64_t)ner * 128;
            if (at + hw > n_words || memcmp(words.data() + at, col + h[1], (size_t)hw * 4) != 0) bad = 2;
            at += hw;
            continue;
        }
        ++coded;
        if (c.triples == 2 || ner != 0 || (h[3] & 0x80u) || slots[(size_t)s] < 3 || np == 0) bad = 3;
        const uint32_t T = (2 * np + 2) / 3, W = (T + 1) / 2;
        if (at + (int64_t)W * G > n_words) bad = 4;
        for (uint32_t lane = 0; lane < 64 && !bad; ++lane) {
            const uint32_t g = lg[64 * s + lane] & 0x3f;
            if (g >= G) bad = 5;
            for (uint32_t i = 0; i < 2 * np && !bad; ++i) {
                const uint32_t hwrd = col[h[1] + (size_t)(i / 2) * G + g], want = (i & 1) ? hwrd >> 16 : hwrd & 0xffff;
                const uint32_t t = i / 3, dw = words[(size_t)at + (size_t)(t / 2) * G + g], got = ((t & 1) ? dw >> 16 : dw & 0xffff) + i % 3;
                const double v = val[((size_t)(h[0] + i / 2) * 64 + lane) * 2 + (i & 1)];
                if (got != want && !(v == 0.0 && want == 0 && got <= 2)) bad = 6;
                if ((int64_t)(got & 0x7fff) >= slots[(size_t)s]) bad = 7;
            }
        }
        at += (int64_t)W * G;
    }
    if (!bad && at != n_words) bad = 8;
    if (!bad && c.triples == 2 && (n_words != n_col || coded != 0)) bad = 9;
    if (!bad && c.want_inline && inl == 0) bad = 10;
    if (!bad && ((c.want_coded > 0 && coded == 0) || (c.want_coded < 0 && coded != 0))) bad = 11;
    printf("%-28s slabs %6lld coded %6lld with inline pairs %4lld words %9lld of %9lld %s\n", c.name, (long long)nslabs, (long long)coded, (long long)inl,
           (long long)n_words, (long long)n_col, bad ? "FAILED" : "ok");
    if (bad) printf("  check %lld failed\n", (long long)bad);
    ehyb_plan_destroy(p);
    ehyb_matrix_free(&m);
    return bad != 0;
}

}  // namespace

int main()
{
    const Case cases[] = {
        {"fem6000 sym", 0, {6000, 3, 12, 12, 20000, 1, 5}, 1024, 1, 0, 0, 0, 0, 0, 1},
        {"fem6000 plain (inline)", 0, {6000, 3, 12, 12, 20000, 1, 5}, 1024, 0, 0, 0, 0, 0, 1, 1},
        {"fem6000 plain own launch", 0, {6000, 3, 12, 12, 20000, 1, 5}, 1024, 0, 2, 0, 0, 0, 0, 1},
        // four columns per pass fit: symmetric pairs with an inline residual keep the pair form whole
        {"fem6000 sym inline", 0, {6000, 3, 12, 12, 20000, 1, 5}, 1024, 1, 1, 0, 0, 0, 1, -1},
        {"fem6000 plain inline", 0, {6000, 3, 12, 12, 20000, 1, 5}, 1024, 0, 1, 0, 0, 0, 1, 1},
        // windows too large for four columns: slabs with inline pairs beside coded ones, symmetric pairs
        {"wide sym inline", 0, {24000, 3, 12, 12, 250000, 1, 5}, 6144, 1, 1, 0, 0, 16, 1, 1},
        {"fem6000 sym, switch off", 0, {6000, 3, 12, 12, 20000, 1, 5}, 1024, 1, 0, 0, 2, 0, 0, -1},
        {"fem24000 sym", 0, {24000, 3, 20, 20, 13500, 1, 4}, 0, 1, 0, 0, 0, 0, 0, 1},
        {"1 unknown per node", 0, {6000, 1, 12, 12, 20000, 1, 5}, 1024, 1, 0, 0, 0, 0, 0, 0},
        {"2 unknowns per node", 0, {6000, 2, 12, 12, 20000, 1, 5}, 1024, 1, 0, 0, 0, 0, 0, 0},
        {"6 unknowns per node", 0, {6000, 6, 12, 12, 20000, 1, 5}, 1024, 1, 0, 0, 0, 0, 0, 1},
        {"6 unknowns per node, plain", 0, {6000, 6, 12, 12, 20000, 1, 5}, 1024, 0, 0, 0, 0, 0, 0, 1},
        {"banded", 1, {1 << 16, 32, 1024}, 0, 0, 0, 2, 0, 0, 0, 0},
        {"rmat", 2, {13, 1 << 16, 2}, 1024, 0, 0, 0, 0, 0, 0, 0},
        {"nodes: 2, 5 and 6 pairs", 3, {2048}, 1024, 0, 0, 2, 0, 0, 0, 1},
    };
    int failed = 0;
    for (const Case& c : cases) failed += check(c);
    printf(failed ? "col_triples_check: %d case(s) FAILED\n" : "col_triples_check: OK\n", failed);
    return failed ? 1 : 0;
}
