// Host layout -> the column words and slab records the device holds (col_triples.h states the form).
#include "col_triples.h"

namespace ehyb {
namespace {

// entry i (0 .. 2 np - 1) of group g: the low half of word i / 2 for an even i, the high half for an odd one
inline uint32_t entry_of(const uint32_t* c, uint32_t G, uint32_t g, uint32_t i)
{
    const uint32_t w = c[(size_t)(i >> 1) * G + g];
    return (i & 1) ? w >> 16 : w & 0xffffu;
}

// Are the 2 np entries of every group node triples (or padding) from the front?
bool slab_is_triples(const uint32_t* c, uint32_t np, uint32_t G)
{
    const uint32_t n = 2 * np;
    for (uint32_t g = 0; g < G; ++g) {
        uint32_t i = 0;
        for (; i + 3 <= n; i += 3) {
            const uint32_t a = entry_of(c, G, g, i), b = entry_of(c, G, g, i + 1), d = entry_of(c, G, g, i + 2);
            // (d == a + 2 with equal bits 15: no carry into the flag, so b's flag is theirs too)
            if ((a | b | d) != 0 && !(b == a + 1 && d == a + 2 && ((a ^ d) & 0x8000u) == 0)) return false;
        }
        if (n - i == 2) {
            const uint32_t a = entry_of(c, G, g, i), b = entry_of(c, G, g, i + 1);
            if ((a | b) != 0 && !(b == a + 1 && ((a ^ b) & 0x8000u) == 0)) return false;
        }
    }
    return true;
}

}  // namespace

int64_t device_cols(const HostLayout& H, bool triples, BigVec<uint32_t>* words, std::vector<uint32_t>* meta)
{
    const int64_t nslabs = (int64_t)(H.slab_meta.size() / kSlabWords);
    // One kernel does not decode the form: four columns per pass with symmetric pairs and an inline residual (ell_device.h: it
    // spilled).  A plan that can take it keeps the host's words (ehyb_internal.h: the rule of ehyb_spmm_max_k itself).
    if (plan_keeps_pair_words(H)) triples = false;
    if (!triples || nslabs == 0) {
        if (words) words->assign(H.ell_col.begin(), H.ell_col.end());
        if (meta) *meta = H.slab_meta;
        return (int64_t)H.ell_col.size();
    }
    // slots of the window every slab reads from: its segment's image (own rows from the even row down, then the halo)
    std::vector<int32_t> slots((size_t)nslabs, 0);
    for (size_t g = 0; g + kSegWords <= H.segs.size(); g += kSegWords) {
        const int32_t* sg = &H.segs[g];
        const int32_t n = sg[SEG_WIN_LEN] + (sg[SEG_ROW_BEGIN] & 1) + sg[SEG_HALO_COUNT];
        for (int64_t s = std::max<int64_t>(sg[SEG_SLAB_BEGIN], 0); s < std::min<int64_t>(sg[SEG_SLAB_END], nslabs); ++s) slots[(size_t)s] = n;
    }
    const uint32_t* col = H.ell_col.data();
    // pass 1: which slabs are coded, and the words each takes
    std::vector<uint8_t> coded((size_t)nslabs, 0);
    std::vector<int64_t> first((size_t)nslabs + 1, 0);
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t s = 0; s < nslabs; ++s) {
        const uint32_t* rec = &H.slab_meta[(size_t)s * kSlabWords];
        const SlabShape sh = unpack_slab_shape(rec[SLAB_SHAPE]);
        const int64_t host_words = (int64_t)sh.pairs * sh.groups + (int64_t)sh.er_pairs * 2 * kSlabRows;
        const bool ok = sh.pairs > 0 && sh.er_pairs == 0 && !sh.relative && slots[(size_t)s] >= 3 &&
                        (size_t)rec[SLAB_COL_PTR] + (size_t)host_words <= H.ell_col.size() && slab_is_triples(col + rec[SLAB_COL_PTR], sh.pairs, sh.groups);
        coded[(size_t)s] = ok;
        first[(size_t)s + 1] = ok ? (int64_t)triple_words(sh.pairs) * sh.groups : host_words;
    }
    for (int64_t s = 0; s < nslabs; ++s) first[(size_t)s + 1] += first[(size_t)s];
    const int64_t total = first[(size_t)nslabs];
    if (!words && !meta) return total;
    if (words) words->resize((size_t)total);
    if (meta) *meta = H.slab_meta;
    // pass 2: every word of the device array is written exactly once
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t s = 0; s < nslabs; ++s) {
        const uint32_t* rec = &H.slab_meta[(size_t)s * kSlabWords];
        const SlabShape sh = unpack_slab_shape(rec[SLAB_SHAPE]);
        if (meta) {
            (*meta)[(size_t)s * kSlabWords + SLAB_COL_PTR] = (uint32_t)first[(size_t)s];
            if (coded[(size_t)s]) (*meta)[(size_t)s * kSlabWords + SLAB_SHAPE] |= kSlabTriples;
        }
        if (!words) continue;
        uint32_t* out = words->data() + first[(size_t)s];
        const uint32_t* c = col + rec[SLAB_COL_PTR];
        if (!coded[(size_t)s]) {
            std::copy(c, c + (first[(size_t)s + 1] - first[(size_t)s]), out);
            continue;
        }
        const uint32_t G = sh.groups, n = 2 * sh.pairs, T = (n + 2) / 3, W = triple_words(sh.pairs);
        for (uint32_t j = 0; j < W; ++j)
            for (uint32_t g = 0; g < G; ++g) {
                const uint32_t a = entry_of(c, G, g, 6 * j);                              // (2 j < T whenever j < W)
                const uint32_t b = 2 * j + 1 < T ? entry_of(c, G, g, 6 * j + 3) : 0u;
                out[(size_t)j * G + g] = a | b << 16;
            }
    }
    return total;
}

}  // namespace ehyb
