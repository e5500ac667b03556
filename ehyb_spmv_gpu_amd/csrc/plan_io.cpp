// On-disk cache of a plan: the permutation and the finished EHYB layout in one file, so that the
// partitioner and the layout builder run once per matrix.  The reference redoes
// mt-metis + COO2EHYB on every run (solver_test.c:369-382, spmv.cu:74); on the bench matrix that
// is seconds of host work in front of a 0.14 ms multiply.
//
// File: "EHYBPLN9", key, resolved Config, layout scalars, stats, the permutation, then every array as
// {u64 count, bytes}, then "EHYBEND4".  Native byte order, same-machine cache -- not an
// interchange format.  A file whose magic, version, key or sizes do not fit is rejected, and so is one
// whose arrays would make a kernel or a host routine index outside an array (ehyb_plan_check below).
#include "ehyb_internal.h"

#include <climits>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <memory>
#include <new>
#include <type_traits>

using namespace ehyb;

namespace {

const char kMagic[8] = {'E', 'H', 'Y', 'B', 'P', 'L', 'N', '9'};
const char kEnd[8] = {'E', 'H', 'Y', 'B', 'E', 'N', 'D', '4'};

struct FileCloser {
    void operator()(FILE* f) const
    {
        if (f) fclose(f);
    }
};
using File = std::unique_ptr<FILE, FileCloser>;

template <class T>
bool put(FILE* f, const T& v)
{
    static_assert(std::is_trivially_copyable<T>::value, "raw write");
    return fwrite(&v, sizeof(T), 1, f) == 1;
}
template <class T>
bool get(FILE* f, T& v)
{
    return fread(&v, sizeof(T), 1, f) == 1;
}
// The configuration as the files hold it: the fields up to ell_nt.  Knobs added since (ell_keep: how a launch reads; ell_triples:
// the form of the column words on the device; nothing of the host layout) stay out, so that files written before them remain
// valid; a loaded plan has them at their defaults.  (val_f32, the form of the values on the device, travels in the spare word of
// the scalars, which files written before it hold as 0 = off.)
constexpr size_t kCfgFileBytes = offsetof(Config, ell_keep);
static_assert(kCfgFileBytes + 3 * sizeof(int) == sizeof(Config), "fields added to Config go behind ell_keep and stay out of plan files");
bool put_cfg(FILE* f, const Config& c) { return fwrite(&c, kCfgFileBytes, 1, f) == 1; }
bool get_cfg(FILE* f, Config& c)
{
    c.ell_keep = 0;
    c.ell_triples = resolve_config(nullptr).ell_triples;
    c.val_f32 = 0;
    return fread(&c, kCfgFileBytes, 1, f) == 1;
}
template <class T, class A>
bool put_vec(FILE* f, const std::vector<T, A>& v)
{
    const uint64_t n = v.size();
    return put(f, n) && (n == 0 || fwrite(v.data(), sizeof(T), n, f) == n);
}
template <class T, class A>
bool get_vec(FILE* f, std::vector<T, A>& v, uint64_t limit)
{
    uint64_t n = 0;
    if (!get(f, n) || n > limit) return false;
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

// Every array of the layout, in file order.
template <class F>
bool each_array(HostLayout& H, F&& io)
{
    return io(H.part_boundary) && io(H.win_len) && io(H.halo_ptr) && io(H.halo_cols) && io(H.slab_pair_ptr) &&
           io(H.slab_row) && io(H.slab_part) && io(H.ell_val) && io(H.ell_col) && io(H.slab_col_ptr) && io(H.lane_group) &&
           io(H.slab_meta) && io(H.items) && io(H.segs) && io(H.er_seg_ptr) && io(H.er_seg_row) && io(H.er_col) &&
           io(H.er_val) && io(H.er_blocks) && io(H.slab_lrow) && io(H.pb_val) && io(H.pb_col) && io(H.pb_dst) &&
           io(H.pb_units1) && io(H.pb_row) && io(H.pb_units2) && io(H.col_seg_first) && io(H.pb_seg_item) && io(H.pb_items1);
}

struct Scalars {
    int32_t n_cols, row_begin, row_end, n_parts, lds_doubles, inline_er;
    int32_t er_bins[8];
    int32_t sym, yacc_doubles;
    int32_t er_panel, pb_panel_cols, pb_rows_max, direct;
    int64_t pb_partials, pb_bytes;
    int32_t pb_assign, val_f32;
};

// The panel residual's arrays must fit together as the two kernels index them.
bool panel_consistent(const HostLayout& H)
{
    if (!H.er_panel)
        return H.pb_val.empty() && H.pb_col.empty() && H.pb_dst.empty() && H.pb_units1.empty() && H.pb_row.empty() && H.pb_units2.empty();
    const size_t ne = H.pb_val.size();
    if (H.pb_col.size() != ne || H.pb_dst.size() != ne || ne % 64 != 0 || H.pb_units1.size() % 4 || H.pb_units2.size() % 4) return false;
    if (H.pb_partials < 0 || H.pb_row.size() != (size_t)H.pb_partials) return false;
    if (H.pb_panel_cols < 64 || H.pb_panel_cols > 16384 || H.pb_rows_max < 1 || H.pb_rows_max > 16384) return false;
    if (H.pb_items1.size() % 2) return false;
    for (size_t i = 0; i < H.pb_items1.size(); i += 2)  // the items are consecutive runs of the unit list, all of it
        if (H.pb_items1[i] != (i ? H.pb_items1[i - 1] : 0) || H.pb_items1[i + 1] <= H.pb_items1[i] || (size_t)H.pb_items1[i + 1] > H.pb_units1.size() / 4) return false;
    if (!H.pb_items1.empty() && (size_t)H.pb_items1.back() != H.pb_units1.size() / 4) return false;
    if (H.pb_items1.empty() != H.pb_units1.empty()) return false;
    if (!H.pb_seg_item.empty() && (H.pb_seg_item.size() != H.col_seg_first.size() + (H.col_seg_first.empty() ? 2 : 0) || H.pb_seg_item.front() != 0 || (size_t)H.pb_seg_item.back() != H.pb_items1.size() / 2)) return false;
    for (size_t u = 0; u < H.pb_units1.size(); u += 4) {
        const int32_t* q = &H.pb_units1[u];
        if (q[0] < 0 || q[1] < 1 || q[1] > H.pb_panel_cols || (int64_t)q[0] + q[1] > H.n_cols || q[2] < 0 || q[3] < q[2] || (size_t)q[3] > ne ||
            q[2] % 64 || q[3] % 64)
            return false;
    }
    for (size_t u = 0; u < H.pb_units2.size(); u += 4) {
        const int32_t* q = &H.pb_units2[u];
        const int32_t rows = q[3] < 0 ? -q[3] : q[3];  // negative: the block assigns y (pb_assign)
        if (q[0] < 0 || q[1] < q[0] || q[1] > H.pb_partials || q[2] < H.row_begin || rows < 1 || rows > H.pb_rows_max || q[2] + rows > H.row_end) return false;
        if (q[3] < 0 && !H.pb_assign) return false;
    }
    for (uint32_t d : H.pb_dst)
        if (d != 0xFFFFFFFFu && d >= (uint64_t)H.pb_partials) return false;
    for (uint16_t c : H.pb_col)
        if (c >= H.pb_panel_cols) return false;  // bits 14 and 15 of the streamed column word are flags
    return true;
}

// ---------------------------------------------------------------- the content check (ehyb_plan_check)
// Every index a kernel (ell_device.h, ell_t_device.h, panel_device.h, the residual kernels) or a host routine (device_cols,
// encode_panel_slots, ehyb_plan_resident_bytes, ehyb_plan_tune's cost model) forms from the arrays lies inside the array it
// indexes.  The first rule that fails is reported with its array and index.  Values may hold any bits.
struct Why {
    char text[384] = "";
    bool say(const char* fmt, ...) __attribute__((format(printf, 2, 3)))
    {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof text, fmt, ap);
        va_end(ap);
        return false;
    }
};
// (a rule inside a parallel pass is evaluated without a message first: why == null)
#define RULE(ok, ...)                          \
    do {                                       \
        if (!(ok)) {                           \
            if (why) why->say(__VA_ARGS__);    \
            return false;                      \
        }                                      \
    } while (0)

// The first index of [0, n) that `ok(i, nullptr)` refuses, found on all host threads; its message from a second call.
template <class F>
bool all_of_parallel(int64_t n, Why* why, F&& ok)
{
    int64_t first = INT64_MAX;
#pragma omp parallel for schedule(dynamic, 256) reduction(min : first)
    for (int64_t i = 0; i < n; ++i)
        if (i < first && !ok(i, (Why*)nullptr)) first = i;
    if (first == INT64_MAX) return true;
    return ok(first, why);
}

// lengths: everything below indexes on their strength
bool sizes_fit(const HostLayout& H, size_t perm_size, Why* why)
{
    const size_t nslab = H.slab_row.size(), nseg = H.er_seg_row.size();
    RULE(H.n_cols > 0 && H.row_begin >= 0 && H.row_begin < H.row_end && H.row_end <= H.n_cols, "scalars: rows [%d, %d) of %d columns", H.row_begin, H.row_end,
         H.n_cols);
    RULE(H.n_parts >= 1 && H.part_boundary.size() == (size_t)H.n_parts + 1, "part_boundary: %zu entries for %d partitions", H.part_boundary.size(), H.n_parts);
    RULE(H.win_len.size() == (size_t)H.n_parts, "win_len: %zu entries for %d partitions", H.win_len.size(), H.n_parts);
    RULE(H.halo_ptr.size() == (size_t)H.n_parts + 1, "halo_ptr: %zu entries for %d partitions", H.halo_ptr.size(), H.n_parts);
    RULE(H.halo_ptr.back() >= 0 && H.halo_cols.size() == (size_t)H.halo_ptr.back(), "halo_ptr[%d] = %d: halo_cols holds %zu", H.n_parts, H.halo_ptr.back(),
         H.halo_cols.size());
    RULE(H.slab_pair_ptr.size() == nslab + 1 && H.slab_col_ptr.size() == nslab + 1 && H.slab_part.size() == nslab,
         "slab_pair_ptr / slab_col_ptr / slab_part: %zu / %zu / %zu entries for %zu slabs (slab_row)", H.slab_pair_ptr.size(), H.slab_col_ptr.size(),
         H.slab_part.size(), nslab);
    RULE(H.slab_meta.size() == nslab * kSlabWords && H.lane_group.size() == nslab * kSlabRows, "slab_meta / lane_group: %zu / %zu entries for %zu slabs",
         H.slab_meta.size(), H.lane_group.size(), nslab);
    RULE(H.ell_val.size() == (size_t)H.slab_pair_ptr.back() * 2 * kSlabRows, "slab_pair_ptr[%zu] = %u pairs: ell_val holds %zu", nslab, H.slab_pair_ptr.back(),
         H.ell_val.size());
    RULE(H.ell_col.size() == (size_t)H.slab_col_ptr.back(), "slab_col_ptr[%zu] = %u: ell_col holds %zu", nslab, H.slab_col_ptr.back(), H.ell_col.size());
    RULE(H.items.size() % kItemWords == 0 && H.segs.size() % kSegWords == 0, "items / segs: %zu / %zu words are no whole records", H.items.size(), H.segs.size());
    RULE(H.er_seg_ptr.size() == nseg + 1, "er_seg_ptr: %zu entries for %zu segments (er_seg_row)", H.er_seg_ptr.size(), nseg);
    RULE(H.er_seg_ptr.back() >= 0 && H.er_col.size() == (uint64_t)H.er_seg_ptr.back() && H.er_val.size() == H.er_col.size(),
         "er_seg_ptr[%zu] = %lld: er_col / er_val hold %zu / %zu", nseg, (long long)H.er_seg_ptr.back(), H.er_col.size(), H.er_val.size());
    RULE(H.er_blocks.size() % 4 == 0, "er_blocks: %zu words are no whole records", H.er_blocks.size());
    RULE(H.sym ? H.slab_lrow.size() == nslab * kSlabRows : H.slab_lrow.empty(), "slab_lrow: %zu entries for %zu slabs%s", H.slab_lrow.size(), nslab,
         H.sym ? "" : " without symmetric pairs");
    // (0: no partition has a window -- every entry went to the residual; the builder makes such plans)
    RULE(H.lds_doubles >= 0 && H.lds_doubles <= EHYB_LDS_MAX_DOUBLES, "scalars: lds_doubles = %d", H.lds_doubles);
    RULE(perm_size == 0 || perm_size == (size_t)H.n_cols, "perm: %zu entries for %d columns", perm_size, H.n_cols);
    return true;
}

bool config_fits(const Config& c, const HostLayout& H, Why* why)
{
    // the words a launch looks its kernel up by (ehyb_hip.hip: ell_kernels, panel_kernels, er_kernels; ehyb_spmv_t.hip)
    RULE(c.threads == 256 || c.threads == 512 || c.threads == 1024, "config: threads = %d, the window kernels are built for 256, 512 and 1024", c.threads);
    RULE(c.er_threads == 256, "config: er_threads = %d, the residual kernels are built for 256", c.er_threads);
    RULE(c.ell_variant == 0 || c.ell_variant == 1 || c.ell_variant == 3, "config: ell_variant = %d (1: LDS slab counter, 3: round robin)", c.ell_variant);
    RULE(c.er_panel_threads == 0 || c.er_panel_threads == 512 || c.er_panel_threads == 1024, "config: er_panel_threads = %d (0, 512, 1024)", c.er_panel_threads);
    RULE(c.host_threads >= 0 && c.host_threads <= (1 << 16), "config: host_threads = %d", c.host_threads);
    RULE(c.val_f32 == 0 || c.val_f32 == 1, "config: val_f32 = %d", c.val_f32);
    // the forms as the builder combines them (layout.cpp: LayoutBuild, inline_residual)
    // (the direct shape keeps the work items of its slabs, which no launch walks: launch_window leaves before it looks at them)
    RULE(!H.direct || (!H.sym && !H.inline_er && !H.pb_assign && H.row_begin == 0 && H.row_end == H.n_cols),
         "scalars: the direct shape with sym %d, inline_er %d, pb_assign %d, rows [%d, %d) of %d", H.sym, H.inline_er, H.pb_assign, H.row_begin, H.row_end, H.n_cols);
    RULE(!H.pb_assign || (H.er_panel && !H.sym), "scalars: pb_assign with er_panel %d, sym %d", H.er_panel, H.sym);
    RULE(!H.inline_er || !H.er_panel, "scalars: inline_er with er_panel");
    RULE(H.sym ? H.yacc_doubles >= 0 && H.yacc_doubles <= H.lds_doubles : H.yacc_doubles == 0, "scalars: yacc_doubles = %d (sym %d, lds_doubles %d)",
         H.yacc_doubles, H.sym, H.lds_doubles);
    // the window launch asks for ell_lds_bytes: the image(s) and the slab counter within the 160 KiB
    RULE(H.direct || ell_lds_bytes(H, 1) <= (size_t)EHYB_LDS_MAX_DOUBLES * 8, "scalars: lds_doubles = %d, a window launch would ask for %zu bytes of LDS",
         H.lds_doubles, ell_lds_bytes(H, 1));
    const size_t nseg = H.er_seg_row.size();
    RULE(H.er_bins[0] == 0 && H.er_bins[0] <= H.er_bins[1] && H.er_bins[1] <= H.er_bins[2] && H.er_bins[2] <= H.er_bins[3] && (size_t)H.er_bins[3] == nseg,
         "er_bins: {%d, %d, %d, %d} for %zu segments (er_seg_row)", H.er_bins[0], H.er_bins[1], H.er_bins[2], H.er_bins[3], nseg);
    return true;
}

// LDS image of partition p: own rows from the even row at or below the start, then the halo
struct PartImage {
    std::vector<int32_t> own, len;  // (start & 1) + win_len; own + halo count
};

bool partitions_fit(const HostLayout& H, PartImage* I, Why* why)
{
    const int np = H.n_parts;
    const std::vector<int32_t>& pb = H.part_boundary;
    RULE(pb[0] == H.row_begin && pb[(size_t)np] == H.row_end, "part_boundary: runs from %d to %d, the rows are [%d, %d)", pb[0], pb[(size_t)np], H.row_begin,
         H.row_end);
    RULE(H.halo_ptr[0] == 0, "halo_ptr[0] = %d", H.halo_ptr[0]);
    I->own.assign((size_t)np, 0), I->len.assign((size_t)np, 0);
    for (int p = 0; p < np; ++p) {
        RULE(pb[p] <= pb[p + 1], "part_boundary[%d] = %d descends to %d", p, pb[p], pb[p + 1]);
        RULE(H.halo_ptr[p] <= H.halo_ptr[p + 1], "halo_ptr[%d] = %d descends to %d", p, H.halo_ptr[p], H.halo_ptr[p + 1]);
        const int64_t wl = H.win_len[p], hn = H.halo_ptr[p + 1] - H.halo_ptr[p], own = (pb[p] & 1) + wl;
        RULE(wl >= 0 && pb[p] + wl <= H.n_cols, "win_len[%d] = %lld: the window from part_boundary[%d] = %d leaves the %d columns", p, (long long)wl, p, pb[p],
             H.n_cols);
        // symmetric pairs: the accumulators of the image's rows sit behind it, and the image's rows are the partition's (they are
        // written to y from there)
        RULE(!H.sym || wl == pb[p + 1] - pb[p], "win_len[%d] = %lld: with symmetric pairs the window is the partition's rows part_boundary[%d..] = [%d, %d)", p,
             (long long)wl, p, pb[p], pb[p + 1]);
        RULE(own + hn + (H.sym ? own : 0) <= H.lds_doubles, "win_len[%d] = %lld (from the even row at or below part_boundary[%d] = %d) + halo_ptr's %lld columns%s exceed lds_doubles = %d",
             p, (long long)wl, p, pb[p], (long long)hn, H.sym ? " + the accumulators" : "", H.lds_doubles);
        RULE(!H.sym || own <= H.yacc_doubles, "win_len[%d] = %lld: more accumulators than yacc_doubles = %d", p, (long long)wl, H.yacc_doubles);
        I->own[(size_t)p] = (int32_t)own, I->len[(size_t)p] = (int32_t)(own + hn);
    }
    return all_of_parallel((int64_t)H.halo_cols.size(), why, [&](int64_t i, Why* why) {
        RULE(H.halo_cols[(size_t)i] >= 0 && H.halo_cols[(size_t)i] < H.n_cols, "halo_cols[%lld] = %d outside the %d columns", (long long)i, H.halo_cols[(size_t)i],
             H.n_cols);
        return true;
    });
}

// One slab: its record against the prefix arrays, its rows against its partition, its lane maps and every column word.
bool slab_fits(const HostLayout& H, const PartImage& I, int64_t s, Why* why)
{
    const size_t z = (size_t)s;
    const uint32_t* rec = &H.slab_meta[z * kSlabWords];
    const SlabShape sh = unpack_slab_shape(rec[SLAB_SHAPE]);
    const long long S = (long long)s;
    RULE(H.slab_pair_ptr[z] <= H.slab_pair_ptr[z + 1], "slab_pair_ptr[%lld] = %u descends to %u", S, H.slab_pair_ptr[z], H.slab_pair_ptr[z + 1]);
    RULE(H.slab_col_ptr[z] <= H.slab_col_ptr[z + 1], "slab_col_ptr[%lld] = %u descends to %u", S, H.slab_col_ptr[z], H.slab_col_ptr[z + 1]);
    RULE(s > 0 || (H.slab_pair_ptr[0] == 0 && H.slab_col_ptr[0] == 0), "slab_pair_ptr[0] = %u, slab_col_ptr[0] = %u", H.slab_pair_ptr[0], H.slab_col_ptr[0]);
    RULE(rec[SLAB_PAIR_PTR] == H.slab_pair_ptr[z], "slab_meta[%lld] = %u is not slab_pair_ptr[%lld] = %u", 4 * S + SLAB_PAIR_PTR, rec[SLAB_PAIR_PTR], S,
         H.slab_pair_ptr[z]);
    RULE(rec[SLAB_COL_PTR] == H.slab_col_ptr[z], "slab_meta[%lld] = %u is not slab_col_ptr[%lld] = %u", 4 * S + SLAB_COL_PTR, rec[SLAB_COL_PTR], S,
         H.slab_col_ptr[z]);
    RULE(rec[SLAB_ROW] == (uint32_t)H.slab_row[z], "slab_meta[%lld] = %u is not slab_row[%lld] = %d", 4 * S + SLAB_ROW, rec[SLAB_ROW], S, H.slab_row[z]);
    RULE(pack_slab_shape(sh.pairs, sh.er_pairs, sh.relative, sh.groups) == rec[SLAB_SHAPE], "slab_meta[%lld] = 0x%08x sets a bit no host record has",
         4 * S + SLAB_SHAPE, rec[SLAB_SHAPE]);
    RULE(sh.er_pairs == 0 || H.inline_er, "slab_meta[%lld] = 0x%08x: inline residual pairs in a plan without an inline residual", 4 * S + SLAB_SHAPE, rec[SLAB_SHAPE]);
    RULE(!sh.relative || !H.sym, "slab_meta[%lld] = 0x%08x: relative columns with symmetric pairs", 4 * S + SLAB_SHAPE, rec[SLAB_SHAPE]);
    RULE(H.slab_pair_ptr[z + 1] - H.slab_pair_ptr[z] == sh.pairs + sh.er_pairs, "slab_meta[%lld] = 0x%08x: %u + %u pairs, slab_pair_ptr[%lld..] has %u",
         4 * S + SLAB_SHAPE, rec[SLAB_SHAPE], sh.pairs, sh.er_pairs, S, H.slab_pair_ptr[z + 1] - H.slab_pair_ptr[z]);
    const uint64_t words = (uint64_t)sh.pairs * sh.groups + (uint64_t)sh.er_pairs * 2 * kSlabRows;
    RULE(H.slab_col_ptr[z + 1] - H.slab_col_ptr[z] == words, "slab_meta[%lld] = 0x%08x: %llu column words, slab_col_ptr[%lld..] has %u", 4 * S + SLAB_SHAPE,
         rec[SLAB_SHAPE], (unsigned long long)words, S, H.slab_col_ptr[z + 1] - H.slab_col_ptr[z]);
    const int32_t p = H.slab_part[z];
    RULE(p >= 0 && p < H.n_parts, "slab_part[%lld] = %d of %d partitions", S, p, H.n_parts);
    const int32_t ps = H.part_boundary[(size_t)p], pe = H.part_boundary[(size_t)p + 1], r0 = H.slab_row[z];
    RULE(r0 >= ps && r0 < pe, "slab_row[%lld] = %d outside the rows [%d, %d) of partition slab_part[%lld] = %d (part_boundary)", S, r0, ps, pe, S, p);
    const uint32_t own = (uint32_t)I.own[(size_t)p], len = (uint32_t)I.len[(size_t)p], odd = (uint32_t)(ps & 1);
    const uint8_t* lg = &H.lane_group[z * kSlabRows];
    for (int l = 0; l < kSlabRows; ++l)
        RULE((uint32_t)(lg[l] & 0x3F) < sh.groups && (H.sym || lg[l] < 64), "lane_group[%lld] = %u: the slab (slab_meta[%lld]) has %u groups", S * 64 + l, lg[l],
             4 * S + SLAB_SHAPE, sh.groups);
    const uint32_t* c = H.ell_col.data() + H.slab_col_ptr[z];
    const long long c0 = (long long)H.slab_col_ptr[z];
    if (H.sym) {
        const uint16_t* lr = &H.slab_lrow[z * kSlabRows];
        for (int l = 0; l < kSlabRows; ++l)
            RULE(lr[l] == 0xFFFF || (lr[l] >= odd && lr[l] < own && lr[l] < H.yacc_doubles),
                 "slab_lrow[%lld] = %u outside the rows [%u, %u) of its partition's image (win_len[%d], yacc_doubles = %d)", S * 64 + l, lr[l], odd, own, p,
                 H.yacc_doubles);
        // bit 15: the entry also stands for its mirror image -- the column is then a row of the partition (an accumulator)
        for (uint64_t w = 0; w < (uint64_t)sh.pairs * sh.groups; ++w)
            for (int h = 0; h < 2; ++h) {
                const uint32_t e = h ? c[w] >> 16 : c[w] & 0xFFFFu, col = e & 0x7FFFu;
                RULE(col < len, "ell_col[%lld] = 0x%08x: column %u outside the %u slots of the image of partition %d (part_boundary, win_len, halo_ptr)", c0 + (long long)w, c[w],
                     col, len, p);
                RULE(!(e & 0x8000u) || (col >= odd && col < own), "ell_col[%lld] = 0x%08x: mirror target %u outside the rows [%u, %u) of partition %d", c0 + (long long)w,
                     c[w], col, odd, own, p);
            }
    } else if (!sh.relative) {
        for (uint64_t w = 0; w < (uint64_t)sh.pairs * sh.groups; ++w)
            RULE((c[w] & 0xFFFFu) < len && (c[w] >> 16) < len, "ell_col[%lld] = 0x%08x: a column outside the %u slots of the image of partition %d (part_boundary, win_len, halo_ptr)",
                 c0 + (long long)w, c[w], len, p);
    } else if (sh.pairs > 0) {
        // relative to the lane's own place in the image, mod 2^16: per group the lanes with a row span [lo, hi], and the image is
        // at most 2^16 slots, so a word fits all of them iff it fits the first without leaving the image by the last
        RULE(len >= 1, "slab_meta[%lld] = 0x%08x: lanes without a row read slot 0 of an empty image (win_len[%d])", 4 * S + SLAB_SHAPE, rec[SLAB_SHAPE], p);
        int32_t lo[kSlabRows], hi[kSlabRows];
        for (uint32_t g = 0; g < sh.groups; ++g) lo[g] = INT32_MAX, hi[g] = -1;
        const int32_t base = ps & ~1;
        for (int l = 0; l < kSlabRows && r0 + l < pe; ++l) {
            const int32_t lrow = r0 + l - base;
            lo[lg[l]] = std::min(lo[lg[l]], lrow), hi[lg[l]] = std::max(hi[lg[l]], lrow);
        }
        for (uint64_t w = 0; w < (uint64_t)sh.pairs * sh.groups; ++w) {
            const uint32_t g = (uint32_t)(w % sh.groups);
            if (hi[g] < 0) continue;  // no lane with a row reads the word
            for (int h = 0; h < 2; ++h) {
                const uint32_t e = h ? c[w] >> 16 : c[w] & 0xFFFFu, first = (e + (uint32_t)lo[g]) & 0xFFFFu;
                RULE(first + (uint32_t)(hi[g] - lo[g]) < len, "ell_col[%lld] = 0x%08x: offset %u leaves the %u slots of the image of partition %d (part_boundary, win_len, halo_ptr) for a lane of slab_row[%lld] (lane_group)",
                     c0 + (long long)w, c[w], e, len, p, S);
            }
        }
    }
    // inline residual: global columns, read by every lane
    const uint32_t* ce = c + (uint64_t)sh.pairs * sh.groups;
    for (uint64_t w = 0; w < (uint64_t)sh.er_pairs * 2 * kSlabRows; ++w)
        RULE(ce[w] < (uint32_t)H.n_cols, "ell_col[%lld] = %u: inline residual column outside the %d columns", c0 + (long long)((uint64_t)sh.pairs * sh.groups + w), ce[w],
             H.n_cols);
    return true;
}

// Work items and segments: what a workgroup walks; every slab in one segment (pb_assign: partitions without a window have none).
bool items_fit(const HostLayout& H, Why* why)
{
    const int64_t nslab = (int64_t)H.slab_row.size(), nsegs = (int64_t)(H.segs.size() / kSegWords), nitems = (int64_t)(H.items.size() / kItemWords);
    const int64_t nseg_er = (int64_t)H.er_seg_row.size();
    std::vector<uint8_t> in_seg((size_t)nslab, 0), in_item((size_t)nsegs, 0);
    for (int64_t g = 0; g < nsegs; ++g) {
        const int32_t* sg = &H.segs[(size_t)g * kSegWords];
        const long long G8 = 8 * (long long)g;
        const int32_t p = sg[SEG_PART];
        RULE(p >= 0 && p < H.n_parts, "segs[%lld] = %d of %d partitions", G8 + SEG_PART, p, H.n_parts);
        RULE(sg[SEG_SLAB_BEGIN] >= 0 && sg[SEG_SLAB_BEGIN] < sg[SEG_SLAB_END] && sg[SEG_SLAB_END] <= nslab, "segs[%lld] = %d, segs[%lld] = %d: slabs of %lld",
             G8 + SEG_SLAB_BEGIN, sg[SEG_SLAB_BEGIN], G8 + SEG_SLAB_END, sg[SEG_SLAB_END], (long long)nslab);
        RULE(sg[SEG_ROW_BEGIN] == H.part_boundary[(size_t)p], "segs[%lld] = %d is not part_boundary[%d] = %d", G8 + SEG_ROW_BEGIN, sg[SEG_ROW_BEGIN], p,
             H.part_boundary[(size_t)p]);
        RULE(sg[SEG_ROW_END] == H.part_boundary[(size_t)p + 1], "segs[%lld] = %d is not part_boundary[%d] = %d", G8 + SEG_ROW_END, sg[SEG_ROW_END], p + 1,
             H.part_boundary[(size_t)p + 1]);
        RULE(sg[SEG_WIN_LEN] == H.win_len[(size_t)p], "segs[%lld] = %d is not win_len[%d] = %d", G8 + SEG_WIN_LEN, sg[SEG_WIN_LEN], p, H.win_len[(size_t)p]);
        RULE(sg[SEG_HALO_BEGIN] == H.halo_ptr[(size_t)p], "segs[%lld] = %d is not halo_ptr[%d] = %d", G8 + SEG_HALO_BEGIN, sg[SEG_HALO_BEGIN], p, H.halo_ptr[(size_t)p]);
        RULE(sg[SEG_HALO_COUNT] == H.halo_ptr[(size_t)p + 1] - H.halo_ptr[(size_t)p], "segs[%lld] = %d is not the %d columns of halo_ptr[%d..]", G8 + SEG_HALO_COUNT,
             sg[SEG_HALO_COUNT], H.halo_ptr[(size_t)p + 1] - H.halo_ptr[(size_t)p], p);
        for (int64_t s = sg[SEG_SLAB_BEGIN]; s < sg[SEG_SLAB_END]; ++s) {
            RULE(H.slab_part[(size_t)s] == p, "segs[%lld..%lld]: slab %lld of the segment has slab_part[%lld] = %d, not segs[%lld] = %d", G8 + SEG_SLAB_BEGIN,
                 G8 + SEG_SLAB_END, (long long)s, (long long)s, H.slab_part[(size_t)s], G8 + SEG_PART, p);
            RULE(!in_seg[(size_t)s], "segs[%lld..%lld]: slab %lld belongs to an earlier segment too", G8 + SEG_SLAB_BEGIN, G8 + SEG_SLAB_END, (long long)s);
            in_seg[(size_t)s] = 1;
        }
    }
    if (nitems > 0)
        for (int64_t s = 0; s < nslab; ++s)
            RULE(in_seg[(size_t)s] || (H.pb_assign && H.win_len[(size_t)H.slab_part[(size_t)s]] == 0 &&
                                      H.halo_ptr[(size_t)H.slab_part[(size_t)s]] == H.halo_ptr[(size_t)H.slab_part[(size_t)s] + 1]),
                 "segs: slab %lld (slab_part[%lld] = %d) belongs to no segment (and win_len[%d] = %d, halo_ptr: not a partition without a window of a plan with pb_assign)", (long long)s,
                 (long long)s, H.slab_part[(size_t)s], H.slab_part[(size_t)s], H.win_len[(size_t)H.slab_part[(size_t)s]]);
    for (int64_t it = 0; it < nitems; ++it) {
        const int32_t* rec = &H.items[(size_t)it * kItemWords];
        const long long I8 = 8 * (long long)it;
        RULE(rec[ITEM_SEG_BEGIN] >= 0 && rec[ITEM_SEG_BEGIN] <= rec[ITEM_SEG_END] && rec[ITEM_SEG_END] <= nsegs, "items[%lld] = %d, items[%lld] = %d: segments of %lld (segs)",
             I8 + ITEM_SEG_BEGIN, rec[ITEM_SEG_BEGIN], I8 + ITEM_SEG_END, rec[ITEM_SEG_END], (long long)nsegs);
        RULE(rec[ITEM_SLAB_BEGIN] >= 0 && rec[ITEM_SLAB_BEGIN] <= rec[ITEM_SLAB_END] && rec[ITEM_SLAB_END] <= nslab, "items[%lld] = %d, items[%lld] = %d: slabs of %lld",
             I8 + ITEM_SLAB_BEGIN, rec[ITEM_SLAB_BEGIN], I8 + ITEM_SLAB_END, rec[ITEM_SLAB_END], (long long)nslab);
        RULE(0 <= rec[ITEM_ER_BEGIN] && rec[ITEM_ER_BEGIN] <= rec[ITEM_ER_B64] && rec[ITEM_ER_B64] <= rec[ITEM_ER_B16] && rec[ITEM_ER_B16] <= rec[ITEM_ER_END] &&
                 rec[ITEM_ER_END] <= nseg_er,
             "items[%lld..%lld] = {%d, %d, %d, %d}: residual bins of %lld segments (er_seg_row)", I8 + ITEM_ER_BEGIN, I8 + ITEM_ER_END, rec[ITEM_ER_BEGIN], rec[ITEM_ER_B64],
             rec[ITEM_ER_B16], rec[ITEM_ER_END], (long long)nseg_er);
        for (int64_t g = rec[ITEM_SEG_BEGIN]; g < rec[ITEM_SEG_END]; ++g) {
            RULE(!in_item[(size_t)g], "items[%lld..%lld]: segment %lld belongs to an earlier item too (two workgroups would write its rows)", I8 + ITEM_SEG_BEGIN,
                 I8 + ITEM_SEG_END, (long long)g);
            in_item[(size_t)g] = 1;
            const int32_t* sg = &H.segs[(size_t)g * kSegWords];
            RULE(sg[SEG_SLAB_BEGIN] >= rec[ITEM_SLAB_BEGIN] && sg[SEG_SLAB_END] <= rec[ITEM_SLAB_END], "items[%lld] = %d, items[%lld] = %d: segment %lld has the slabs segs[%lld..] = [%d, %d)",
                 I8 + ITEM_SLAB_BEGIN, rec[ITEM_SLAB_BEGIN], I8 + ITEM_SLAB_END, rec[ITEM_SLAB_END], (long long)g, 8 * (long long)g + SEG_SLAB_BEGIN, sg[SEG_SLAB_BEGIN],
                 sg[SEG_SLAB_END]);
        }
    }
    for (int64_t g = 0; g < nsegs; ++g) RULE(in_item[(size_t)g], "items: segment %lld (segs[%lld..]) belongs to no item", (long long)g, 8 * (long long)g);
    return true;
}

// The CSR residual: er_bin / er_bin_t walk er_col and er_val over [er_seg_ptr[s], er_seg_ptr[s + 1]) and write y[er_seg_row[s]].
bool residual_fits(const HostLayout& H, Why* why)
{
    const int64_t nseg = (int64_t)H.er_seg_row.size();
    RULE(H.er_seg_ptr[0] == 0, "er_seg_ptr[0] = %lld", (long long)H.er_seg_ptr[0]);
    if (!all_of_parallel(nseg, why, [&](int64_t s, Why* why) {
            RULE(H.er_seg_ptr[(size_t)s] <= H.er_seg_ptr[(size_t)s + 1], "er_seg_ptr[%lld] = %lld descends to %lld", (long long)s, (long long)H.er_seg_ptr[(size_t)s],
                 (long long)H.er_seg_ptr[(size_t)s + 1]);
            const int32_t raw = H.er_seg_row[(size_t)s], r = raw & 0x7FFFFFFF;
            RULE(r >= H.row_begin && r < H.row_end, "er_seg_row[%lld] = 0x%08x: row %d outside [%d, %d)", (long long)s, (uint32_t)raw, r, H.row_begin, H.row_end);
            RULE(!H.direct || raw >= 0, "er_seg_row[%lld] = 0x%08x: a split row in the direct shape, whose kernel assigns y", (long long)s, (uint32_t)raw);
            return true;
        }))
        return false;
    if (!all_of_parallel((int64_t)H.er_col.size(), why, [&](int64_t i, Why* why) {
            RULE(H.er_col[(size_t)i] >= 0 && H.er_col[(size_t)i] < H.n_cols, "er_col[%lld] = %d outside the %d columns", (long long)i, H.er_col[(size_t)i], H.n_cols);
            return true;
        }))
        return false;
    for (size_t b = 0; b < H.er_blocks.size(); b += 4) {
        const int32_t* q = &H.er_blocks[b];
        RULE(q[0] >= 0 && q[0] <= q[1] && q[1] <= nseg, "er_blocks[%zu] = %d, er_blocks[%zu] = %d: segments of %lld (er_seg_row)", b, q[0], b + 1, q[1], (long long)nseg);
        RULE(q[2] == 64 || q[2] == 16 || q[2] == 4, "er_blocks[%zu] = %d lanes per segment (64, 16, 4)", b + 2, q[2]);
    }
    return true;
}

// What panel_consistent leaves open: the rows pass 2 adds into, the columns pass 1 gathers from the panel a unit staged, units
// that are not empty (pass 1 reads the chunk records of its first chunk before it looks at the count), ascending segment items.
bool panel_fits(const HostLayout& H, Why* why)
{
    RULE(panel_consistent(H), "pb_*: the panel arrays do not fit together (pb_units1, pb_units2, pb_items1, pb_seg_item, pb_dst, pb_col, col_seg_first)");
    if (!H.er_panel) return true;
    for (size_t i = 0; i + 1 < H.pb_seg_item.size(); ++i)
        RULE(H.pb_seg_item[i] <= H.pb_seg_item[i + 1], "pb_seg_item[%zu] = %d descends to %d", i, H.pb_seg_item[i], H.pb_seg_item[i + 1]);
    if (!all_of_parallel((int64_t)(H.pb_units1.size() / 4), why, [&](int64_t u, Why* why) {
            const int32_t* q = &H.pb_units1[(size_t)u * 4];
            RULE(q[3] > q[2], "pb_units1[%lld] = %d, pb_units1[%lld] = %d: a unit without entries", 4 * (long long)u + 2, q[2], 4 * (long long)u + 3, q[3]);
            for (int64_t e = q[2]; e < q[3]; ++e)
                RULE(H.pb_col[(size_t)e] < q[1], "pb_col[%lld] = %u outside the %d columns its unit (pb_units1[%lld..]) stages", (long long)e, H.pb_col[(size_t)e], q[1],
                     4 * (long long)u);
            return true;
        }))
        return false;
    return all_of_parallel((int64_t)(H.pb_units2.size() / 4), why, [&](int64_t u, Why* why) {
        const int32_t* q = &H.pb_units2[(size_t)u * 4];
        const int32_t rows = q[3] < 0 ? -q[3] : q[3];
        for (int64_t i = q[0]; i < q[1]; ++i)
            RULE(H.pb_row[(size_t)i] < rows, "pb_row[%lld] = %u outside the %d rows of its block (pb_units2[%lld..])", (long long)i, H.pb_row[(size_t)i], rows,
                 4 * (long long)u);
        return true;
    });
}

bool col_segs_fit(const HostLayout& H, Why* why)
{
    const std::vector<int32_t>& f = H.col_seg_first;
    if (f.empty()) return true;
    RULE(f.size() >= 2 && f.front() == 0 && f.back() == H.n_cols, "col_seg_first: %zu entries from %d to %d, the columns are [0, %d)", f.size(), f.front(), f.back(),
         H.n_cols);
    for (size_t s = 0; s + 1 < f.size(); ++s)
        RULE(f[s] <= f[s + 1] && !(s > 0 && (f[s] & 1)), "col_seg_first[%zu] = %d (segments ascend and start on even columns)", s, f[s]);
    return true;
}

bool perm_fits(const std::vector<int32_t>& perm, int n_cols, Why* why)
{
    if (perm.empty()) return true;
    std::vector<uint8_t> seen((size_t)n_cols, 0);
    for (size_t i = 0; i < perm.size(); ++i) {
        RULE(perm[i] >= 0 && perm[i] < n_cols, "perm[%zu] = %d outside the %d columns", i, perm[i], n_cols);
        RULE(!seen[(size_t)perm[i]], "perm[%zu] = %d appears twice", i, perm[i]);
        seen[(size_t)perm[i]] = 1;
    }
    return true;
}

bool plan_fits(const ehyb_plan* P, Why* why)
{
    const HostLayout& H = P->host;
    if (!sizes_fit(H, P->perm.size(), why) || !config_fits(P->cfg, H, why)) return false;
    OmpScope omp(P->cfg.host_threads);
    PartImage I;
    if (!partitions_fit(H, &I, why)) return false;
    if (!all_of_parallel((int64_t)H.slab_row.size(), why, [&](int64_t s, Why* why) { return slab_fits(H, I, s, why); })) return false;
    if (!items_fit(H, why) || !residual_fits(H, why) || !col_segs_fit(H, why)) return false;
    // (a panel form built on the device keeps its streams there until somebody asks for them: nothing of it is on the host)
    if (!H.pb_host_missing && !H.deferred.pending && !panel_fits(H, why)) return false;
    return perm_fits(P->perm, H.n_cols, why);
}
#undef RULE

}  // namespace

extern "C" {

// Order-sensitive 64-bit digest of the matrix a plan was built from (dimension, entry count,
// coordinates and values as stored).  0 is never returned: it means "do not check" to ehyb_plan_load.
uint64_t ehyb_matrix_key(const matrixCOO* m)
{
    if (!m) return 1;
    uint64_t h = mix64(0x45485942ull ^ (uint64_t)(uint32_t)m->dimension) ^ mix64((uint64_t)(uint32_t)m->totalNum + 0x9E37ull);
    const int64_t nnz = m->totalNum;
    if (m->I && m->J && m->V) {
        // four independent lanes, so the loop is not one long multiply chain
        uint64_t a[4] = {h, h ^ 0x1111, h ^ 0x2222, h ^ 0x3333};
        for (int64_t k = 0; k < nnz; ++k) {
            uint64_t bits;
            memcpy(&bits, &m->V[k], 8);
            const uint64_t w = ((uint64_t)(uint32_t)m->I[k] << 32 | (uint32_t)m->J[k]) ^ (bits * 0x9E3779B97F4A7C15ull);
            uint64_t& s = a[k & 3];
            s = (s ^ w) * 0xBF58476D1CE4E5B9ull;
            s ^= s >> 29;
        }
        h = mix64(a[0]) ^ mix64(a[1] + 1) ^ mix64(a[2] + 2) ^ mix64(a[3] + 3);
    }
    return h ? h : 1;
}

// Host arithmetic only: would any entry point (ehyb_spmv[_phase, _walk, _part, _t], ehyb_spmm up to ehyb_spmm_max_k, the solvers'
// fused multiply, the transcoder of ehyb_plan_upload, encode_panel_slots) index outside an array of this plan?
int ehyb_plan_check(const ehyb_plan* plan)
{
    clear_error();
    if (!plan) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_check: null plan");
    Why why;
    if (!plan_fits(plan, &why)) EHYB_FAIL(EHYB_ERR_FORMAT, "ehyb_plan_check: %s", why.text);
    return EHYB_OK;
}

int ehyb_plan_save(const ehyb_plan* plan, const int* reorder_list, uint64_t matrix_key, const char* path)
{
    clear_error();
    if (!plan || !path) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_save: null argument");
    if (plan->host_values_stale)
        EHYB_FAIL(EHYB_ERR_STATE, "ehyb_plan_save: the plan's values were replaced on the device (ehyb_plan_set_values); its host copy is stale");
    if (plan->host.pb_host_missing) {  // a panel form built on the device: its streams come back first
        const int rc = materialize_panel_host(const_cast<ehyb_plan*>(plan));
        if (rc != EHYB_OK) return rc;
    }
    HostLayout& H = const_cast<HostLayout&>(plan->host);  // each_array takes non-const; nothing is modified
    File f(fopen(path, "wb"));
    if (!f) EHYB_FAIL(EHYB_ERR_IO, "ehyb_plan_save: cannot create %s", path);
    Scalars s{H.n_cols, H.row_begin, H.row_end, H.n_parts, H.lds_doubles, H.inline_er ? 1 : 0, {0}, H.sym ? 1 : 0, H.yacc_doubles,
              H.er_panel ? 1 : 0, H.pb_panel_cols, H.pb_rows_max, H.direct ? 1 : 0, H.pb_partials, H.pb_bytes, H.pb_assign ? 1 : 0, plan->cfg.val_f32 == 1 ? 1 : 0};
    memcpy(s.er_bins, H.er_bins, sizeof s.er_bins);
    std::vector<int32_t> perm;
    if (reorder_list) perm.assign(reorder_list, reorder_list + H.n_cols);
    bool ok = fwrite(kMagic, 8, 1, f.get()) == 1 && put(f.get(), matrix_key) && put_cfg(f.get(), plan->cfg) && put(f.get(), s) &&
              put(f.get(), H.stats) && put_vec(f.get(), perm) &&
              each_array(H, [&](auto& v) { return put_vec(f.get(), v); }) && fwrite(kEnd, 8, 1, f.get()) == 1;
    FILE* raw = f.release();
    ok = (fclose(raw) == 0) && ok;
    if (!ok) {
        remove(path);
        EHYB_FAIL(EHYB_ERR_IO, "ehyb_plan_save: write to %s failed", path);
    }
    return EHYB_OK;
}

int ehyb_plan_load(const char* path, uint64_t expect_key, ehyb_plan** plan, int* reorder_list)
{
    clear_error();
    if (!path || !plan) EHYB_FAIL(EHYB_ERR_ARG, "ehyb_plan_load: null argument");
    *plan = nullptr;
    File f(fopen(path, "rb"));
    if (!f) EHYB_FAIL(EHYB_ERR_IO, "ehyb_plan_load: cannot open %s", path);
    char magic[8];
    uint64_t key = 0;
    if (fread(magic, 8, 1, f.get()) != 1 || memcmp(magic, kMagic, 8) != 0 || !get(f.get(), key))
        EHYB_FAIL(EHYB_ERR_FORMAT, "ehyb_plan_load: %s is not a plan file of this version", path);
    if (expect_key != 0 && key != expect_key)
        EHYB_FAIL(EHYB_ERR_FORMAT, "ehyb_plan_load: %s was built from another matrix (key %016llx, expected %016llx)", path,
                  (unsigned long long)key, (unsigned long long)expect_key);
    std::unique_ptr<ehyb_plan> P(new (std::nothrow) ehyb_plan());
    if (!P) EHYB_FAIL(EHYB_ERR_ALLOC, "ehyb_plan_load: out of memory");
    Scalars s;
    HostLayout& H = P->host;
    std::vector<int32_t> perm;
    const uint64_t limit = 1ull << 36;  // sanity bound for any array count
    try {
        bool ok = get_cfg(f.get(), P->cfg) && get(f.get(), s) && get(f.get(), H.stats) && get_vec(f.get(), perm, limit) &&
                  each_array(H, [&](auto& v) { return get_vec(f.get(), v, limit); });
        char end[8];
        ok = ok && fread(end, 8, 1, f.get()) == 1 && memcmp(end, kEnd, 8) == 0;
        if (!ok) EHYB_FAIL(EHYB_ERR_FORMAT, "ehyb_plan_load: %s is truncated or damaged", path);
    } catch (const std::bad_alloc&) {
        EHYB_FAIL(EHYB_ERR_ALLOC, "ehyb_plan_load: out of memory reading %s", path);
    }
    H.n_cols = s.n_cols, H.row_begin = s.row_begin, H.row_end = s.row_end, H.n_parts = s.n_parts;
    H.lds_doubles = s.lds_doubles, H.inline_er = s.inline_er != 0;
    H.sym = s.sym != 0, H.yacc_doubles = s.yacc_doubles;
    H.er_panel = s.er_panel != 0, H.pb_panel_cols = s.pb_panel_cols, H.pb_rows_max = s.pb_rows_max, H.direct = s.direct != 0;
    H.pb_partials = s.pb_partials, H.pb_bytes = s.pb_bytes;
    H.pb_padded = (int64_t)H.pb_val.size();
    H.pb_assign = s.pb_assign != 0 && H.er_panel;
    memcpy(H.er_bins, s.er_bins, sizeof s.er_bins);
    P->cfg.val_f32 = s.val_f32 == 1 ? 1 : 0;
    P->cfg.value_map = 0;  // the slot maps are not part of the file: a loaded plan cannot be refilled
    P->perm.swap(perm);    // also readable through ehyb_plan_host_array(EHYB_ARR_PERM)
    // the sizes the kernels rely on must fit together, and every index they form from the arrays must stay inside the array it
    // indexes -- a damaged file must not reach the GPU (nor device_cols / encode_panel_slots on the host)
    Why why;
    if (!plan_fits(P.get(), &why)) EHYB_FAIL(EHYB_ERR_FORMAT, "ehyb_plan_load: %s is damaged: %s", path, why.text);
    if (H.er_panel) encode_panel_slots(&H);  // what pass 1 streams is derived from pb_col + pb_dst, not stored
    if (reorder_list) {
        if (P->perm.empty()) EHYB_FAIL(EHYB_ERR_FORMAT, "ehyb_plan_load: %s holds no permutation", path);
        std::copy(P->perm.begin(), P->perm.end(), reorder_list);
    }
    *plan = P.release();
    return EHYB_OK;
}

}  // extern "C"
