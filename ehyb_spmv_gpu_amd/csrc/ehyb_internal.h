// Internal declarations shared by the host builder, the partitioner and the HIP side.
// Nothing here is part of the C-ABI (see include/ehyb.h).
#pragma once
#include <atomic>
#include <cstdint>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>
#include "ehyb.h"

namespace ehyb {

// The big arrays of a layout (hundreds of MB each): a vector whose resize() does NOT write the new elements -- the builder
// fills every element itself, partition by partition on all host threads; a value-initialising resize was one more pass
// over the array on ONE thread (audikw_1-like: 1.2 GB of such fills, a quarter of the plan's build time).
// release_big: free() of a malloc()ed block; a block of 64 MiB or more is handed to a helper thread -- giving 600 MB of touched pages back to the
// kernel takes 70-75 ms on the GPU box's host (more than gathering them took), and nothing the caller does next has to wait for it.
void release_big(void* p, size_t bytes);
template <class T>
struct NoInitAlloc {
    using value_type = T;
    template <class U>
    struct rebind {
        using other = NoInitAlloc<U>;
    };
    NoInitAlloc() = default;
    template <class U>
    NoInitAlloc(const NoInitAlloc<U>&) {}
    T* allocate(size_t n)
    {
        void* p = malloc(std::max<size_t>(n * sizeof(T), 1));
        if (!p) throw std::bad_alloc();
        return static_cast<T*>(p);
    }
    void deallocate(T* p, size_t) { free(p); }
    template <class U>
    bool operator==(const NoInitAlloc<U>&) const { return true; }
    template <class U>
    bool operator!=(const NoInitAlloc<U>&) const { return false; }
    template <class U, class... A>
    void construct(U* p, A&&... a)
    {
        if constexpr (sizeof...(A) == 0)
            ::new ((void*)p) U;  // default-initialised: left as it is for arithmetic types
        else
            ::new ((void*)p) U(std::forward<A>(a)...);
    }
};
template <class T>
using BigVec = std::vector<T, NoInitAlloc<T>>;

// ---------------------------------------------------------------- errors
void set_error(const char* fmt, ...);
void clear_error();

#define EHYB_FAIL(code, ...)            \
    do {                                \
        ::ehyb::set_error(__VA_ARGS__); \
        return (code);                  \
    } while (0)

// ---------------------------------------------------------------- config
// Resolved configuration: every field has its final value.
struct Config {
    int lds_doubles;
    int part_rows;
    int threads;
    int window_mode;
    int items_per_cu;
    int partitioner;
    int er_seg_len;
    int host_threads;
    int verbose;
    int seed;
    int n_top;
    int er_threads;
    int ell_variant;
    int col_sharing;
    int fuse_er;
    int cap_split;
    int hub_rule;
    int sym_pairs;
    int part_boundary_cap;  // ints the caller's partBoundary holds; 0 = m->nParts + 1, never more
    int er_mode;            // 0 automatic, 1 CSR segments, 2 panel form
    int er_panel_cols;
    int er_block_rows;
    int direct;             // 0 automatic, 1 on, 2 off
    int ell_prune;          // 0/1: windows that cost more than the panel residual are given up, 2 = never
    int value_map;          // 1: keep the slot maps of the value streams (ehyb_plan_set_values)
    int prune_pct;          // ell_prune threshold in per cent of the panel form's cost (110)
    int er_units1;          // panel form: work units aimed at, pass 1 / pass 2 (2048)
    int er_units2;
    int graph_compress;     // 0 automatic (on with symmetric pair storage), 1 on, 2 off, 3 on + a refinement on the rows themselves (twins may part)
    int balance;            // 0 automatic, 1 entries, 2 rows
    int req_margin;         // 0 default, -1 none, > 0 as given
    int sym_slack_permille; // 30
    int xcd_map;            // 1 on, 2 off
    int graphs;             // 1 on, 2 off
    int er_sums;            // 1 DPP scan, 2 LDS words
    int er_panel_threads;   // 0 automatic, 512, 1024
    int er_queue;           // 0 automatic (queues from six items per resident workgroup up), 1 per-XCD work queues with stealing, 2 one workgroup per item
    int symbolic;           // where the panel form is built by ehyb_plan_create[_segs]: 1 host, 2 device (default)
    int cg_fused_dot;       // 1 on (default), 2 off
    int ell_alternate;      // 0 automatic (streams that do not fit the Infinity Cache, ell_nt 1-3), 1 on, 2 off
    int row_split;          // panel form: no row block of pass 2 straddles this row (0 = none)
    int col_map;            // host builder: 1 per-thread column look-up arrays where they fit (default), 2 sorted lists + binary search
    int er_nt;              // panel form, pass 2 reads past the caches: 0 by size, 1 always, 2 never
    int ell_nt;             // window kernel, value stream past the caches: 4 (default) / 5 all but a fixed set of slabs that stays in the Infinity
                            // Cache (spread over a segment / its first slabs), 3 all but the end of an alternating walk, 1 every slab, 2 never
    int ell_keep;           // ell_nt 4 / 5: the share of the slabs in that set, per mille; 0 = from the cache's size (ehyb_hip.hip)
    int ell_triples;        // 1: the device holds one column base per node triple where a slab allows it (col_triples.h), 2: the host's words
    int val_f32;            // 1: the device holds the value streams in fp32 (device_values_f32), 0: fp64
};
Config resolve_config(const ehyb_config* cfg);

constexpr int kSlabRows = EHYB_SLAB_ROWS;  // one row per lane
constexpr int kNumCU = 256;                // MI355X: 8 XCD x 32 CU
constexpr int kErBins = 4;                 // lanes per residual segment: 4, 16, 64, 64(atomic)

// ---------------------------------------------------------------- layout
// Host image of the EHYB layout.  Device arrays mirror these one to one.
struct HostLayout {
    int n_cols = 0;       // dimension of the matrix (length of x)
    int row_begin = 0;    // rows covered: [row_begin, row_end)
    int row_end = 0;
    int n_parts = 0;
    int lds_doubles = 0;  // max over partitions of win_len + halo_len

    // per partition
    std::vector<int32_t> part_boundary;  // [n_parts+1] first row
    std::vector<int32_t> win_len;        // [n_parts] contiguous window length (from part start)
    std::vector<int32_t> halo_ptr;       // [n_parts+1]
    std::vector<int32_t> halo_cols;      // gathered columns (global ids), ascending per part
    std::vector<int64_t> part_nnz_ell;   // [n_parts] stored ELL entries of the partition without padding (host only)

    // per slab (64 rows, one wave)
    std::vector<uint32_t> slab_pair_ptr;  // [n_slabs+1] prefix of (width/2)
    std::vector<int32_t> slab_row;        // [n_slabs]
    std::vector<int32_t> slab_part;       // [n_slabs]

    // ELL payload: element (pair p, lane l, half h) at ((pair_ptr[s]+p)*64 + l)*2 + h
    // Column indices are stored once per *group* of lanes with identical column lists:
    // word (pair p, group g) at slab_col_ptr[s] + p*G_s + g holds two 16-bit window-local columns.
    BigVec<double> ell_val;
    BigVec<uint32_t> ell_col;
    std::vector<uint32_t> slab_col_ptr;  // [n_slabs+1] prefix of pairs*groups
    std::vector<uint8_t> lane_group;     // [n_slabs*64]
    std::vector<uint32_t> slab_meta;     // [n_slabs*kSlabWords] slab records (SlabField, SlabShape below)

    // work items (kItemWords each, ItemField below): a run of slabs of (nearly) equal cost; it is cut into
    // segments where it crosses a partition boundary
    std::vector<int32_t> items;
    // segments (kSegWords each, SegField below): the slabs of an item that share one partition's window
    std::vector<int32_t> segs;

    // residual (CSR segments sorted by length, descending)
    std::vector<int64_t> er_seg_ptr;  // [n_seg+1]
    std::vector<int32_t> er_seg_row;  // [n_seg] row | 0x80000000 if the row is split
    std::vector<int32_t> er_col;
    std::vector<double> er_val;
    int32_t er_bins[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // [3] = number of segments
    std::vector<int32_t> er_blocks;                 // {seg_lo, seg_hi, lanes per segment, 0} per block
    // inline form: the residual is also stored as extra pairs behind each slab's ELL pairs
    // (slab_meta word 3, bits 8..15) and the ELL launch multiplies it
    bool inline_er = false;
    // symmetric pair storage: bit 15 of a 16-bit column = "also add value * x[row] to row `column`";
    // the accumulators of a partition's rows live in LDS behind the window (yacc_doubles of them)
    bool sym = false;
    int yacc_doubles = 0;
    std::vector<uint16_t> slab_lrow;  // [n_slabs*64] sym only: image-local row of every lane (0xFFFF: none)

    // direct shape (small matrices): every row in the residual, the residual kernel ASSIGNS y, no ELL launch
    bool direct = false;

    // panel form of a large residual (er_panel.cpp): two streaming passes instead of gathers from global memory
    bool er_panel = false;
    int pb_panel_cols = 0;            // columns per x panel (LDS of pass 1)
    int pb_rows_max = 0;              // rows of the largest row block (LDS of pass 2)
    int64_t pb_partials = 0;
    int64_t pb_bytes = 0;             // bytes both passes move per multiply
    int64_t pb_padded = 0;            // length of pb_val / pb_col / pb_dst / pb_src (panels padded to multiples of 64 entries)
    std::vector<double> pb_val;       // pass-1 order, panels padded to multiples of 64 entries
    std::vector<uint16_t> pb_col;     // column - panel start
    std::vector<uint32_t> pb_dst;     // partial slot; 0xFFFFFFFF = padding
    std::vector<int32_t> pb_units1;   // {first column, columns, first entry, end entry}: a stretch of one panel's entries
    std::vector<int32_t> pb_items1;   // {first unit, end unit}: one pass-1 workgroup's work, a run of units of equal total cost
    std::vector<uint16_t> pb_row;     // per partial: row - first row of its block
    std::vector<int32_t> pb_units2;   // {first partial, end partial, first row, rows}; rows < 0: the block ASSIGNS y (-rows rows)
    // Partitions that went to the residual whole (their window did not pay, plan.cpp) have no ELL work at all:
    // with pb_assign their rows get y from pass 2 alone (row blocks that assign instead of add, also where no
    // partial arrives), the ELL launch skips them, and their slabs cost its work items nothing.
    bool pb_assign = false;
    std::vector<uint8_t> part_windowless;  // [n_parts] host only
    // Column segments (multi-GPU, ehyb_plan_create_host_segs): [0] = 0 < ... < [n] = n_cols; a panel never straddles a
    // boundary, and the pass-1 items of segment s are pb_seg_item[s] .. pb_seg_item[s+1] -- the multiply can then run
    // segment by segment as the x entries of each arrive (ehyb_spmv_part).  Empty = one segment.
    std::vector<int32_t> col_seg_first;
    std::vector<int32_t> pb_seg_item;
    // what pass 1 streams in place of pb_col + pb_dst (derived from them by encode_panel_slots, not stored in plan files)
    std::vector<uint16_t> pb_colf;    // column | head flag (bit 15) | jump flag (bit 14)
    std::vector<uint32_t> pb_chunk;   // per 64-entry chunk: its first jump
    std::vector<uint32_t> pb_jump;    // per jump: slot - pieces before it in its chunk

    // slot maps (cfg.value_map): entry of the source matrix every slot of a value stream was filled from, -1 = padding
    BigVec<int32_t> ell_src;          // like ell_val
    BigVec<int32_t> ell_src2;            // like ell_val, sym only: the mirror entry the slot also stands for, else -1
    std::vector<int32_t> er_src;      // like er_val
    std::vector<int32_t> pb_src;      // like pb_val
    int64_t src_entries = 0;          // entries of the source matrix (length ehyb_plan_set_values expects)

    // Panel form left to the device (ehyb_plan_create with cfg.symbolic = 2, er_panel_dev.hip): the residual entries in
    // ROW order, as the layout builder met them -- either views into the caller's matrix (every entry is residual: R-MAT)
    // or the builder's own row-order copies.  `pending` until the device has dealt them out; after that the pb_*
    // streams live on the device alone until somebody asks for them (pb_host_missing, materialize_panel_host).
    struct Deferred {
        bool pending = false;
        int64_t nnz_er = 0;
        std::vector<int64_t> er_rp;   // [rows + 1] first residual entry of every row
        const int32_t* col = nullptr;
        const double* val = nullptr;
        const int32_t* src = nullptr; // source entry of every residual entry; null: src_base + its position
        int64_t src_base = 0;
        bool want_src = false;        // cfg.value_map: keep the slot map of pb_val
        std::vector<int32_t> own_col, own_src;
        std::vector<double> own_val;
    } deferred;
    bool pb_host_missing = false;

    ehyb_stats stats{};
};

// Named views of the packed records above, host side (the kernels decode the same words in ell_device.h).
// The 16-byte slab record the window kernel reads:
constexpr int kSlabWords = 4;
enum SlabField { SLAB_PAIR_PTR, SLAB_COL_PTR, SLAB_ROW, SLAB_SHAPE };
// its word SLAB_SHAPE = pairs << 16 | er_pairs << 8 | relative << 7 | groups - 1
struct SlabShape {
    uint32_t pairs;     // ELL pairs per lane (the slab's width / 2)
    uint32_t er_pairs;  // inline residual pairs per lane behind them (HostLayout::inline_er)
    uint32_t groups;    // groups of lanes that share their column words, 1..64
    bool relative;      // the columns are stored relative to the lane's own row
};
inline uint32_t pack_slab_shape(uint32_t pairs, uint32_t er_pairs, bool relative, uint32_t groups)
{
    return (pairs << 16) | (er_pairs << 8) | (relative ? 0x80u : 0u) | (groups - 1);
}
inline SlabShape unpack_slab_shape(uint32_t w) { return {w >> 16, (w >> 8) & 0xFF, (w & 0x3F) + 1, (w & 0x80u) != 0}; }
// work item: its segments, its slabs, and its residual segments by length bin (64 lanes per segment for >= 128 entries, 16 for 17..127, 4 below)
constexpr int kItemWords = 8;
enum ItemField { ITEM_SEG_BEGIN, ITEM_SEG_END, ITEM_SLAB_BEGIN, ITEM_SLAB_END, ITEM_ER_BEGIN, ITEM_ER_B64, ITEM_ER_B16, ITEM_ER_END };
constexpr int kSegWords = 8;
enum SegField { SEG_PART, SEG_SLAB_BEGIN, SEG_SLAB_END, SEG_HALO_COUNT, SEG_ROW_BEGIN, SEG_ROW_END, SEG_WIN_LEN, SEG_HALO_BEGIN };

// The host's share of the panel builder (er_panel.cpp), common to the host and the device route
struct PanelGeometry {
    int W = 0;
    std::vector<int32_t> seg_first;    // [segments + 1] column segments
    std::vector<int32_t> seg_panel0;   // [segments + 1] first panel of every segment
    std::vector<int32_t> panel_first;  // [panels + 1] first column of every panel
    std::vector<int32_t> rb_first;     // [row blocks + 1] first row of every row block of pass 2
    std::vector<uint8_t> row_assign;   // [rows] pb_assign only: the row's partition has no window
};
int panel_geometry(const Config& cfg, const HostLayout& L, const int32_t* cnt_row, int64_t nnz_er, PanelGeometry* G);
int64_t panel_pass1_items(const Config& cfg, const PanelGeometry& G, const std::vector<int64_t>& pstart, int64_t nnz_er, HostLayout* L);
void panel_finish(const PanelGeometry& G, const std::vector<int64_t>& rb_count, int64_t staged, int64_t padded, int64_t n_pieces, int64_t n_jumps,
                  HostLayout* L);

// What a caller of build_layout may ask for beyond the plain layout of the rows
struct LayoutOptions {
    // partitions (by their index in the layout's own partition list) whose rows go to the residual whole (plan.cpp decides)
    const std::vector<uint8_t>* part_to_er = nullptr;
    // multi-GPU: the rank's own columns, where the rows laid out are only a sample of the rank's (-1: the rows themselves)
    int local_lo = -1, local_hi = -1;
    // a panel form that is certain (cfg.er_mode = 2, or partitions given up) is left to the device --
    // out->deferred.pending, no CSR segments either; the views of out->deferred may point into *m
    bool defer_panel = false;
    // stop after the windows and slab widths (plan.cpp's sample): out->stats holds the entry counts, nothing is filled
    bool stats_only = false;
};
int build_layout(const matrixCOO* m, int row_begin, int row_end, const Config& cfg, HostLayout* out, const LayoutOptions& opt = LayoutOptions());
int create_host_plan(const matrixCOO* m, int row_begin, int row_end, const ehyb_config* cfg, int n_col_segs, const int* col_seg_first,
                     bool defer_panel, ehyb_plan** plan);                         // plan.cpp
int spmv_xy_partials(const ehyb_plan* P);            // ehyb_hip.hip: y = A x with x . y on the side -- partials it leaves, 0 = not this plan
int spmv_xy(ehyb_plan* P, const double* x, double* y, void* stream, double* xy_partials);
int build_panel_on_device(ehyb_plan* P);              // er_panel_dev.hip: P->host.deferred -> the d_pb_* arrays
int materialize_panel_host(ehyb_plan* P);             // er_panel_dev.hip: pb_* streams of a device-built plan back to the host
int build_panel_residual(const Config& cfg, HostLayout* L);  // er_panel.cpp; reads the CSR residual of *L
void encode_panel_slots(HostLayout* L);                      // er_panel.cpp; pb_col + pb_dst -> pb_colf, pb_chunk, pb_jump
bool sym_storage_suits(const matrixCOO* m);  // spmvGPuEHYB's own choice of the storage (plan.cpp)
int windows_that_do_not_pay(const HostLayout& H, int pct, std::vector<uint8_t>* to_er, int64_t* entries_moved);  // plan.cpp

// ---------------------------------------------------------------- widths (host arithmetic; the launches and the transcoder of the column words share it)
constexpr int kSpmmMaxK = 4;  // widest window / residual kernel built

// Doubles of the LDS x image per vector (the window, with symmetric pair storage the y accumulators behind it); the kernel's
// slab counter sits right behind the image(s).
inline int ell_win_cap(const HostLayout& H) { return (H.lds_doubles + 1) / 2 * 2; }
// Dynamic LDS of a window launch for k columns: k images and the slab counter
inline size_t ell_lds_bytes(const HostLayout& H, int k) { return (size_t)k * ell_win_cap(H) * 8 + 16; }

// Widest pass of ehyb_spmm on a plan (ehyb_spmm_max_k; the rule is stated in include/ehyb.h): what fits the 160 KiB of LDS -- k
// window images and the slab counter; for a panel-form residual also k panel images and the hand-over word of pass 1, and k
// accumulators per row of the largest row block of pass 2.
inline int spmm_width(const HostLayout& H)
{
    if (H.deferred.pending) return 1;  // (the panel form is not built yet: nothing can be multiplied)
    int64_t k = kSpmmMaxK;
    if (H.er_panel && H.pb_panel_cols > 0 && H.pb_rows_max > 0)
        k = std::min<int64_t>(k, std::min<int64_t>((EHYB_LDS_MAX_DOUBLES - 1) / H.pb_panel_cols, EHYB_LDS_MAX_DOUBLES / H.pb_rows_max));
    const int64_t cap = ell_win_cap(H);
    if (!H.direct && cap > 0) k = std::min<int64_t>(k, ((int64_t)EHYB_LDS_MAX_DOUBLES * 8 - 16) / (8 * cap));
    return (int)std::max<int64_t>(1, k);
}

// One window kernel carries no triple arm (ell_device.h: it spilled with both forms of the column words in it): K columns from this
// width up with symmetric pairs AND an inline residual.  A plan that can launch it keeps the host's column words on the device
// (col_triples.cpp: plan_keeps_pair_words); launch_window refuses that kernel on a plan with coded slabs.
// cfg.val_f32: the value streams as the device holds them -- every fp64 value rounded to nearest-even (the host's default
// rounding mode; beyond the fp32 range +-inf, fp32 subnormals kept, NaN stays NaN).  common.cpp, on the OpenMP threads of the scope
// the caller opened.
void device_values_f32(const double* src, size_t n, float* dst);
// the widest pass of ehyb_spmm on the plan: the fp32-value kernels are built one column wide
inline int plan_spmm_width(const ehyb_plan* P);
constexpr int kNoTripleArmK = 4;
static_assert(kNoTripleArmK <= kSpmmMaxK + 1, "a width no kernel is built for");
inline bool plan_keeps_pair_words(const HostLayout& H) { return H.sym && H.inline_er && spmm_width(H) >= kNoTripleArmK; }

// ---------------------------------------------------------------- partitioner
// *by_degree (may be null) = true: the parts are blocks of the degree order (EHYB_PART_DEGREE, or EHYB_PART_AUTO on a
// graph that does not coarsen) -- the caller should number the rows of a part in that order (degree_order)
int partition_graph(int n, const int64_t* xadj, const int* adjncy, const int* vwgt, int nparts,
                    int max_part_w, const Config& cfg, int* part, int64_t* edgecut, bool* by_degree = nullptr);
void degree_order(int n, const int64_t* xadj, std::vector<int>* order);
// the finest-level refinement of partition_graph alone, on a partition that exists: greedy boundary refinement, the hard cap, a polish
// (adjncy may hold self loops: they are skipped)
int refine_partition(int n, const int64_t* xadj, const int* adjncy, const int* vwgt, int nparts, int max_part_w, const Config& cfg, int* part,
                     int64_t* edgecut);

// Optional mt-metis backend: resolved at run time from the process image (weak symbol) --
// see INTEGRATION.md.  Returns false when not linked.
bool mtmetis_available();
int mtmetis_partition(int n, const int64_t* xadj, const int* adjncy, int nparts, int nthreads,
                      int* part, int64_t* edgecut);

// ---------------------------------------------------------------- misc
double wall_seconds();
// cfg.col_map: the host builders look columns up in ONE array over all columns per host thread where that array is small enough to be
// looked into at random cheaply -- 16 MiB, 4 M columns (the bench matrix: 3.7 MB) -- and fall back to sorted lists / hash tables of a
// partition's own candidates beyond (R-MAT 2^24: 64 MiB per thread, first touched and zeroed per thread and per window sample, cost the
// plan 0.36 s, and a partition's 10^5 candidates scattered over it miss the caches and the TLB every time).
inline bool col_map_fits(const Config& cfg, int n_cols) { return cfg.col_map != 2 && (int64_t)n_cols * 4 <= (int64_t(16) << 20); }
void prefault(void* p, size_t bytes);  // fresh pages of an array about to be filled, mapped in one sweep instead of a trap per page
template <class T, class A>
inline void prefault_vector(std::vector<T, A>& v, size_t n)  // reserve + prefault: the resize / push_backs that follow touch mapped pages
{
    v.reserve(n);
    prefault((void*)v.data(), n * sizeof(T));
}
int default_host_threads();  // OpenMP threads when cfg.host_threads is 0: capped by affinity and cgroup quota
// The library's OpenMP regions run on cfg.host_threads (or the default above) threads; the caller's
// own OpenMP setting (the calling thread's nthreads-var) is put back when the entry point returns.
struct OmpScope {
    int saved;
    explicit OmpScope(int want);
    explicit OmpScope(const ehyb_config* cfg) : OmpScope(cfg ? cfg->host_threads : 0) {}
    ~OmpScope();
    OmpScope(const OmpScope&) = delete;
    OmpScope& operator=(const OmpScope&) = delete;
};
inline uint64_t splitmix64(uint64_t& s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The kernel tables of ehyb_hip.hip (EHYB_KERNELS_*: window, panel passes, CSR residual) and the rows a plan's launch log has
// room for per table (ehyb_debug_kernel_table refuses a table that outgrew it: 96, 22 and 10 rows today).
constexpr int kKernelTables = 3;
constexpr int kKernelTableCap = 128;
// The table of the transposed multiply (ehyb_spmv_t.hip, ehyb_debug_kernel_table_t: 7 rows) has a launch log of its own
constexpr int kKernelTableTCap = 8;
int spmv_t_opt_in_lds();  // ehyb_spmv_t.hip: the transposed window kernels opt in to the full LDS (ehyb_plan_upload)

}  // namespace ehyb

// The plan object behind the opaque handle.
struct ehyb_plan {
    ehyb::Config cfg;
    ehyb::HostLayout host;
    bool uploaded = false;
    bool d_triples = false;  // the device's column words hold triple-coded slabs (col_triples.h)
    int device = -1;
    std::vector<int32_t> perm;  // reorderList a cached plan was saved with (ehyb_plan_load), else empty
    // device arrays (same names as HostLayout; what the kernels do not read stays on the host)
    int32_t* d_halo_cols = nullptr;
    int32_t* d_segs = nullptr;
    double* d_ell_val = nullptr;
    uint32_t* d_ell_col = nullptr;
    uint8_t* d_lane_group = nullptr;
    uint32_t* d_slab_meta = nullptr;
    int32_t* d_items = nullptr;
    int32_t* d_item_map = nullptr;      // ehyb_plan_tune: item of every ELL workgroup (null: the built-in order)
    std::vector<int32_t> item_map;      // its host copy (a property of the device the plan was tuned on: not saved)
    std::vector<int32_t*> retired_item_maps;  // maps a later ehyb_plan_tune replaced: kept until the plan goes (captured graphs)
    int64_t* d_er_seg_ptr = nullptr;
    int32_t* d_er_seg_row = nullptr;
    int32_t* d_er_col = nullptr;
    double* d_er_val = nullptr;
    int32_t* d_er_blocks = nullptr;
    uint16_t* d_slab_lrow = nullptr;
    double* d_pb_val = nullptr;
    uint16_t* d_pb_colf = nullptr;
    uint32_t* d_pb_chunk = nullptr;
    uint32_t* d_pb_jump = nullptr;
    int32_t* d_pb_units1 = nullptr;
    int32_t* d_pb_items1 = nullptr;
    int* d_pb_queue = nullptr;          // pass 1 work queues: [16 k] items taken of XCD k's eighth, [128] workgroups gone
    uint16_t* d_pb_row = nullptr;
    int32_t* d_pb_units2 = nullptr;
    double* d_pb_partial = nullptr;  // [pb_partials] written by pass 1, read by pass 2: one multiply at a time per plan
    // slot maps on the device, uploaded by the first ehyb_plan_set_values
    int32_t* d_ell_src = nullptr;
    int32_t* d_ell_src2 = nullptr;
    int32_t* d_er_src = nullptr;
    int32_t* d_pb_src = nullptr;
    bool host_values_stale = false;  // the device values were refilled: the host copy no longer matches
    // direction of the next ELL launch's walk (cfg.ell_alternate), and of pass 1 of the panel residual: atomics, so that host
    // threads that multiply with one plan on their own streams (ELL-only plans: include/ehyb.h) each draw a direction
    std::atomic<int> launch_parity{0};
    std::atomic<int> panel_parity{0};
    // launch log (ehyb_debug_launched): one byte per row of the three kernel tables of ehyb_hip.hip, set by the launch that looked
    // the row up -- a relaxed byte store, no lock and no allocation on the launch path; every thread stores the same 1
    uint8_t launched[ehyb::kKernelTables][ehyb::kKernelTableCap] = {};
    void mark_launched(int which, size_t row)
    {
        if (row < (size_t)ehyb::kKernelTableCap) __atomic_store_n(&launched[which][row], (uint8_t)1, __ATOMIC_RELAXED);
    }
    // the same for the table of the transposed multiply (ehyb_debug_launched_t)
    uint8_t launched_t[ehyb::kKernelTableTCap] = {};
    void mark_launched_t(size_t row)
    {
        if (row < (size_t)ehyb::kKernelTableTCap) __atomic_store_n(&launched_t[row], (uint8_t)1, __ATOMIC_RELAXED);
    }
};
inline int ehyb::plan_spmm_width(const ehyb_plan* P) { return P->cfg.val_f32 == 1 ? 1 : spmm_width(P->host); }
