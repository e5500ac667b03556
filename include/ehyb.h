/*
 * ehyb.h -- C-ABI of the MI355X-native Explicit-Caching HYB (EHYB) fp64 SpMV.
 *
 * Plain C: pointers, sizes and an opaque plan handle; no C++ or torch types cross
 * this boundary.  One shared library (libehyb.so) exports everything declared here
 * and in spmv.h / reordering.h.  Each entry point names the reference interface it
 * stands in for (paths are into the reference repository).
 *
 *   reference symbol / code                         replaced by
 *   ---------------------------------------------   --------------------------------------
 *   spmvGPuEHYB                 spmv.cu:61-133      spmvGPuEHYB (spmv.h) = plan_create +
 *                                                   10 warm-ups + MAXIter x ehyb_spmv
 *   COO2EHYB + helpers          convert.c:61-369    ehyb_plan_create_host (layout builder)
 *   cudaMallocTransDataEHYB     spmv.cu:6-60        ehyb_plan_upload
 *   matrixVectorEHYB[_small]    kernel.cu:490-552   ehyb_spmv / ehyb_spmv_phase
 *     kernelCachedBlockedELL*   kernel.cu:110-284     -> ehyb_ell_kernel   (HIP, gfx950)
 *     ER loop + vecReorderER    kernel.cu:169-194,69-77 -> ehyb_er_kernel  (HIP, gfx950)
 *     longRowKernel             kernel.cu:43-67       -> long segments of ehyb_er_kernel
 *   matrixReorder[_unsym]       reordering.c:41-378 ehyb_matrix_reorder (+ C++ names in
 *                                                   reordering.h)
 *   vectorReorder/vectorRecover reordering.c:380-391 ehyb_vector_reorder / _recover
 *   sizing heuristic            solver_test.c:53-77,158-182  ehyb_sizing
 *   matrixRead_sym/_unsym       solver_test.c:31-265 ehyb_mm_read (+ ehyb_x_glibc)
 *   MTMETIS_PartGraphKway       reordering.c:126-139,280-293  ehyb_partition_graph
 *                                                   (built-in multilevel k-way; an
 *                                                   mt-metis build can be plugged in,
 *                                                   see INTEGRATION.md)
 */
#ifndef EHYB_H
#define EHYB_H

#include <stdint.h>
#include <stddef.h>
#include "spmv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
typedef enum ehyb_status {
    EHYB_OK            = 0,
    EHYB_ERR_ARG       = 1,  /* null pointer, negative size, inconsistent matrixCOO   */
    EHYB_ERR_ALLOC     = 2,  /* host allocation failed                                */
    EHYB_ERR_HIP       = 3,  /* a HIP runtime call failed (message via ehyb_last_error) */
    EHYB_ERR_NO_DEVICE = 4,  /* no gfx950-capable device visible                      */
    EHYB_ERR_IO        = 5,  /* file missing / unreadable                             */
    EHYB_ERR_FORMAT    = 6,  /* Matrix Market content not supported or malformed      */
    EHYB_ERR_INTERNAL  = 7,  /* layout self-check failed (the reference exit()s here:
                                convert.c:122-125,226-263,287-303)                    */
    EHYB_ERR_STATE     = 8   /* plan not uploaded / wrong call order                  */
} ehyb_status;

/* Thread-local text of the last failure ("" if none). Never NULL. */
const char* ehyb_last_error(void);
/* "ehyb-mi355x <version> gfx950" */
const char* ehyb_version(void);

/* ------------------------------------------------------------------ config */
enum { EHYB_WINDOW_DEFAULT = 0, EHYB_WINDOW_REFERENCE = 1, EHYB_WINDOW_HALO = 2 };
enum { EHYB_PART_AUTO = 0, EHYB_PART_CONTIGUOUS = 1, EHYB_PART_MULTILEVEL = 2, EHYB_PART_MTMETIS = 3,
       EHYB_PART_DEGREE = 4 /* rows in order of falling degree (row + column entries), cut into equal blocks: what
                               EHYB_PART_AUTO falls back to on graphs a k-way partitioner finds nothing to cut in
                               (power-law: R-MAT) -- the hub columns then share x panels and the hub rows share row
                               blocks of the panel-form residual (er_panel.cpp) */ };

#define EHYB_LDS_MAX_DOUBLES 20480   /* 160 KiB of LDS per workgroup on gfx950 */
#define EHYB_SLAB_ROWS       64      /* one row per lane of a wave64           */

/* Which shape for which size (round 2, NOTEBOOK.md 2: fem3d with 3 unknowns per node, ~78 entries per
 * row, microseconds per SpMV: direct / window with every entry stored / symmetric pair storage):
 *    24,576 rows   5.6 /  8.8 /  9.4        65,535 rows  14.8 / 16.5 / 13.1
 *    32,766 rows   7.2 /  9.3 /  9.7        81,918 rows  17.4 / 17.4 / 13.8
 *    40,959 rows   9.5 / 10.6 /  9.8        98,304 rows  20.6 / 19.7 / 15.0
 *    49,152 rows  11.6 / 14.3 / 11.1       131,070 rows  25.9 / 21.9 / 15.7
 * Symmetric pair storage (one workgroup per partition) needs enough partitions to fill the 256 CUs: it
 * pays from about 45,000 rows; callers that pick the storage from the matrix's symmetry (matrixReorder,
 * spmvGPuEHYB, solver_test, bench.py) use EHYB_SYM_MIN_ROWS.  Below, and for unsymmetric matrices up to
 * EHYB_DIRECT_MAX_ROWS, the direct shape (cfg.direct: no window, one small launch) is the fastest. */
#define EHYB_SYM_MIN_ROWS 45056
#define EHYB_DIRECT_MAX_ROWS 81920

/* OpenMP threads the host builder uses when cfg.host_threads is 0: what OpenMP would take, capped by
 * the CPUs the process may really use (affinity mask, cgroup CPU quota). */
int ehyb_host_threads(void);

/*
 * Tuning knobs.  They take the place of the reference's compile-time constants
 * (kernel.h:20-28: warpSize 32, smSize 82, maxSharedMem 93 KiB, threadELL 1024,
 * threadLongVec 512).  Zero in any field means "use the default".
 */
typedef struct ehyb_config {
    int32_t lds_doubles;   /* x-window capacity per workgroup (own rows + halo), <= 20480 */
    int32_t part_rows;     /* upper bound of rows per partition, <= lds_doubles           */
    int32_t threads;       /* ELL workgroup size: multiple of 64, <= 1024                 */
    int32_t window_mode;   /* EHYB_WINDOW_REFERENCE: window = [start, start+cache) exactly
                              as convert.c:247; EHYB_WINDOW_HALO: own rows + the most
                              referenced outside columns gathered into LDS                */
    int32_t items_per_cu;  /* ELL work items per CU (load-balance granularity)            */
    int32_t partitioner;   /* EHYB_PART_*                                                 */
    int32_t er_seg_len;    /* residual rows longer than this are split into segments      */
    int32_t host_threads;  /* OpenMP threads of the host builder (0 = runtime default)    */
    int32_t verbose;       /* 1: print the reference's format metrics (toER, waste, ...)  */
    int32_t seed;          /* partitioner tie-breaking seed (deterministic per seed)      */
    int32_t n_top;         /* top-level row blocks (one per GPU); 0/1 = single GPU        */
    int32_t er_threads;    /* residual workgroup size                                     */
    int32_t ell_variant;   /* how ELL slabs reach the waves of a workgroup: 0/1 = LDS counter (default),
                              3 = static round-robin (A/B arm)                                   */
    int32_t col_sharing;   /* 0/1 = rows with the column list of the row above share its indices, 2 = off */
    int32_t fuse_er;       /* residual placement: 0 = automatic (inside the ELL launch iff it holds < 0.2 %
                              of the entries), 1 = always inside (single GPU only), 2 = own launch     */
    int32_t cap_split;     /* 0/1 = bisect partitions whose halo overflows the window (reorder step), 2 = off */
    int32_t hub_rule;      /* 0/1 = rows that would pad their slab by > 25 % go to the residual whole
                              (the reference's long-row intent, convert.c:92-101), 2 = off          */
    int32_t sym_pairs;     /* symmetric pair storage (halo window): an in-partition pair a_ij == a_ji is stored
                              once; the owning lane adds a_ij*x_j to its own row and a_ij*x_i to row j's
                              accumulator in LDS (ds_add_f64), so one value read serves two entries.  One
                              workgroup per partition; ehyb_sizing makes nParts a multiple of 256 and the
                              window the whole 160 KiB (own rows twice -- x image and accumulators -- plus halo).  Set it BEFORE reading/generating/reordering the matrix (the
                              partition sizes depend on it).  Results do not depend on the matrix being
                              symmetric (entries without an equal partner stay as they are), but the order
                              of the LDS adds varies from run to run (last-bit differences).
                              1 = on -- what solver_test and bench.py choose for symmetric inputs of at
                              least EHYB_SYM_MIN_ROWS rows; 0/2 = off */
    int32_t part_boundary_cap; /* ints the caller's matrixCOO.partBoundary can hold.  ehyb_matrix_reorder may end
                              with MORE partitions than m->nParts asked for (partitions whose halo overflows the
                              window are bisected, cap_split; two-level partitions, n_top > 1) and writes
                              nParts+1 boundaries.  0 = unknown: exactly the m->nParts+1 entries of the reference
                              contract (spmv.h:31) -- then the partition count is never raised (no capacity
                              split; n_top > 1 fails with EHYB_ERR_ARG if it would need more).  Matrices
                              allocated by this library (ehyb_mm_read, ehyb_gen_*, ehyb_matrix_from_csr) hold
                              dimension+1 entries; the reference harness callocs `dimension`
                              (solver_test.c:42,146), which is what matrixReorder[_unsym] assume.          */
    int32_t er_mode;       /* form of a residual too large to ride inside the ELL launch: 1 = CSR segments
                              (ehyb_er_kernel: x gathered from global memory), 2 = panel form (two streaming passes,
                              x panels and y blocks in LDS: er_panel.cpp), 0 = automatic: the panel form from 2^21
                              residual entries up when the residual shows no locality (more than one distinct
                              128-byte line of x per two consecutive entries), else CSR segments            */
    int32_t er_panel_cols; /* panel form: columns per x panel staged in LDS (<= 16384 = 128 KiB, the default)          */
    int32_t er_block_rows; /* panel form: most rows of a y block accumulated in LDS (<= 16384, default 2048)          */
    int32_t direct;        /* small matrices: 0 = automatic (plans of at most EHYB_DIRECT_MAX_ROWS rows, single GPU,
                              plain storage, window sizing left at its defaults), 1 = on, 2 = off.  On: no LDS window at all -- every row is multiplied by
                              the row-segment kernel straight from global x (which sits in L2 at this size), one
                              launch of 256-thread workgroups, y assigned, not accumulated.  A 160 KiB window per
                              1024-thread workgroup is the wrong shape when the whole matrix is a few MB: the
                              reference has a small-matrix branch for the same reason (kernel.cu:197-284,
                              solver_test.c:56-69).                                                           */
    int32_t ell_prune;     /* with the residual in panel form: 0/1 = a partition whose LDS window costs more bytes and
                              L2 requests than the panel form would for its entries (padding, halo gathers: power-law
                              matrices) goes to the residual whole, 2 = never                                 */
    int32_t value_map;     /* 1 = the plan remembers, for every slot of its value streams, which entry of the matrix it
                              was filled from (4 B per stored value on the host, and on the device from the first
                              ehyb_plan_set_values on): the NUMERIC phase of the build can then be repeated on the
                              GPU for new values on the same pattern.  0 = off                                 */
    /* ---- tuning knobs of the A/B tools (tools/); every one of them used to be an environment variable of
       the library.  The library reads NO tuning variable from the environment any more (the one variable left,
       EHYB_MTMETIS_LIB, names a shared object to load the optional mt-metis backend from). */
    int32_t prune_pct;     /* ell_prune: a window is given up when it costs more than this share (per cent) of what
                              the panel form would cost for its entries; 0 = 110                                */
    int32_t er_units1;     /* panel form: work items (workgroups) pass 1 aims at (0 = one per 49,152
                              residual entries, between 512 and 4096)                                           */
    int32_t er_units2;     /* panel form: row blocks pass 2 aims at (0 = 2048)                                 */
    int32_t graph_compress;/* the k-way partitioner works on the compressed graph where rows come in groups with one column
                              list (the unknowns of a node): 0 = with symmetric pair storage only (plain storage runs 4 %
                              slower on such partitions, reorder.cpp), 1 = always, 2 = never, 3 = always, followed by one
                              refinement on the rows themselves (the groups may then be cut)                      */
    int32_t balance;       /* symmetric pair storage, what the partitions are balanced on: 0 = rows unless the row lengths
                              vary by more than 30 % (sigma/mean), 1 = entries, 2 = rows                         */
    int32_t req_margin;    /* entry-balanced partitions of a graded mesh: partitions asked for = nParts - margin; 0 =
                              max(2, nParts/64), -1 = no margin                                                   */
    int32_t sym_slack_permille; /* ehyb_sizing, symmetric pair storage: rows a partition may hold above the mean, in
                              1/1000 (0 = 30)                                                                     */
    int32_t xcd_map;       /* 0/1 = workgroup b takes the work item that gives every XCD one contiguous run of items
                              (plain storage; the panel form's pass 1: the units of one x panel on one XCD), 2 = items
                              in blockIdx order                                                                   */
    int32_t graphs;        /* 0/1 = the timed loop of ehyb_spmv_bench and the iterations of ehyb_cg/ehyb_pcg are replayed
                              from hipGraphs, 2 = plain launches (A/B, debugging)                                */
    int32_t er_sums;       /* panel form, pass 1: how the products of one row inside a 64-entry chunk are added up: 0/1 =
                              segmented DPP scan in registers, 2 = ds_add_f64 into per-wave LDS words (round 2's way) */
    int32_t er_panel_threads; /* panel form, pass 1: workgroup size, 512 or 1024 (0 = automatic)                 */
    int32_t er_queue;      /* panel form, pass 1: 2 = one workgroup per item; 1 = one resident round of workgroups takes the items from
                              per-XCD queues, an XCD whose own eighth is used up helping the one with the most left (the 8 XCDs do not
                              stream equally fast), and a workgroup that takes the next item of the SAME panel does not stage it again;
                              0 = automatic: the queues from six items per resident workgroup up (R-MAT 2^24, 2,700 items: 574 -> 544 us;
                              2^22, 770 items: 132 -> 138 us, so not there)                                                    */
    int32_t symbolic;      /* ehyb_plan_create / ehyb_plan_create_segs (the calls that build AND upload): where the panel form
                              of a residual is built when it is certain to be used (R-MAT: every partition given up, or
                              er_mode = 2).  0/2 = on the DEVICE, from the entries in row order (radix sort by panel, row,
                              column; scans for the partial sums and their slots): the arrays are the host builder's, entry
                              for entry, where the rows arrive in column order; 1 = on the host.  ehyb_plan_create_host never
                              leaves anything to the device                                                        */
    int32_t cg_fused_dot;  /* ehyb_cg / ehyb_pcg: 0/1 = p . (A p) is left by the multiply itself where the plan multiplies in one
                              window launch (one vector kernel fewer per iteration), 2 = always the separate dot kernel (A/B) */
    int32_t ell_alternate; /* successive multiplies of a plan walk the slabs of every partition in alternating directions, so that a
                              launch starts with what the one before it left in the 256 MB Infinity Cache (a solver multiplies with
                              the same matrix again and again): 0 = where the plan's stream is larger than that cache and at most
                              8 GB (a smaller one stays resident anyway, of a far larger one the cache holds too little to pay for
                              the walk from the short slabs up) and cfg.ell_nt is 1, 2 or 3 -- the fixed set of ell_nt = 4 / 5 is the
                              same for both directions, and such a plan measured 1-1.5 us faster first to last --, 1 = always,
                              2 = never (always first to last).  With more work items
                              than resident workgroups the items are taken from the far end as well.  Pass 1 of the panel
                              residual alternates the same way                                                        */
    int32_t row_split;     /* panel form, multi-GPU: a row block of pass 2 never straddles this row (0 = none).  The rows from it on
                              are the FOREIGN rows of a rank -- partial sums it computes for other ranks from its own x entries
                              (dist.py: exchange "cover") -- and ehyb_spmv_part can close them early (EHYB_PART_LAST_FOREIGN), so
                              that they travel while the rank's own rows are still being multiplied                       */
    int32_t col_map;       /* host builder, how a partition finds the window place of an outside column: 0/1 = in a look-up array over the
                              columns, one per host thread (matrices of up to 4 M columns: 16 MiB per thread), 2 = in the sorted list
                              of the window's outside columns by binary search (A/B; the way for larger inputs).  The layouts are
                              the same array for array                                                                  */
    int32_t er_nt;         /* panel form, pass 2: the partial sums and their row words are read with the non-temporal hint (past the caches):
                              0 = where they are more than half the 256 MB Infinity Cache (10 B per partial sum), 1 = always, 2 = never (A/B) */
    int32_t ell_nt;        /* the window kernel reads its value stream (read once per multiply) with the non-temporal hint, past the caches,
                              all but a share that the 256 MB Infinity Cache is to keep for the next multiply (none where the whole stream
                              fits that cache: plain loads throughout).  0/4 = all but a FIXED set of slabs, the same in every launch
                              whatever its walk direction, spread evenly over the slabs of every partition: after the first launch the set
                              is resident and nothing evicts it; 5 = the same with the set at the start of every partition (A/B);
                              3 = all but the END of an alternating walk, which the next launch reads first (round 4; every slab where
                              the walk does not alternate); 1 = every slab, 2 = never (rounds 1-3).  The result never depends on it   */
    int32_t ell_keep;      /* ell_nt = 4 / 5: the share of a partition's slabs in that set, per mille (1..1000).  0 = automatic: what the
                              256 MiB cache holds beside the bytes the launch re-reads and writes with plain accesses (column words,
                              lane maps, slab records, x, y), times a safety factor; all of a stream that fits whole       */
    int32_t ell_triples;   /* the window kernel's column words ON THE DEVICE: 0/1 = a slab whose column lists are node triples c, c+1,
                              c+2 (three unknowns per node) holds one 16-bit base per triple, two per word -- a third of the words
                              of such a slab; ehyb_plan_upload transcodes, the host layout (EHYB_ARR_ELL_COL, EHYB_ARR_SLAB_META,
                              stats, plan files) is the same either way; 2 = the host's words as they are (A/B).  With every x
                              finite the result does not depend on it (ehyb_plan_device_cols)                       */
    int32_t val_f32;       /* 1 = the DEVICE holds every value stream of the plan in fp32 (half the bytes of the window kernel's
                              largest stream): each value is the fp64 value rounded to nearest-even by ehyb_plan_upload (out of
                              range: +-inf; fp32 subnormals kept; NaN stays NaN; a pair a_ij == a_ji stays a pair), converted back
                              to fp64 right after its load; x, y, the LDS window and every sum stay fp64.  The host layout
                              (EHYB_ARR_ELL_VAL, EHYB_ARR_ER_VAL), stats, the slot maps and plan files are the same either way
                              (ehyb_plan_device_values_f32).  Not for a residual in panel form, stamped launches, ehyb_plan_tune
                              or ell_variant = 3 (EHYB_ERR_ARG); ehyb_spmm_max_k is 1.  0 = off (default): fp64 values      */
    int32_t reserved[18];  /* zero; keeps sizeof(ehyb_config) = 260 bytes when knobs are added                  */
} ehyb_config;

void ehyb_config_default(ehyb_config* cfg);
/* *out = *in with every "0 = default" field replaced by the value the library will use given the
 * other fields (window and partition sizes depend on window_mode and sym_pairs).  in may be NULL
 * (all defaults) and may alias out. */
void ehyb_config_resolve(const ehyb_config* in, ehyb_config* out);

/* ------------------------------------------------- host pre-step (a-7, a-9) */

/*
 * Partition/window sizing for an n-row matrix: the MI355X re-derivation of
 * solver_test.c:53-77 / 158-182 (82 SMs x 93 KiB -> 256 CUs x 160 KiB, wave64).
 * Outputs may be NULL.  vectorCacheSize is the window the partitions are sized for,
 * kernelPerPart the number of work items one partition is cut into.
 */
int ehyb_sizing(int dimension, const ehyb_config* cfg,
                int* nParts, int* vectorCacheSize, int* kernelPerPart);

/*
 * k-way partition of an undirected graph in CSR form (xadj has n+1 entries; adjncy may
 * contain self loops, they are ignored).  Stands in for MTMETIS_PartGraphKway as called
 * at reordering.c:126-139 / 280-293 (unit vertex weights, ubvec 1.001): every part gets
 * at most max_part_rows vertices (<= 0: ceil(1.001*n/nparts)).  part[v] in [0,nparts).
 * If vwgt is non-NULL parts are balanced on it instead (used for the per-GPU blocks).
 */
int ehyb_partition_graph(int n, const int64_t* xadj, const int* adjncy, const int* vwgt,
                         int nparts, int max_part_rows, const ehyb_config* cfg,
                         int* part, int64_t* edgecut);

/*
 * In-place symmetric permutation P*A*P^T of a row-grouped COO matrix, as
 * matrixReorder (symmetric_pattern != 0, reordering.c:231-378) or matrixReorder_unsym
 * (== 0: the pattern is symmetrised first, reordering.c:41-228):
 *   - k-way partition into m->nParts parts (m->nParts and m->vectorCacheSize must be set,
 *     e.g. by ehyb_sizing);
 *   - new numbering: partition-contiguous, rows of a partition sorted by their number of
 *     in-partition entries, descending (reordering.c:312-334) -- ties keep the old order,
 *     so the permutation is deterministic here;
 *   - I/J/V are replaced (old arrays freed with free()), rowIdx/numInRow/numInRow2/
 *     partBoundary/reorderList are filled (reordering.c:335-362).
 * partBoundary and reorderList must be caller-allocated with >= nParts+1 and
 * >= dimension entries (the reference harness callocs `dimension` ints for both).
 */
int ehyb_matrix_reorder(matrixCOO* m, int symmetric_pattern, const ehyb_config* cfg);
/* The same with cfg.n_top > 1 row blocks (one per GPU): block_first[b] = first partition of block b,
 * block_first[n_top] = nParts (n_top+1 ints, caller-allocated; NULL: not wanted). */
int ehyb_matrix_reorder_blocks(matrixCOO* m, int symmetric_pattern, const ehyb_config* cfg, int* block_first);

/* v_rodr[list[i]] = v_in[i]  (reordering.c:380-384) */
void ehyb_vector_reorder(int dimension, const double* v_in, double* v_rodr, const int* list);
/* v[i] = v_rodr[list[i]]     (reordering.c:386-391) */
void ehyb_vector_recover(int dimension, const double* v_rodr, double* v, const int* list);

/*
 * A second matrix on the partitions of the first (host only).  a has been through ehyb_matrix_reorder; b has the same dimension
 * and is row-grouped in a's ORIGINAL numbering (a mass matrix on the mesh of a stiffness matrix, say).  b receives the symmetric
 * permutation new = a->reorderList[old] -- the convention of ehyb_vector_reorder --: its rows are grouped, the entries of a row
 * stand in rising new column order (equal columns keep their stored order, so the result is deterministic), I/J/V are replaced
 * (the old arrays freed with free()), rowIdx/numInRow/numInRow2/maxCol are refilled, and b takes a's nParts, vectorCacheSize and
 * kernelPerPart and copies of its partBoundary and reorderList into its own arrays (caller-allocated as for ehyb_matrix_reorder:
 * >= a->nParts + 1 and >= dimension ints).  ehyb_plan_create_host(b, ...) then builds a plan that walks a's partitions, as the
 * plan of an FSAI factor does.  Build it with cfg.sym_pairs off (2) unless b's rows are known to fit the windows sized for a:
 * the partitions were cut for a's pattern, not for b's.
 * EHYB_ERR_ARG: a null pointer, an incomplete b, different dimensions, a without partition data (nParts < 1, no partBoundary
 * spanning the rows, no reorderList, or one that is no permutation), a column of b outside the matrix.
 */
int ehyb_matrix_reorder_like(matrixCOO* b, const matrixCOO* a);

/* Cuts a reordered matrix into n_top runs of whole partitions with (nearly) equal entry counts:
 * part_of_block[b] = first partition of run b, n_top+1 entries.  A pure function of m (for matrices
 * whose two-level block boundaries were not kept; ehyb_matrix_reorder_blocks returns the real ones). */
int ehyb_top_boundary(const matrixCOO* m, const ehyb_config* cfg, int n_top, int* part_of_block);

/* ------------------------------------------------------------------- plan */
typedef struct ehyb_plan ehyb_plan;

/*
 * Build the EHYB layout on the host from a permuted matrix (COO2EHYB, convert.c:316-369).
 * No GPU needed.  Rows [row_begin,row_end) only (whole matrix: 0, dimension); the range
 * must start and end on partition boundaries.  The plan keeps no pointer into m.
 */
int ehyb_plan_create_host(const matrixCOO* m, int row_begin, int row_end,
                          const ehyb_config* cfg, ehyb_plan** plan);
/*
 * The same for a multi-GPU rank (no reference counterpart): the columns come in n_col_segs SEGMENTS,
 * col_seg_first[0] = 0 < ... <= col_seg_first[n_col_segs] = dimension, every start but the first even -- the rank's
 * own columns first, then the ghost columns in the order their x entries ARRIVE (one segment per exchange step).
 * A panel of the panel-form residual never straddles a boundary, so ehyb_spmv_part can multiply segment by segment
 * while later segments are still on the wire.  n_col_segs = 0: one segment (ehyb_plan_create_host).
 */
int ehyb_plan_create_host_segs(const matrixCOO* m, int row_begin, int row_end, const ehyb_config* cfg,
                               int n_col_segs, const int* col_seg_first, ehyb_plan** plan);
/* Allocate device arrays and copy the layout (cudaMallocTransDataEHYB, spmv.cu:6-60). */
int ehyb_plan_upload(ehyb_plan* plan);
/* Build + upload in one call, for the rows [0, dimension).  Unlike ehyb_plan_create_host followed by ehyb_plan_upload
 * this call may build on the DEVICE what it can (cfg.symbolic: the panel form of a residual without locality -- the
 * part of the symbolic phase that costs a power-law matrix seconds on the host).  Such a plan keeps the
 * pb_* streams on the device; ehyb_plan_host_array and ehyb_plan_save fetch them when asked. */
int ehyb_plan_create(const matrixCOO* m, const ehyb_config* cfg, ehyb_plan** plan);
/* The same for a row range and column segments (ehyb_plan_create_host_segs' arguments). */
int ehyb_plan_create_segs(const matrixCOO* m, int row_begin, int row_end, const ehyb_config* cfg, int n_col_segs, const int* col_seg_first,
                          ehyb_plan** plan);
void ehyb_plan_destroy(ehyb_plan* plan);

/*
 * On-disk cache of the pre-step: the reference repeats mt-metis and COO2EHYB on
 * every run (solver_test.c:369-382, spmv.cu:74).  ehyb_plan_save writes the host layout of a plan
 * together with the permutation that produced its matrix (reorder_list: n_cols ints, may be NULL)
 * and a key of the caller's choice -- ehyb_matrix_key(m) of the UNPERMUTED matrix is the intended
 * one.  ehyb_plan_load rebuilds a host plan (then ehyb_plan_upload); it fails with
 * EHYB_ERR_FORMAT when the file is damaged, from another version, or expect_key (non-zero) differs.
 * Same-machine cache, native byte order.
 */
uint64_t ehyb_matrix_key(const matrixCOO* m);
int ehyb_plan_save(const ehyb_plan* plan, const int* reorder_list, uint64_t matrix_key, const char* path);
int ehyb_plan_load(const char* path, uint64_t expect_key, ehyb_plan** plan, int* reorder_list);
/*
 * The content check ehyb_plan_load applies after its size checks, callable on any plan; host arithmetic only, no device.
 * EHYB_OK when every index a kernel or a host routine forms from the plan's arrays lies inside the array it indexes, for
 * every entry point a plan can be given to (ehyb_spmv, _phase, _walk, _part, ehyb_spmv_t, ehyb_spmm up to ehyb_spmm_max_k,
 * the solvers' multiplies, the transcoder of ehyb_plan_upload); else EHYB_ERR_FORMAT, and ehyb_last_error names the first
 * array, index and rule that failed.  It is about safety, not about the product: values may hold any bits, and a column
 * that stays inside its window cannot be told from another matrix.  The panel streams of a plan whose panel form was built
 * on the device are on the device alone and are not looked at.
 */
int ehyb_plan_check(const ehyb_plan* plan);

/* Format metrics; the first five are the ones the reference prints
 * (convert.c:140,310; spmv.cu:82). */
typedef struct ehyb_stats {
    int64_t nnz;            /* stored entries in the plan's rows                      */
    int64_t nnz_ell;        /* entries multiplied from the LDS window ("kernel calculation") */
    int64_t nnz_er;         /* entries in the residual ("toER")                       */
    int64_t ell_padding;    /* zero fill in the ELL slabs ("wasteElement")            */
    int64_t size_block_ell; /* stored ELL elements incl. padding ("sizeBlockELL")     */
    int64_t size_er;        /* stored residual elements ("sizeER")                    */
    int64_t rows_er;        /* rows with a residual part ("numOfRowER")               */
    int64_t er_segments;    /* residual segments (long rows are split)                */
    int64_t n_rows;         /* rows covered by the plan                               */
    int64_t n_cols;         /* dimension                                              */
    int64_t n_parts;
    int64_t n_slabs;
    int64_t n_items;        /* ELL workgroups per multiply                            */
    int64_t halo_cols;      /* gathered window entries over all partitions            */
    int64_t window_loads;   /* doubles staged into LDS per multiply (all items)       */
    int64_t bytes_format;   /* bytes the kernels must move per multiply in this format */
    int64_t bytes_alg;      /* 12*nnz + 4*(rows+1) + 8*cols + 8*rows      */
    int64_t max_row;        /* longest row                                            */
    int64_t lds_bytes;      /* dynamic LDS per ELL workgroup                          */
    int64_t col_words;      /* stored 4-byte column words (2 x 16 bit) after sharing  */
    int64_t er_inline;      /* stored inline-residual elements incl. padding; > 0: the residual rides in
                               the ELL launch (ehyb_spmv is one launch), see EHYB_ARR_SLAB_META */
    int64_t sym_pairs;      /* stored entries that stand for a symmetric pair (cfg.sym_pairs): nnz_ell counts
                               both entries of such a pair, size_block_ell one                          */
    int64_t bytes_format_ell; /* the part of bytes_format the ELL launch moves (an inline residual included);
                               the rest belongs to the residual launch                                   */
    int64_t er_partials;    /* > 0: the residual is stored in panel form; partial sums written by its first pass
                               and read by its second, per multiply                                    */
} ehyb_stats;
int ehyb_plan_stats(const ehyb_plan* plan, ehyb_stats* out);
/* Bytes of the window kernel's value stream that the plan reads with plain loads, i.e. leaves in the Infinity Cache (cfg.ell_nt,
 * cfg.ell_keep; for ell_nt = 3 the walk first to last); -1 = null plan.  Host arithmetic over EHYB_ARR_SLAB_META. */
int64_t ehyb_plan_resident_bytes(const ehyb_plan* plan);
/* The rule behind it, as the kernel applies it: is slab `pos` of a segment of `n` slabs in the set, for a share of
 * keep1024 / 1024 and shape 1 = spread (cfg.ell_nt = 4), 2 = block (5); 0 = the end of a walk (3), pos = the walk position. */
int ehyb_ell_slab_resident(int pos, int n, int keep1024, int shape);
/* The automatic share (cfg.ell_keep = 0) in 1/1024 for a value stream of value_bytes beside plain_bytes of other traffic. */
int ehyb_ell_auto_keep1024(int64_t value_bytes, int64_t plain_bytes);

/* Read-only views of the host layout, for invariant tests (i-iv). */
enum {
    EHYB_ARR_PART_BOUNDARY = 0, /* int32  [n_parts+1]  first row of each partition            */
    EHYB_ARR_WIN_LEN       = 1, /* int32  [n_parts]    contiguous window length               */
    EHYB_ARR_HALO_PTR      = 2, /* int32  [n_parts+1]  into HALO_COLS                         */
    EHYB_ARR_HALO_COLS     = 3, /* int32  [halo_cols]  global column of each gathered entry   */
    EHYB_ARR_SLAB_PAIR_PTR = 4, /* uint32 [n_slabs+1]  prefix of slab widths / 2              */
    EHYB_ARR_SLAB_ROW      = 5, /* int32  [n_slabs]    first row of the slab                  */
    EHYB_ARR_SLAB_PART     = 6, /* int32  [n_slabs]    partition of the slab                  */
    EHYB_ARR_ELL_VAL       = 7, /* double [size_block_ell]  [pair][lane][2]                   */
    EHYB_ARR_ELL_COL       = 8, /* uint32 [col_words] two 16-bit window-local columns per word:
                                   word (pair k, group g) of slab s at SLAB_COL_PTR[s] + k*G_s + g  */
    EHYB_ARR_ITEMS         = 9, /* int32  [n_items*8]  one workgroup's work: {seg_begin, seg_end, slab_begin,
                                   slab_end, er_begin, er_end_len>=128, er_end_len>16, er_end} -- a run
                                   of slabs of equal cost (cut into SEGS at partition boundaries) and
                                   the residual segments of its rows, longest first                 */
    EHYB_ARR_ER_SEG_PTR    = 10,/* int64  [er_segments+1]                                     */
    EHYB_ARR_ER_SEG_ROW    = 11,/* int32  [er_segments] bit31 set: row has several segments   */
    EHYB_ARR_ER_COL        = 12,/* int32  [size_er]    global column                          */
    EHYB_ARR_ER_VAL        = 13,/* double [size_er]                                           */
    EHYB_ARR_ER_BINS       = 14,/* int32  [8]  {0, -, -, er_segments, ...}                        */
    EHYB_ARR_SLAB_COL_PTR  = 15,/* uint32 [n_slabs+1]  prefix of pairs * groups               */
    EHYB_ARR_LANE_GROUP    = 16,/* uint8  [n_slabs*64] column-list group of every lane        */
    EHYB_ARR_SLAB_META     = 17,/* uint32 [n_slabs*4]  {pair_ptr, col_ptr, row, pairs<<16 | er_pairs<<8 | G-1}:
                                   what the kernel reads.  er_pairs > 0 only in the inline-residual form
                                   (stats.er_inline): behind the slab's `pairs` ELL pairs the value stream
                                   holds er_pairs more pairs [pair][lane][2], and behind its pairs*G column
                                   words the column stream holds [er pair][2][lane] GLOBAL 32-bit columns */
    EHYB_ARR_SEGS          = 18,/* int32  [n_segs*8]   {partition, slab_begin, slab_end, halo_count, first row,
                                   end row, win_len, halo_begin}: one LDS window staging each       */
    EHYB_ARR_PERM          = 19,/* int32  [n_cols]     reorderList stored with a plan that came from
                                   ehyb_plan_load (empty for plans built in this process)          */
    EHYB_ARR_SLAB_LROW     = 20,/* uint16 [n_slabs*64] symmetric pair storage only: the row every lane works on, as
                                   its place in the partition's LDS image (row - even(partition start));
                                   0xFFFF = no row.  The rows of a partition sit in its slabs longest first. */
    /* panel form of the residual (stats.er_partials > 0; the CSR arrays 10-13 describe the same entries) */
    EHYB_ARR_PB_VAL        = 21,/* double [entries, every panel padded to a multiple of 64]  pass-1 order: by column
                                   panel, inside a panel by (row, column); padding = 0.0                   */
    EHYB_ARR_PB_COL        = 22,/* uint16 same length: column - first column of the panel                  */
    EHYB_ARR_PB_DST        = 23,/* uint32 same length: partial sum the entry belongs to (entries of one row that are
                                   neighbours inside a 64-entry chunk share one); 0xFFFFFFFF = padding     */
    EHYB_ARR_PB_UNITS1     = 24,/* int32  [4*u1] pass-1 units {first column, columns, first entry, end entry}: a stretch of the
                                   entries of one panel (multiples of 64), staged once                     */
    EHYB_ARR_PB_ROW        = 25,/* uint16 [er_partials] row of the partial - first row of its row block; partials are
                                   numbered by (row block, panel, row)                                     */
    EHYB_ARR_PB_UNITS2     = 26,/* int32  [4*u2] pass-2 work units {first partial, end partial, first row, rows}    */
    /* slot maps of the value streams (cfg.value_map; empty otherwise): index into the V array of the matrix the plan
       was built from, -1 = padding.  What ehyb_plan_set_values gathers through on the device. */
    EHYB_ARR_ELL_SRC       = 27,/* int32  same length as ELL_VAL                                                      */
    EHYB_ARR_ER_SRC        = 28,/* int32  same length as ER_VAL                                                       */
    EHYB_ARR_PB_SRC        = 29,/* int32  same length as PB_VAL                                                       */
    EHYB_ARR_ELL_SRC2      = 30,/* int32  same length as ELL_VAL, symmetric pair storage only: the mirror entry a_ji
                                   this slot also stands for (-1: the slot stands for one entry)                      */
    /* panel form: what pass 1 streams in place of PB_COL + PB_DST (derived from them; PB_DST stays the definition).
       Inside a 64-entry chunk the slots are runs, so 4 bytes per entry become two flag bits:                          */
    EHYB_ARR_PB_COLF       = 31,/* uint16 like PB_COL: bits 0-13 column, bit 15 = first entry of a piece (its partial),
                                   bit 14 = that piece's slot does not follow the previous piece's: a "jump" (the
                                   first entry of a chunk always is one)                                              */
    EHYB_ARR_PB_CHUNK      = 32,/* uint32 [chunks+1] index of the chunk's first jump in PB_JUMP; last = number of jumps */
    EHYB_ARR_PB_JUMP       = 33,/* uint32 per jump: its slot minus the pieces before it in its chunk (mod 2^32), so that
                                   slot(entry) = PB_JUMP[chunk's first + jumps up to the entry - 1] + pieces before the
                                   entry's; the padding piece of a panel's last chunk yields 0xFFFFFFFF             */
    EHYB_ARR_COL_SEG_FIRST = 34,/* int32  [segments+1] column segments of ehyb_plan_create_host_segs (empty: one segment)  */
    EHYB_ARR_PB_SEG_ITEM   = 35,/* int32  [segments+1] panel form: first pass-1 item of every column segment              */
    EHYB_ARR_PB_ITEMS1     = 36 /* int32  [2*items] {first unit, end unit}: the work of one pass-1 workgroup -- consecutive
                                   units of (nearly) equal total cost (entries streamed + panels staged)                */
};
/*
 * The column words and slab records as ehyb_plan_upload sends them (cfg.ell_triples); host arithmetic, valid on a plan that was
 * never uploaded.  A slab is TRIPLE-CODED iff it has no inline residual pairs, is not a relative slab, its window has at least 3
 * slots, and for every group the 2 * pairs 16-bit entries, cut into threes from the front, are triples (b, b+1, b+2) with equal
 * bits 15 or (0, 0, 0) (padding), a remainder of two entries being (b, b+1) or (0, 0).  Such a slab holds T = ceil(2 * pairs / 3)
 * bases per group, two per 32-bit word (low half first), W = ceil(T / 2) words per group at [word][group] with stride G; a base
 * carries bit 15 for its triple, a padding triple is base 0.  With (A, B) = word j, pair 3j reads the columns (A, A+1), pair 3j+1
 * (A+2, B), pair 3j+2 (B+1, B+2).  Every other slab keeps its words.  In the records, word 1 is the slab's offset in the
 * transcoded array and bit 6 of word 3 marks a triple-coded slab.
 *   ONE EXCEPTION, by plan: a plan with symmetric pairs AND an inline residual (stats.er_inline > 0) whose window is small enough
 *   for four columns per pass (ehyb_spmm_max_k = 4) keeps every slab in the host's form -- the window kernel of exactly that
 *   combination carries no decoder (it would spill).  The rule is the one behind ehyb_spmm_max_k; ehyb_spmm refuses that
 *   kernel on coded words (EHYB_ERR_INTERNAL), which the rule makes unreachable.
 *   ehyb_plan_device_col_words  the number of words (-1: null plan); equals stats.col_words with cfg.ell_triples = 2.
 *   ehyb_plan_device_cols       the arrays: words_out holds that many words, meta_out the 4 * n_slabs words of the records.
 */
int64_t ehyb_plan_device_col_words(const ehyb_plan* plan);
int ehyb_plan_device_cols(const ehyb_plan* plan, uint32_t* words_out, uint32_t* meta_out);
/*
 * The value streams as ehyb_plan_upload sends them (cfg.val_f32); host arithmetic, valid on a plan that was never uploaded.
 *   ehyb_plan_device_value_bytes  bytes of the window kernel's value stream (inline residual pairs included) and of the CSR
 *                                 residual's values on the device: 8 per value, 4 with cfg.val_f32 = 1.  Either output may be NULL.
 *   ehyb_plan_device_values_f32   (cfg.val_f32 = 1 only, else EHYB_ERR_STATE) the fp32 stream itself: which = EHYB_ARR_ELL_VAL
 *                                 ([pair][lane][2] floats, the order and slab offsets of the host array) or EHYB_ARR_ER_VAL (one
 *                                 float per entry); count must be the host array's length.
 */
int ehyb_plan_device_value_bytes(const ehyb_plan* plan, int64_t* ell_bytes, int64_t* er_bytes);
int ehyb_plan_device_values_f32(const ehyb_plan* plan, int which, float* out, int64_t count);

/* Read-only view of one array of the plan's host layout.  A plan whose panel form was built on the device (ehyb_plan_create,
 * cfg.symbolic) downloads the PB_* streams on the first call that asks for one; it has no CSR form of that residual
 * (ER_SEG_*, ER_COL, ER_VAL empty, er_segments = 0). */
int ehyb_plan_host_array(const ehyb_plan* plan, int which, const void** ptr, int64_t* count);

/* ------------------------------------------------------------ multiply (GPU) */

/*
 * y = A*x on `stream` (a hipStream_t passed as void*; NULL = the null stream).
 * x and y are DEVICE pointers to full-length vectors in the permuted numbering
 * (x: n_cols doubles; y: rows [row_begin,row_end) of it are written).  Asynchronous.
 * One launch (ehyb_ell_kernel) when the residual is empty or tiny enough to ride inside
 * it (stats.er_inline > 0), else two: ehyb_ell_kernel then ehyb_er_kernel.
 * Replaces matrixVectorEHYB / matrixVectorEHYB_small (kernel.cu:490-552).
 * A plan multiplies ONE vector at a time: with the residual in panel form (stats.er_partials > 0) the
 * partial sums of a multiply live in a buffer of the plan, so two multiplies of the same plan must not
 * overlap on different streams (the reference is not re-entrant either: global device counters).
 * Non-finite values.  A NaN or an infinity in the MATRIX reaches exactly the rows that store it: a row comes out NaN, +inf,
 * -inf or finite as the exact sum of its entries' products would (that class does not depend on the order of summation), and
 * no other row changes.  A NaN or an infinity in x makes every row that stores its column non-finite (a NaN is never lost;
 * an infinity may come out as NaN).  Rows that do NOT store that column may come out NaN as well: padding slots hold the
 * value 0.0 and still read a column -- ELL lanes without an entry read columns 0 to 2 of their window (column 0, as the
 * reference's ELL padding does, convert.c, in the host layout; in a triple-coded slab on the device, cfg.ell_triples, a padding
 * triple reads columns 0, 1, 2), and the padding of an inline residual (stats.er_inline) reads x[0] -- and 0 * inf, 0 * NaN are
 * NaN.  (A NaN in x[0] alone turns most rows of an inline-residual plan NaN.)  The padding of the panel form and the direct
 * shape reads nothing.  With every x finite no padding slot changes a result.
 * Range.  Subnormal matrix values, x entries, products and partial sums are kept on every path, never flushed to zero: the
 * window, halo and direct kernels, the CSR and inline residual, both passes of the panel form, and the fp64 atomic adds --
 * ds_add_f64 for symmetric pairs and for the panel form's piece sums, global_atomic_add_f64 for split rows -- which were observed
 * to keep subnormal operands and results on gfx950 (tests/test_gpu_range.py; every kernel is built with both denormal modes of
 * its descriptor at "keep", tests/test_range_layout.py).  Every value and x travels with all 53 bits of its mantissa (ehyb_plan_
 * set_values and the plan cache included; the refill compares a stored pair a_ij == a_ji as fp64 numbers, so two different
 * subnormals differ).  No row's arithmetic touches another row's: rows hundreds of binades apart do not disturb each other.  A
 * product is finite whenever every ordering of its partial sums is: no path meets an infinity before the end of a finite sum.
 * fp32 values (cfg.val_f32 = 1).  The multiply is the fp64 multiply of the matrix whose values are float(a_ij): the same kernels'
 * arithmetic on fp64 operands, per accumulator in the same order (inline residual, pairs in rising order, .x and .y halves apart,
 * then their sum), so with plain storage and no split rows the result equals, bit for bit, that of an fp64 plan built from the
 * rounded values; with symmetric pairs or split rows, up to the order of their atomic adds.  A value beyond the fp32 range is
 * +-inf and its row comes out so; fp32 subnormal values (down to 2^-149) are kept and multiplied exactly.  A solver on such a
 * plan solves the ROUNDED system: ehyb_pcg_refine gives the fp64 answer.
 */
int ehyb_spmv(ehyb_plan* plan, const double* x_dev, double* y_dev, void* stream);
/*
 * THE WALK.  Successive multiplies of a plan whose streams do not fit the 256 MB Infinity Cache walk them in ALTERNATING
 * directions (cfg.ell_alternate), so that a launch starts with what the one before it left in that cache: a loop of multiplies
 * -- a solver's -- runs about 10 % faster than the same launches all first to last (audikw_1-like: 76 against 83 us).  A single
 * multiply after other work gets the cold-cache time either way.  The direction is per-plan state, flipped atomically by every
 * launch: several host threads may multiply with ONE plan on their own streams and vectors at the same time where the plan
 * multiplies in ELL launches only (no panel-form residual: see above); with plain storage the result does not depend on the
 * direction bit for bit, with symmetric pair storage it differs by the rounding of the LDS adds' order, as between any two launches.
 * ehyb_spmv_walk states the direction per call: EHYB_WALK_AUTO = ehyb_spmv, _FIRST_TO_LAST / _LAST_TO_FIRST explicit (honoured
 * whatever cfg.ell_alternate says) -- what a caller that captures multiplies into its own hipGraph uses, because a captured launch
 * keeps the direction it was captured with: capture an even number of multiplies with alternating directions, or use
 * ehyb_spmv_graph_create, which does exactly that.
 */
enum { EHYB_WALK_AUTO = -1, EHYB_WALK_FIRST_TO_LAST = 0, EHYB_WALK_LAST_TO_FIRST = 1 };
int ehyb_spmv_walk(ehyb_plan* plan, const double* x_dev, double* y_dev, void* stream, int walk);
/*
 * `multiplies` back-to-back multiplies y = A x captured into a hipGraph with the directions alternating explicitly inside the run;
 * for an odd count (1: the solver that launches one multiply per iteration) TWO executables are captured, beginning first-to-last
 * and last-to-first, and ehyb_graph_launch replays them in turn -- the alternation survives the capture.  A plan that multiplies in
 * window launches alone and keeps a fixed set of slabs in the Infinity Cache (cfg.ell_nt = 0/4/5, cfg.ell_alternate != 1) gains nothing
 * from a direction: every captured multiply walks first to last and one executable serves.  x and y are bound at capture.  One launch
 * at a time per graph object.
 */
typedef struct ehyb_graph ehyb_graph;
int ehyb_spmv_graph_create(ehyb_plan* plan, const double* x_dev, double* y_dev, int multiplies, ehyb_graph** graph);
int ehyb_graph_launch(ehyb_graph* graph, void* stream);
void ehyb_graph_destroy(ehyb_graph* graph);

/*
 * THE TRANSPOSED MULTIPLY y = A^T x on the plan A already has, in the permuted numbering: no second plan, no second reorder, no
 * second copy of the matrix on the device.  x_dev holds n_rows doubles, y_dev n_cols (the matrix is square).  Asynchronous on
 * `stream`; may be captured in a hipGraph.  y is ASSIGNED: the call first zeroes y in-stream (a memset node in a captured graph),
 * and every contribution to it is then an fp64 atomic add.  x_dev == y_dev is rejected (EHYB_ERR_ARG).
 *   Window plans: the work items, segments, item map and the plain / non-temporal split of the value stream are those of
 *   ehyb_spmv's window launch.  The LDS window of a partition (own rows plus halo) holds accumulators instead of x: a lane loads
 *   x[its row] once per slab and adds value * x[row] to the window column of each of its entries (ds_add_f64; lanes that share a
 *   column list -- the unknowns of a node -- are summed across lanes first, one add for three), pair, relative and triple-coded
 *   column words alike; the window is then added to y (global_atomic_add_f64), own columns and halo columns.  An
 *   inline residual adds its products straight to y[column].  x is not staged: the LDS of the launch is that of ehyb_spmv.
 *   A CSR residual and the direct shape: every lane of the row-segment kernel adds value * x[row] to y[column]; on a window plan
 *   this launch follows the window launch, on a direct-shape plan it is the whole multiply.
 * Served: plain storage over all rows with fp64 values.  Refused with EHYB_ERR_ARG before any device work, y untouched and the
 * form named in ehyb_last_error: symmetric pair storage (for a symmetric matrix A^T = A: call ehyb_spmv; the form's LDS has no
 * room for halo accumulators), a residual in panel form, cfg.val_f32 = 1, a plan not over all rows, a plan with column segments --
 * checked in this order, after null pointers and x == y.  Then EHYB_ERR_STATE on a plan never uploaded.
 * ehyb_spmv_t_supported applies the same rule on the host (EHYB_OK or EHYB_ERR_ARG with the form named); it works on a plan that
 * was never uploaded.
 * Contract.
 *   Order.  The LDS and global adds arrive in an order that varies from run to run: a result is reproducible only up to the order
 *   of summation, as with symmetric pair storage under ehyb_spmv.  Where every product and partial sum is exact (integer data) it
 *   is bit-exact.  A column that receives nothing, or only zeros, is +0.0.
 *   Range.  Subnormal values, x entries, products and sums are kept (ds_add_f64 and global_atomic_add_f64 keep them on gfx950).
 *   Non-finite values.  A non-finite MATRIX value reaches exactly the columns of the rows that store it.  A non-finite x[i] makes
 *   every column that row i stores non-finite (a NaN is never lost; an infinity may come out as NaN).  Through padding slots
 *   (value 0.0: 0 * inf and 0 * NaN are NaN) it may additionally turn NaN the columns 0 to 2 of row i's window -- in a slab with
 *   relative columns: column i itself --, and with an inline residual y[0].  This is the transposed image of the rule under
 *   ehyb_spmv.  With every x finite no padding slot changes a result.
 * One multiply at a time per y; several host threads may multiply with one plan on their own streams and vectors.
 */
int ehyb_spmv_t(ehyb_plan* plan, const double* x_dev, double* y_dev, void* stream);
int ehyb_spmv_t_supported(const ehyb_plan* plan);

/*
 * SEVERAL VECTORS per pass over the matrix: Y[:, j] = A X[:, j] for j < k.  X, Y: device pointers, column j at X + j*ldx and
 * Y + j*ldy (column-major: a torch.empty(k, n) is this layout with ld = n); ldx >= n_cols, ldy >= the plan's row_end (n_rows for a
 * plan of every row).  Only rows [row_begin, row_end) of each Y column are written; nothing between the columns is read or written.
 * walk: EHYB_WALK_AUTO / _FIRST_TO_LAST / _LAST_TO_FIRST, as ehyb_spmv_walk, for every pass.  Asynchronous on `stream`.
 * The multiply makes ceil(k / k_max) passes over the matrix (ehyb_spmm_max_k), of widths as even as they come; a pass of width 1
 * is the ehyb_spmv_walk launch sequence itself, a wider one stages the K columns' windows interleaved in LDS and reads the
 * matrix's streams once for all of them.  Column j of a plain-storage multiply equals ehyb_spmv of X[:, j] bit for bit, but for
 * rows the residual splits into several segments (fp64 atomics); with symmetric pair storage the LDS adds' order is free, as
 * between any two launches.  The non-finite contract of ehyb_spmv holds per column: a non-finite X[c, j] reaches column j only.
 * So does its range contract: subnormal values, X entries, products and partial sums are kept at every width and in both panel
 * passes (LDS atomics included, as observed on gfx950), a column is finite whenever every ordering of its partial sums is, and a
 * subnormal column beside one near 2^1023 in the same call do not reach each other (tests/test_gpu_range.py).
 * A residual in PANEL FORM (stats.er_partials > 0) is multiplied K wide too: the window launch K wide where the plan kept windows,
 * then both panel passes -- pass 1 stages K interleaved images of every x panel and reads the entry stream (values, column words,
 * chunk records, jump lists) once for the K products; pass 2 reads one row word per partial sum for its K adds.
 *   Exactness: pass 2 adds the partial sums with LDS atomics, in any order, at every width (as between two one-vector launches
 *   of such a plan).  A column of a K-wide panel multiply equals the one-vector multiply up to the order of summation, and bit
 *   for bit wherever every product and sum is exact (integer data).
 *   Non-finite values, per column: the padding of the panel form reads nothing (a padding slot stores nothing), so a non-finite
 *   X[c, j] reaches column j only, and in it only the rows that store column c -- plus, through windows the plan kept, what the
 *   window contract allows.
 *   One multiply at a time per plan (the partial-sum buffer, k_max * stats.er_partials doubles), as for ehyb_spmv.
 *   The multiply in parts (ehyb_spmv_part, ehyb_halo_*) stays one vector wide.
 * EHYB_ERR_ARG for a null pointer, k < 1, an ld too small or a bad walk; EHYB_ERR_STATE on a plan never uploaded.
 */
int ehyb_spmm(ehyb_plan* plan, const double* X_dev, int64_t ldx, double* Y_dev, int64_t ldy, int k, void* stream, int walk);
/*
 * Widest k one pass over the matrix serves on this plan (1..4).  Host-side only: valid on a plan built by
 * ehyb_plan_create_host that was never uploaded.
 *   window plans: min(4, (EHYB_LDS_MAX_DOUBLES * 8 - 16) / (8 * window capacity)) -- K window images (x, with symmetric pair
 *                 storage the y accumulators too) and the 16-byte slab counter in the 160 KiB of LDS.  A plan built with the
 *                 default window has k_max = 1: to get a wide plan, build it with cfg.lds_doubles = EHYB_LDS_MAX_DOUBLES / k
 *                 (the partitions are then sized for k vectors; the one-vector multiply of such a plan still works);
 *   the direct shape (no window): 4;
 *   a residual in panel form (stats.er_partials > 0): min(k_panel, k_window) with
 *                 k_panel  = min(4, (EHYB_LDS_MAX_DOUBLES - 1) / panel columns, EHYB_LDS_MAX_DOUBLES / rows of the largest row block)
 *                 -- K panel images and the one hand-over word behind them in pass 1, K accumulators per row of the largest
 *                 row block in pass 2 -- and k_window = the window rule above where the plan still makes a window launch (4
 *                 where no partition kept its window: stats.lds_bytes == 0).  Integer division throughout.  The panel columns
 *                 are the CONFIGURED width (cfg.er_panel_cols, default 16,384), not the widest panel the matrix fills, so a
 *                 default plan has k_max = 1: build with cfg.er_panel_cols = 16384 / k (4096 for k = 4, 5120 for 3, 8192 for
 *                 2) and, where windows are kept, cfg.lds_doubles = EHYB_LDS_MAX_DOUBLES / k as well.  A window that holds no
 *                 entry still counts (cfg.er_mode = 2 keeps the windows).  Host- and device-built plans of one matrix report
 *                 one width.  Narrower panels mean more partial sums per vector (R-MAT 2^22: 8.9 M at 16,384 columns, 13.3 M
 *                 at 4,096), and the partial sums scale with K: see DESIGN.md 10 for what each width measured before
 *                 choosing one -- k_max says what FITS, not what pays.
 */
int ehyb_spmm_max_k(const ehyb_plan* plan, int* k_max);

/* phase 1: ELL part only (needs only window columns);  phase 2: residual only
 * (y += ...);  phase 0: both.  Lets a multi-GPU caller overlap the x exchange.
 * Phase 2 must follow phase 1 on the same stream before y is read: where partitions were given up to a
 * panel-form residual (their windows did not pay), phase 1 leaves their rows alone and phase 2 ASSIGNS them. */
int ehyb_spmv_phase(ehyb_plan* plan, const double* x_dev, double* y_dev, void* stream, int phase);

/*
 * Tuning on the device the plan lives on (optional; no reference counterpart).  The 8 XCDs of an MI355X do not stream at
 * the same rate -- on every box measured two of them finish a launch 8-12 % behind the fastest at equal bytes, and which
 * ones is a property of the box -- while the ELL launch of a plan with one resident round of workgroups lasts as long as
 * its LAST workgroup.  This call times a few stamped launches of the ELL kernel (per-workgroup clocks, XCC id), ranks the
 * XCDs by the rate they streamed at, and lets workgroup b take item item_map[b] with the heaviest items on the fastest XCD
 * and so on down; it keeps the new map only if the stamped launch got shorter.  *span_before_us / *span_after_us (may be
 * NULL): launch span before and with the map the plan ends with.  Synchronous (null stream); y is overwritten with A*x.
 * No-op for plans whose ELL launch needs more than one round of workgroups, for the direct shape and for plans without
 * an ELL launch.  spmvGPuEHYB does it during its warm-up; plan-API callers decide for themselves -- before they capture
 * multiplies of the plan into a hipGraph (a captured launch keeps the map it was captured with; replaced maps stay
 * allocated until the plan is destroyed, so such a graph stays valid).
 */
int ehyb_plan_tune(ehyb_plan* plan, const double* x_dev, double* y_dev, int reps, double* span_before_us, double* span_after_us);

/*
 * DIAGNOSTICS (tools/, tests/): no part of the product's contract beyond what is said here.
 * ehyb_debug_ell_stamps        one launch of the STAMPED instantiation of the plan's one-vector window kernel (not cfg.val_f32) on
 *                              the null stream, synchronous.  y is written as by the window launch of ehyb_spmv; out_host receives 4
 *                              words per item (stats.n_items of them): entry / window staged / exit wall-clock ticks (100 MHz) and
 *                              the XCC id (ehyb_plan_tune masks it with 15).  An item without a segment stages nothing.
 * ehyb_debug_ell_stamps_probe  the same launch with the staging replaced (triple_gather 1: every window entry from three vectors,
 *                              2: no halo gather) -- for timing only, y is WRONG by design.
 * ehyb_debug_panel_times       mean time in ms of each pass of a panel-form residual alone, `iters` launches each between HIP events
 *                              on the null stream; probe != 0 switches steps of pass 1 off (y wrong by design).
 * THE KERNEL TABLES.  The library builds three tables of kernel instantiations and every launch looks its kernel up in one:
 *   EHYB_KERNELS_WINDOW   EHYB_KERNEL_ROW_WINDOW = 7 ints per row:  threads, k, dyn, stamp, inl, sym, f32 -- workgroup size; columns
 *                         per pass; 1 = LDS slab counter, 0 = static round-robin (cfg.ell_variant = 3); stamped (above); inline
 *                         residual; symmetric pairs; cfg.val_f32
 *   EHYB_KERNELS_PANEL    EHYB_KERNEL_ROW_PANEL = 6:  pass, threads, k, dpp, probe, nt -- pass 1 or 2; workgroup size; columns; 1 =
 *                         register-scan sums, 0 = LDS sums (cfg.er_sums = 2); the timing probes; pass 2's streaming hint (cfg.er_nt).
 *                         A field its pass does not have holds one value.
 *   EHYB_KERNELS_ER_CSR   EHYB_KERNEL_ROW_ER_CSR = 3:  k, assign, f32 -- columns; 1 = the direct shape (assigns), 0 = adds; cfg.val_f32
 * ehyb_debug_kernel_table      the rows of table `which`: *n_rows = their number, the first min(cap, *n_rows) rows are written to
 *                              `rows` (cap rows of the table's width; rows may be NULL with cap 0).  Host only: needs no device.
 * ehyb_debug_launched          the plan's LAUNCH LOG of table `which`: out[i] = 1 iff a launch of this plan took row i since the plan
 *                              was made or the log last cleared; cap >= the table's rows (EHYB_ERR_ARG otherwise).  A launch marks
 *                              its row with one byte store before it enqueues the kernel; a launch that finds nothing to do (no
 *                              item, no residual) marks nothing.  ehyb_debug_launched_clear zeroes all three logs.
 * THE ITEM MAP.  Workgroup b of a window launch takes item map[b]; a launch that walks a plan of several rounds of workgroups from
 * the far end (ehyb_spmv_walk 1) takes map[n_items - 1 - b].  The transposed launch and the stamped launch read the same map.
 * ehyb_debug_item_map          the map in force: *n_items = stats.n_items, the first min(cap, *n_items) entries are written to out
 *                              (out may be NULL with cap 0); *installed = 1 if the plan holds a map (ehyb_plan_tune kept one, or
 *                              ehyb_debug_set_item_map set one), 0 if the launches take the built-in order, which is then what out
 *                              receives: item b for symmetric pairs and cfg.xcd_map = 2, else one contiguous run of items per XCD
 *                              (k = b mod 8, j = b / 8: item k * (n / 8) + min(k, n mod 8) + j).  Host only: needs no device and
 *                              works on a plan that was never uploaded.
 * ehyb_debug_set_item_map      installs map[0..n) as the plan's map, the way ehyb_plan_tune installs the one it keeps: the map it
 *                              replaces stays allocated until the plan is destroyed, so a hipGraph captured under it stays valid.
 *                              n must be stats.n_items and every entry in [0, n), whatever strict is: EHYB_ERR_ARG otherwise, the
 *                              plan untouched.  strict = 1 also demands a permutation.  strict = 0 allows an item to be named
 *                              twice and another not at all -- for tests that show that a kernel READS the map: the rows of an
 *                              item nobody takes are not written (ehyb_spmv_t: not added), so products are WRONG by design, as
 *                              with the stamp probes.  map = NULL with n = 0 removes the plan's map (back to the built-in order)
 *                              and retires it the same way.  Any uploaded plan with a window launch: several rounds of
 *                              workgroups and cfg.val_f32, which ehyb_plan_tune leaves alone, included.  EHYB_ERR_ARG for the
 *                              direct shape and for plans without items; all of the above is checked first, then EHYB_ERR_STATE
 *                              for a plan never uploaded.  Synchronises the device before it changes the map and before it returns.
 * ehyb_debug_tune_decide       the decision of ehyb_plan_tune on the caller's numbers, a pure host function: cost[i] of item i,
 *                              xcc[b] (0..15) and dur[b] (us) of workgroup b, which took item map_now[b].  The rate of an XCD is the
 *                              median over its workgroups of cost[map_now[b]] / max(dur[b], 1e-3) (the upper median of an even
 *                              count); XCDs are ordered fastest first, equal rates by id; items by falling cost, equal costs by
 *                              index; each XCD's workgroups, in rising b, take the next items.  *stable = 1 and map_new[0..n_items)
 *                              is that map -- or *stable = 0 and map_new untouched where some xcc[b] < 0 (ehyb_plan_tune: a
 *                              workgroup that ran on two XCDs in two launches).  EHYB_ERR_ARG for a null pointer, n_items < 1, an
 *                              xcc[b] > 15 or a map_now[b] outside [0, n_items).
 */
enum { EHYB_KERNELS_WINDOW = 0, EHYB_KERNELS_PANEL = 1, EHYB_KERNELS_ER_CSR = 2 };
enum { EHYB_KERNEL_ROW_WINDOW = 7, EHYB_KERNEL_ROW_PANEL = 6, EHYB_KERNEL_ROW_ER_CSR = 3 };
int ehyb_debug_ell_stamps(ehyb_plan* plan, const double* x_dev, double* y_dev, unsigned long long* out_host);
int ehyb_debug_ell_stamps_probe(ehyb_plan* plan, const double* x_dev, double* y_dev, unsigned long long* out_host, int triple_gather);
int ehyb_debug_panel_times(ehyb_plan* plan, const double* x_dev, double* y_dev, int iters, int probe, double* ms_scale, double* ms_reduce);
int ehyb_debug_kernel_table(int which, int32_t* rows, int cap, int* n_rows);
int ehyb_debug_launched(const ehyb_plan* plan, int which, uint8_t* out, int cap);
int ehyb_debug_launched_clear(ehyb_plan* plan);
int ehyb_debug_item_map(const ehyb_plan* plan, int32_t* out, int cap, int* n_items, int* installed);
int ehyb_debug_set_item_map(ehyb_plan* plan, const int32_t* map, int n, int strict);
int ehyb_debug_tune_decide(int n_items, const double* cost, const int* xcc, const double* dur, const int32_t* map_now, int32_t* map_new, int* stable);
/*
 * The kernels of the transposed multiply (ehyb_spmv_t) have a table and a launch log of their own; the three tables above do not
 * list them.  EHYB_KERNEL_ROW_T = 3 ints per row: kind, threads, inl -- EHYB_KERNEL_T_WINDOW (the transposed window kernel) or
 * EHYB_KERNEL_T_RESIDUAL (the transposed row-segment kernel: CSR residual and direct shape); workgroup size; inline residual.
 * ehyb_debug_kernel_table_t and ehyb_debug_launched_t work as their namesakes above (host only / one byte per row, cap >= the
 * table's rows); ehyb_debug_launched_clear zeroes this log too.
 */
enum { EHYB_KERNEL_T_WINDOW = 0, EHYB_KERNEL_T_RESIDUAL = 1 };
enum { EHYB_KERNEL_ROW_T = 3 };
int ehyb_debug_kernel_table_t(int32_t* rows, int cap, int* n_rows);
int ehyb_debug_launched_t(const ehyb_plan* plan, uint8_t* out, int cap);

/*
 * The multiply in PARTS, for a caller that receives x segment by segment (multi-GPU, ehyb_plan_create_host_segs):
 *   flags & EHYB_PART_FIRST   the ELL launch (window columns: all inside column segment 0) runs first;
 *   column segments [seg_begin, seg_end): pass 1 of the panel-form residual over the panels of those segments
 *                             (needs x of those columns only, and writes no y);
 *   flags & EHYB_PART_LAST    pass 2 of the panel form (every pass 1 must have been enqueued on `stream` before; reads no x) --
 *                             or, for a plan whose residual is in CSR form, the residual launch (all of x).
 * ehyb_spmv == one call with every segment and both flags.  Parts of one multiply go to ONE stream, in order.
 * "Window columns: all inside column segment 0" holds for the plan of a rank: segment 0 covers the own columns of the plan's
 * partitions (its rows) and cfg.n_top > 1 keeps every window, contiguous part and gathered columns, inside them (dist.py:
 * RankLocalMatrix; a plan with cfg.row_split is built with every window given up).  On any other plan -- segments cut through a single-GPU matrix, tests/test_gpu_parts.py -- the FIRST launch
 * reads whatever columns its windows hold, and all of x must be there.
 * A refused call (EHYB_ERR_ARG: segments outside the plan; EHYB_ERR_STATE: a plan that multiplies in one launch, or
 * EHYB_PART_LAST_FOREIGN on a plan without cfg.row_split) has enqueued nothing.
 * tests/test_gpu_parts_exact.py pins all of this bit for bit, with every column that has not arrived poisoned.
 */
enum { EHYB_PART_FIRST = 1, EHYB_PART_LAST = 2,
       EHYB_PART_LAST_FOREIGN = 4 /* panel form with cfg.row_split: pass 2 over the row blocks from row_split on only (they have entries in
                                     column segment 0 alone, so they are complete once segment 0's pass 1 is enqueued); with such a
                                     plan EHYB_PART_LAST closes the rows IN FRONT of row_split only: ehyb_spmv == one call with every
                                     segment and all three flags */ };
int ehyb_spmv_part(ehyb_plan* plan, const double* x_dev, double* y_dev, void* stream, int seg_begin, int seg_end, int flags);
/* Column segments of the plan (1 unless made by ehyb_plan_create_host_segs). */
int ehyb_plan_col_segs(const ehyb_plan* plan, int* n_col_segs);
/* dst[i] = src[idx[i]], i < n, on `stream`: packs the x entries the other ranks asked for (the send list of a halo
 * exchange) -- device pointers. */
int ehyb_gather(const double* src_dev, const int32_t* idx_dev, double* dst_dev, int64_t n, void* stream);
/* y[idx[i]] += src[i], i < n, on `stream` (fp64 atomics: an index may occur more than once): the partial sums other ranks
 * computed for this rank's rows, added in (exchange "cover") -- device pointers. */
int ehyb_scatter_add(double* y_dev, const int32_t* idx_dev, const double* src_dev, int64_t n, void* stream);
/*
 * Stream plumbing of one exchange step, so that the host issues ONE call per part instead of an event record, a stream
 * wait and a launch each (the host side of a step costs as much as the device side at 8 GPUs: DESIGN.md 5):
 *   ehyb_step_pack   on compute_stream: ehyb_gather into send_buf; then comm_stream waits for it (the collective that
 *                    the caller enqueues on comm_stream next reads send_buf);
 *   ehyb_step_part   wait_comm != 0: compute_stream first waits for everything enqueued on comm_stream so far (the
 *                    collective that delivers this part's columns); then ehyb_spmv_part on compute_stream.
 */
int ehyb_step_pack(const double* x_dev, const int32_t* idx_dev, double* send_buf_dev, int64_t n, void* compute_stream, void* comm_stream);
int ehyb_step_part(ehyb_plan* plan, const double* x_dev, double* y_dev, void* compute_stream, void* comm_stream, int wait_comm,
                   int seg_begin, int seg_end, int flags);
/*
 * The whole exchange step as ONE call, for a caller that issues its collectives from C (RCCL: ncclGroupStart / ncclSend /
 * ncclRecv / ncclGroupEnd) -- no reference counterpart.  The plan was made by ehyb_plan_create_host_segs with 1 + n_chunks
 * column segments (own columns, then one per chunk).  Sequence: ehyb_step_pack; own columns (EHYB_PART_FIRST); then for
 * k = 0 .. n_chunks-1: exchange(k, comm_stream, user) -- the caller ENQUEUES on comm_stream the collective that fills chunk k's
 * ghost columns of x_dev (0 = ok; anything else aborts the step with EHYB_ERR_STATE) -- and the panels of chunk k on
 * compute_stream behind it, the last one with EHYB_PART_LAST.  Everything asynchronous.
 */
typedef int (*ehyb_exchange_fn)(int chunk, void* comm_stream, void* user);
int ehyb_halo_step(ehyb_plan* plan, const double* x_dev, double* y_dev, const int32_t* send_idx_dev, double* send_buf_dev, int64_t n_send,
                   int n_chunks, ehyb_exchange_fn exchange, void* user, void* compute_stream, void* comm_stream);

/*
 * ---- RCCL-native exchange (multi-GPU, one process per GPU; no reference counterpart: kernel.h:12 is a commented-out mpi.h).
 * librccl is opened at run time (dlopen; inside a process that has loaded torch the soname resolves to torch's copy), so a
 * single-GPU caller needs no RCCL.  A communicator is made from a ncclUniqueId that rank 0 creates and the caller hands to
 * every rank (bench.py / dist.py: a torch.distributed broadcast of the 128 bytes); the device current at
 * ehyb_comm_create is the rank's GPU.  The communicator owns a high-priority stream its exchanges run on.
 */
#define EHYB_COMM_ID_BYTES 128
typedef struct ehyb_comm ehyb_comm;
int ehyb_rccl_version(int* version, char* where, int where_len);   /* ncclGetVersion + the file name dlopen found; EHYB_ERR_STATE: no librccl */
int ehyb_comm_unique_id(void* id_out /* EHYB_COMM_ID_BYTES */);     /* ncclGetUniqueId */
int ehyb_comm_create(const void* id, int rank, int world, ehyb_comm** comm);   /* ncclCommInitRank: collective over all ranks */
void ehyb_comm_destroy(ehyb_comm* comm);
int ehyb_comm_info(const ehyb_comm* comm, int* rank, int* world, void** stream);
/* sum of `count` doubles over the ranks, in place (the dot products of a distributed CG); stream NULL = the communicator's */
int ehyb_comm_allreduce_sum(ehyb_comm* comm, double* buf_dev, int64_t count, void* stream);
int ehyb_comm_allgather(ehyb_comm* comm, const double* send_dev, double* recv_dev, int64_t count_per_rank, void* stream);
/*
 * One rank's halo exchange + multiply as ONE host call per step (ehyb_halo_spmv), for a plan made by ehyb_plan_create_segs
 * with 1 + n_chunks column segments: [own columns | ghost columns of chunk 0 | chunk 1 | ...], inside a chunk the entries
 * of peer 0, peer 1, ... in rank order.
 *   send_idx_host   n_send own columns (plan order) the peers asked for, chunk by chunk, inside a chunk peer by peer;
 *   send_counts / recv_counts   [n_chunks * world]: doubles sent to / received from peer p in chunk k (entry k*world + p;
 *                   what rank a sends to b in chunk k must be what b receives from a -- the caller agrees on that when it
 *                   builds the lists, dist.py: RankLocalMatrix).  A rank may send to itself (world 1: the loop-back test).
 * ehyb_halo_spmv(h, x, y, stream): pack (one gather) on `stream`; on the communicator's stream, behind the pack, chunk
 * after chunk as a group of ncclSend / ncclRecv pairs straight into the ghost columns of x; on `stream` the own-column
 * part at once, then chunk k's panels as soon as chunk k has landed, the closing pass last -- the panels of chunk k multiply
 * while chunk k+1 is on the wire.  Plans that multiply in one launch exchange first, then multiply.  Asynchronous.
 * The plan, x and y must outlive the calls; one step at a time per halo object.
 */
typedef struct ehyb_halo ehyb_halo;
int ehyb_halo_create(ehyb_comm* comm, ehyb_plan* plan, int n_chunks, const int32_t* send_idx_host, int64_t n_send,
                     const int64_t* send_counts, const int64_t* recv_counts, ehyb_halo** halo);
void ehyb_halo_destroy(ehyb_halo* halo);
int ehyb_halo_spmv(ehyb_halo* halo, double* x_dev, double* y_dev, void* compute_stream);
/*
 * Exchange "cover" (dist.py: RankLocalMatrix(exchange="cover")): per pair of ranks only the hub columns of the block
 * A[r, s] travel as x entries; the rest of the block is handed to the columns' owner s at set-up, who multiplies it with its own x
 * and ships ONE PARTIAL SUM PER ROW -- a vertex cover of the block's bipartite graph instead of all its columns (R-MAT 2^24: 2.2-2.7 x
 * fewer doubles on the wire at 2 / 4 / 8 ranks, tools/dist_volume_model.py).  The plan of such a rank was built with cfg.row_split
 * = its number of own rows; the rows behind are its FOREIGN rows (ehyb_matrix_append_rows), grouped by destination rank:
 * ysend_counts[p] of them belong to rank p, yrecv_counts[p] partial sums arrive from rank p, partial i (arrival order, peer 0's first)
 * is added to row yrecv_idx_host[i].  ehyb_halo_spmv then: pack; the x chunks on the wire at once; segment 0 (own columns: own AND
 * foreign rows); the foreign rows closed (EHYB_PART_LAST_FOREIGN) and sent off; the chunks' panels as they land; the own rows closed;
 * the received partial sums added (ehyb_scatter_add).  y_dev holds own rows followed by the foreign rows.  Panel-form plans only.
 */
int ehyb_halo_set_partials(ehyb_halo* halo, int row_split, const int64_t* ysend_counts, const int64_t* yrecv_counts,
                           const int32_t* yrecv_idx_host, int64_t n_yrecv);
/* north_star's "all-gatherv of x" as one call per step: x = [own segment padded to seg_len | segment of rank 0 | ... | of rank
 * world-1]; ncclAllGather on the communicator's stream while the ELL phase runs, then the residual phase (dist.py: GatherSpmv) */
int ehyb_gather_spmv(ehyb_comm* comm, ehyb_plan* plan, double* x_dev, double* y_dev, int64_t seg_len, void* compute_stream);

/*
 * Timed loop on device-resident vectors: `warmup` untimed multiplies, then `iters`
 * multiplies bracketed by HIP events on `stream` (no copies inside, residual recomputed
 * every time: SURVEY 8d "Timing protocol").  ms_total = whole loop.  If ms_ell / ms_er
 * are non-NULL a second pass of min(iters, 200) multiplies brackets every launch with its
 * own event pair and returns the AVERAGE duration of the ELL launch and of the residual
 * launch (0-length interval when the residual is inline or empty).
 */
int ehyb_spmv_bench(ehyb_plan* plan, const double* x_dev, double* y_dev, void* stream,
                    int warmup, int iters, double* ms_total, double* ms_ell, double* ms_er);

/*
 * spmvGPuEHYB (spmv.h) with an explicit configuration and a status code; *ms_total (may be NULL)
 * receives the time of the MAXIter timed multiplies.  cfg == NULL is what spmvGPuEHYB itself does:
 * every knob at its default and the storage chosen from the matrix it is handed -- symmetric pair
 * storage iff the matrix has at least EHYB_SYM_MIN_ROWS rows, its partitions leave room for the y
 * accumulators (they do when matrixReorder made them) and a sample of its entries has bitwise equal
 * mirror images; no environment variable takes part.
 */
int spmvGPuEHYB_cfg(matrixCOO* localMatrix, const double* vectorIn, double* vectorOut, const int MAXIter,
                    int* realIter, const ehyb_config* cfg, double* ms_total);

/*
 * Numeric phase of the build on the GPU: new VALUES on the pattern the plan was built from.
 * The reference fills its ELL / ER value arrays on one host thread (convert.c:316-369, after the scatter of V
 * through the permutation in reordering.c:348-362) and repeats partition, conversion and upload for every
 * matrix.  A plan built with cfg.value_map = 1 keeps the slot maps of its value streams; this call gathers
 * `values` through them straight into the device arrays the kernels read (ehyb_fill_kernel: ELL stream,
 * residual segments or panel stream), padding = 0.0 -- no partitioner, no layout pass, no re-upload of the
 * index arrays.
 *   values       count doubles = the V array of a matrix with the SAME row-grouped pattern: in the order of the
 *                reordered matrix the plan was built from (entry_order NULL), or in the caller's order BEFORE
 *                ehyb_matrix_reorder with entry_order[k] = place of reordered entry k in `values`
 *                (ehyb_entry_order computes it).
 *   on_device    0: values / entry_order are host arrays (uploaded for the call);  1: both are device pointers.
 * With symmetric pair storage a slot stands for a_ij AND a_ji: the new values must be equal there (a_ij == a_ji, the test the builder paired them with); they
 * are checked on the device first and the plan is left untouched (EHYB_ERR_ARG) if any pair differs.  The builder pairs by
 * VALUE, so on a matrix that is not symmetric entries that merely happened to be equal are pairs too, and new values must
 * keep them equal; a NaN never equals itself, so a NaN in a pair is refused as well.
 * After a successful call the HOST copy of the value arrays (ehyb_plan_host_array, ehyb_plan_save) is stale:
 * ehyb_plan_save refuses such a plan.  Synchronous with respect to `stream` when on_device = 0.
 */
int ehyb_plan_set_values(ehyb_plan* plan, const double* values, int64_t count, const int32_t* entry_order,
                         int on_device, void* stream);
/* entry_order[k_new] = k_old: where entry k_new of the matrix AFTER ehyb_matrix_reorder sat in the caller's
 * row-grouped arrays before it (rows move as wholes and keep their stored order).  row_idx_before = the rowIdx of
 * the matrix before the call (dimension+1 ints), reorder_list as the call left it. */
int ehyb_entry_order(int dimension, const int* row_idx_before, const int* reorder_list, int32_t* entry_order);

/* Convenience: host vectors in, host vector out (H2D, `iters` multiplies, D2H). */
int ehyb_spmv_host(ehyb_plan* plan, const double* x_host, double* y_host, int iters);

/* Device plumbing for callers without their own allocator (tests, the CLI). */
int ehyb_device_count(int* count);
int ehyb_device_set(int device);
int ehyb_device_name(char* buf, int len);
int ehyb_dev_alloc(size_t bytes, void** ptr);
int ehyb_dev_free(void* ptr);
int ehyb_h2d(void* dst_dev, const void* src_host, size_t bytes);
int ehyb_d2h(void* dst_host, const void* src_dev, size_t bytes);
int ehyb_dev_sync(void);
/* a non-blocking stream of the current device (hipStream_t as void*), for callers without a HIP binding of their own */
int ehyb_stream_create(void** stream);
int ehyb_stream_destroy(void* stream);
int ehyb_stream_sync(void* stream);
/* free and total device memory in bytes (hipMemGetInfo): what a harness checks a plan's life cycle against */
int ehyb_dev_mem_info(size_t* free_bytes, size_t* total_bytes);
/* Streaming-read ceiling of this device: sums `bytes` of doubles `iters` times, returns GB/s. */
int ehyb_measure_read_bw(size_t bytes, int iters, double* gbps);

/* ------------------------------------------------ iterative caller */

/*
 * Unpreconditioned conjugate gradients for A x = b on the plan's (symmetric positive definite)
 * matrix, entirely on the device: x_dev starts as the initial guess and ends as the solution,
 * both in the permuted numbering.  This is the solver the reference was cut down from (its
 * leftovers: kernelMyxpy y = x + gamma*y, kernel.cu:288-296; initialize_all, kernel.cu:20-31;
 * the PRECOND/FACT switches of cb_s) and the caller for which "x changes every multiply" matters.
 * One ehyb_spmv plus three fused vector kernels per iteration; dot products stay on the device
 * (per-workgroup partial sums added in a fixed order, no atomics), two iterations are replayed
 * from one hipGraph, and the host looks at the residual every `check_every` iterations (<= 0: 10;
 * odd values are rounded up to even).
 * Stops when ||r|| <= rtol * ||b|| or after max_iter iterations.  Outputs may be NULL.
 * Needs a plan over all rows (single GPU).  stream NULL: a private stream, synchronised with the
 * default stream on entry and finished on return.
 */
int ehyb_cg(ehyb_plan* plan, const double* b_dev, double* x_dev, int max_iter, double rtol,
            int check_every, void* stream, int* iters_done, double* rel_residual);
/*
 * Iterative refinement: fp64 answers from a plan that stores fp32 values (cfg.val_f32).  Per outer step: q = A x on `plan` (its
 * values fp64; walked first to last), r = b - q with ||r||^2 and ||b||^2 (one kernel; per-workgroup partials added in the fixed
 * order of the solvers); stop if ||r|| <= rtol ||b||, or if ||r|| did not at least halve since the previous step (stagnation:
 * EHYB_OK, the caller reads rel_residual); else d = 0, ehyb_pcg(inner_plan, inv_diag, r, d, inner_max_iter, inner_rtol) on the
 * same stream, x += d (one kernel).  At most max_outer corrections.  inner_plan is normally the val_f32 plan of the same reordered
 * matrix; any uploaded plan over all rows with the same number of rows is taken (an fp64 plan: restarted CG).  x_dev: the initial
 * guess in, the solution out.  outer_done: corrections applied; inner_iters_total: CG iterations over all of them; rel_residual:
 * the last ||b - A x|| / ||b|| computed with `plan`.  Stream and NULL outputs as for ehyb_pcg.  A breakdown of an inner solve is
 * returned as ehyb_pcg returns it.
 * ehyb_refine_residual_step / ehyb_refine_axpy_step launch the two vector kernels one at a time, as the ehyb_cg_*_step calls do:
 * r = b - q with the partials of r.r in s[0 .. slot_doubles) and of b.b in s[slot_doubles .. 2 slot_doubles) (slot_doubles of
 * ehyb_cg_layout; slot_doubles / 2 workgroups write, the rest stays as it is), and x += d.
 */
int ehyb_pcg_refine(ehyb_plan* plan, ehyb_plan* inner_plan, const double* inv_diag_dev, const double* b_dev, double* x_dev,
                    int max_outer, int inner_max_iter, double rtol, double inner_rtol, void* stream, int* outer_done,
                    int* inner_iters_total, double* rel_residual);
int ehyb_refine_residual_step(int n, const double* b_dev, const double* q_dev, double* r_dev, double* s_dev, void* stream);
int ehyb_refine_axpy_step(int n, const double* d_dev, double* x_dev, void* stream);
/* The same with the diagonal (Jacobi) preconditioner -- the PRECOND switch of the reference's cb_s
 * (spmv.h:7-15): inv_diag_dev[i] = 1 / a_ii in the permuted numbering (matrixCOO.diag, permuted
 * like x); NULL = ehyb_cg.  z = M^-1 r is recomputed on the fly, no extra vector is stored. */
int ehyb_pcg(ehyb_plan* plan, const double* inv_diag_dev, const double* b_dev, double* x_dev, int max_iter,
             double rtol, int check_every, void* stream, int* iters_done, double* rel_residual);

/*
 * BiCGSTAB for a general (unsymmetric) A x = b on the plan's matrix, entirely on the device, right-preconditioned with
 * M = diag(A): inv_diag_dev[i] = 1 / a_ii in the permuted numbering (NULL = no preconditioner).  Arguments, stream and
 * outputs as ehyb_pcg: x_dev holds the initial guess on entry and the solution on return, stream NULL = a private stream,
 * check_every <= 0 = 10 (odd values rounded up to even), outputs may be NULL, the plan must cover all rows.
 * Recurrences (shadow residual rh = r0 = b - A x0, p^ = M^-1 r0; only p^ = M^-1 p and s^ = M^-1 s are stored):
 *   v = A p^;  alpha = rho / (rh.v);  s = r - alpha v;  s^ = M^-1 s;  t = A s^;  omega = (t.s) / (t.t);
 *   x += alpha p^ + omega s^;  r = s - omega t;  rho_new = rh.r;  beta = (rho_new / rho) (alpha / omega);
 *   p^ = M^-1 r + beta (p^ - omega M^-1 v)
 * Two multiplies (walking first to last, then last to first) and five vector kernels per iteration; an even and an odd
 * iteration are replayed from one hipGraph (cfg.graphs = 2: plain launches; cfg.cg_fused_dot is ignored).
 * Stopping and breakdown are decided on the device, after every iteration: converged when r.r <= rtol^2 b.b, or after
 * the half step when s.s <= rtol^2 b.b (then x += alpha p^, r = s); the convergence test comes first.  A zero or non-finite
 * rho, rh.v, t.t or omega as a divisor, or a non-finite rho_new, is a breakdown: the kernel that meets it changes nothing and
 * every later one returns at once.  x is the last iterate whose update had finite scalars, iters_done the exact number of
 * such updates (the device's counter), rel_residual = sqrt(r.r / b.b) of that iterate (b.b = 0: 1 in its place); the host
 * only looks every check_every iterations, to stop launching.  With plain storage x, iters_done and rel_residual are
 * therefore the same bits for every check_every, for graphs and plain launches, and from run to run.  A breakdown returns
 * EHYB_ERR_ARG ("breakdown" in ehyb_last_error) after every output is written; so does a NaN in b, x0 or the initial residual,
 * with x unchanged.  EHYB_ERR_ARG for a null plan, b or x, max_iter < 0, a negative or NaN rtol or a plan not over all rows;
 * EHYB_ERR_STATE on a plan never uploaded -- all before any device work.
 */
int ehyb_bicgstab(ehyb_plan* plan, const double* inv_diag_dev, const double* b_dev, double* x_dev, int max_iter, double rtol,
                  int check_every, void* stream, int* iters_done, double* rel_residual);

/*
 * k INDEPENDENT solves on the plan's matrix that share every multiply: column j of X is what ehyb_pcg(b_j) makes of it (not a
 * block CG: every column keeps its own alpha, beta and stopping test).  Per iteration one ehyb_spmm of the k directions
 * (ceil(k / ehyb_spmm_max_k) passes over the matrix) and three vector kernels up to four columns wide.  B, X: device pointers,
 * column j at B + j*ldb and X + j*ldx (column-major, as ehyb_spmm), ldb, ldx >= n; only rows [0, n) of each column are read or
 * written.  X holds the initial guesses on entry and the solutions on return.  inv_diag_dev: one Jacobi preconditioner for
 * every column, as ehyb_pcg (NULL = none).  iters_done, rel_residual: host arrays of k entries, may be NULL.
 * Stopping, per column: at each check point (every `check_every` iterations, as ehyb_pcg) a column with ||r_j|| <= rtol ||b_j||
 * is frozen -- its x, r and p stop changing -- and iters_done[j] is that check point; the call returns when every column is
 * frozen or after max_iter iterations.  A column whose r.r or r.z turns NaN is frozen with rel_residual[j] = NaN, the others go
 * on, and the call returns EHYB_ERR_ARG (breakdown) at the end with every output written.  With plain storage column j equals
 * ehyb_pcg on b_j bit for bit, but for rows the residual splits into several segments (ehyb_spmm).  Iterations are replayed
 * from a hipGraph as in ehyb_pcg (cfg.graphs = 2: plain launches); cfg.cg_fused_dot is ignored: p . (A p) always comes from a
 * dot kernel of its own.  Needs a plan over all rows.  EHYB_ERR_ARG for a null pointer, k < 1, ldb or ldx < n, max_iter < 0, a
 * negative or NaN rtol or a plan not over all rows; EHYB_ERR_STATE on a plan never uploaded -- all before any device work.
 */
int ehyb_cg_multi(ehyb_plan* plan, const double* B_dev, int64_t ldb, double* X_dev, int64_t ldx, int k, int max_iter, double rtol,
                  int check_every, void* stream, int* iters_done, double* rel_residual);
int ehyb_pcg_multi(ehyb_plan* plan, const double* inv_diag_dev, const double* B_dev, int64_t ldb, double* X_dev, int64_t ldx, int k,
                   int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual);

/*
 * k INDEPENDENT BiCGSTAB solves on the plan's (unsymmetric) matrix that share both multiplies of every iteration: column j of X
 * is what ehyb_bicgstab(b_j) makes of it (not a block method: every column keeps its own rho, alpha, omega, beta, status word
 * and iteration counter).  Per iteration ehyb_spmm of the k directions p^ (first to last) and of the k s^ (last to first) --
 * ceil(k / ehyb_spmm_max_k) passes over the matrix each -- and the five vector kernels of ehyb_bicgstab up to four columns wide.
 * B, X, ldb, ldx, inv_diag_dev, iters_done, rel_residual, stream and check_every as ehyb_pcg_multi: column j at B + j*ldb and
 * X + j*ldx, ldb, ldx >= n, only rows [0, n) of a column are read or written, the outputs are host arrays of k entries and may be
 * NULL.  X holds the initial guesses on entry and, per column, the last iterate whose update had finite scalars on return.
 * Stopping and breakdown, per column and on the device, after every iteration, by the rules of ehyb_bicgstab: a column whose
 * status is set is skipped by every vector kernel from then on -- its x, r, p^ and partial sums stop changing -- while the
 * others go on; the multiplies keep multiplying it (a NaN stays in its column, ehyb_spmm).  A column with r.r <= rtol^2 b.b at
 * the start is converged with 0 iterations, one with a non-finite b.b or r.r a breakdown with x untouched.  The host looks every
 * check_every iterations and launches on while any column is running and fewer than max_iter iterations were issued.
 * iters_done[j] is column j's device counter, rel_residual[j] = sqrt(r.r / b.b) of its last iterate (b.b = 0: 1 in its place).
 * With plain storage column j therefore equals ehyb_bicgstab on b_j bit for bit -- x, iters_done and rel_residual -- for every
 * k, every check_every, graphs and plain launches (cfg.graphs = 2), and whatever the other columns do, but for rows the residual
 * splits into several segments (ehyb_spmm); with symmetric pair storage or a panel-form residual up to the order of summation.
 * If any column broke down the call returns EHYB_ERR_ARG ("breakdown" in ehyb_last_error) after every output is written.
 * Needs a plan over all rows.  EHYB_ERR_ARG for k < 1, ldb or ldx < n, a null plan, B or X, max_iter < 0, a negative or NaN rtol
 * or a plan not over all rows, checked in this order; EHYB_ERR_STATE on a plan never uploaded -- all before any device work.
 */
int ehyb_bicgstab_multi(ehyb_plan* plan, const double* inv_diag_dev, const double* B_dev, int64_t ldb, double* X_dev, int64_t ldx,
                        int k, int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual);

/*
 * CG with a Chebyshev polynomial preconditioner: the preconditioner that is all multiplies -- no triangular solve, no second
 * matrix format, no dot product inside.  Let [lmin, lmax] enclose the spectrum of D^-1 A, where D^-1 = inv_diag (NULL: the
 * identity, and the interval encloses the spectrum of A).  theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2,
 * sigma = theta / delta.  z = M^-1 r of degree m >= 0 is
 *   c0 = 1 / theta;  rho_0 = 1 / sigma
 *   d = c0 D^-1 r;  z = d;  w = r
 *   for j = 1 .. m:  t = A~ d;  w = w - t;  rho_j = 1 / (2 sigma - rho_{j-1});  a_j = rho_j rho_{j-1};  b_j = 2 rho_j / delta
 *                    d = a_j d + b_j D^-1 w;  z = z + d
 * A~ is the matrix of poly_plan; m multiplies per application; degree 0 is Jacobi scaled by 1 / theta.  With z = p(D^-1 A) D^-1 r,
 * 1 - lambda p(lambda) = T_{m+1}((theta - lambda) / delta) / T_{m+1}(sigma), and p > 0 on (0, lmax].  p can turn negative just
 * above lmax (degree 1 does at 1.1 lmax): lmax MUST be an upper bound of the spectrum, or CG breaks down.  lmin need not be a
 * lower bound: it only says where the polynomial stops trying.
 *
 * ehyb_cheb_coeffs (host only): c0 and a[j-1], b[j-1] for j = 1 .. degree, computed in the order stated above.  EHYB_ERR_ARG
 * for a degree outside 0 .. EHYB_CHEB_MAX_DEGREE, unless 0 < lmin < lmax < inf, or a null output that would be written.
 *
 * ehyb_lambda_max: `iters` steps of the power method on D^-1 A from v_i = 1 + (i mod 7) / 8, v <- D^-1 A v / ||D^-1 A v||_2;
 * *lambda = (v.Av) / (v.Dv) of the last v -- a Rayleigh quotient: never above the largest eigenvalue in exact arithmetic, so a
 * caller multiplies it by a safety factor.  iters + 1 multiplies (walks alternating) and as many launches of one small kernel;
 * the norms stay on the device.  Stream and plan as for a solve; EHYB_ERR_ARG for iters < 1, and -- after *lambda is written --
 * for an estimate that is not a positive finite number.
 *
 * ehyb_pcg_cheb: x_dev, b_dev, stream, check_every, outputs and stopping as ehyb_pcg; iters_done is the check point at which the
 * solve stopped, as in ehyb_pcg_multi.  poly_plan NULL = plan; otherwise any uploaded plan over all rows with the same number of
 * rows -- the intended one is the cfg.val_f32 = 1 plan of the same reordered matrix (half the value bytes per multiply of the
 * polynomial; the CG around it stays in fp64 on `plan`, so the answer is an fp64 answer without an outer refinement loop); a
 * panel-form plan works too, the polynomial only calls the multiply.  lmax <= 0: estimated, 1.1 * ehyb_lambda_max(poly_plan,
 * inv_diag_dev, 20) on the solve's stream.  lmin <= 0: lmax / 30.  The 20 steps, the factor 1.1 and the ratio 30 are the defaults
 * hypre and Ifpack2 ship for their Chebyshev smoothers: defaults, not values tuned on this library's matrices.
 * Per iteration: q = A p on `plan`, p.q (a dot kernel of its own: cfg.cg_fused_dot is ignored), the update kernel of ehyb_pcg
 * without a preconditioner (x += alpha p, r -= alpha q, r.r), the polynomial -- one start kernel, then `degree` rounds of a
 * multiply on poly_plan and one step kernel; whichever kernel finishes z also reads r and leaves the partials of r.z --, and
 * the direction kernel p = z + beta p.  Every multiply states its walk, alternating along the sequence each plan sees; an even
 * and an odd iteration are replayed from one hipGraph, cfg.graphs = 2 issues the same launches unrecorded.  With plain storage
 * x, iters_done and rel_residual are the same bits from run to run, for graphs and plain launches.
 * Breakdown (EHYB_ERR_ARG, "breakdown" in ehyb_last_error, after every output is written, rel_residual NaN): r.r or r.z NaN at
 * a check point, or an r.z <= 0 there short of convergence -- the polynomial was not positive on the spectrum.
 * EHYB_ERR_ARG, in this order: what ehyb_pcg rejects (a null plan, b or x, max_iter < 0, a negative or NaN rtol, a plan not over
 * all rows); a degree outside 0 .. EHYB_CHEB_MAX_DEGREE; lmin >= lmax when both are positive; a NaN bound; a poly_plan with
 * another number of rows, or one that does not cover all rows.  Then EHYB_ERR_STATE for a plan, then a poly_plan, that was never
 * uploaded.  All before any device work.  (A given lmin that turns out >= an estimated lmax is EHYB_ERR_ARG after the estimate.)
 *
 * ehyb_pcg_cheb_multi is ehyb_pcg_multi with this preconditioner: B, X, ldb, ldx, k, the per-column freezing at check points and
 * the outputs as there (k < 1 and ldb, ldx < n are rejected first).  One ehyb_spmm of the k directions on `plan` and `degree`
 * ehyb_spmm of the k columns of d on poly_plan per iteration, each ceil(k / ehyb_spmm_max_k) passes: a cfg.val_f32 plan has
 * k_max = 1 and runs k passes of width 1.  The coefficients are the same for every column.  With plain storage column j equals
 * ehyb_pcg_cheb on b_j bit for bit -- it is the same driver --, but for rows the residual splits into several segments (ehyb_spmm).
 *
 * ehyb_cheb_start_step / ehyb_cheb_step: the two kernels one launch at a time with slot_doubles / 2 workgroups, as the
 * ehyb_cg_*_step calls.  start: d = z = c0 D^-1 r.  step: w_out = w_in - t, d = a d + b D^-1 w_out, z += d; w_out may be w_in.
 * rz = -1: no sum, s_dev is not touched (and r_dev of the step not read); rz = 0 / 1: the partials of r.z go to r.z slot number
 * rz of ehyb_cg_layout (slot rz0 + 2 rz).  EHYB_ERR_ARG for n < 0, another rz or a null pointer that would be used.
 */
#define EHYB_CHEB_MAX_DEGREE 16
/* host only: c0 and a[j-1], b[j-1] for j = 1..degree, computed in the order stated above */
int ehyb_cheb_coeffs(double lmin, double lmax, int degree, double* c0, double* a, double* b);
int ehyb_lambda_max(ehyb_plan* plan, const double* inv_diag_dev, int iters, void* stream, double* lambda);
int ehyb_pcg_cheb(ehyb_plan* plan, ehyb_plan* poly_plan, const double* inv_diag_dev, const double* b_dev, double* x_dev,
                  int degree, double lmin, double lmax, int max_iter, double rtol, int check_every, void* stream,
                  int* iters_done, double* rel_residual);
int ehyb_pcg_cheb_multi(ehyb_plan* plan, ehyb_plan* poly_plan, const double* inv_diag_dev, const double* B_dev, int64_t ldb,
                        double* X_dev, int64_t ldx, int k, int degree, double lmin, double lmax, int max_iter, double rtol,
                        int check_every, void* stream, int* iters_done, double* rel_residual);
int ehyb_cheb_start_step(int n, const double* r_dev, const double* inv_diag_dev, double c0, double* d_dev, double* z_dev,
                         double* s_dev, int rz, void* stream);
int ehyb_cheb_step(int n, const double* w_in_dev, const double* t_dev, const double* inv_diag_dev, double a, double b,
                   double* w_out_dev, double* d_dev, double* z_dev, const double* r_dev, double* s_dev, int rz, void* stream);

/*
 * Two-level PCG with an aggregate coarse space: what removes the low end of the spectrum of D^-1 A, which no polynomial in A
 * reaches cheaply.  P is piecewise constant over aggregates of rows (Nicolaides' coarse grid correction, the two-level form of
 * aggregation AMG), E = P^T A P is dense (nc x nc, nc <= EHYB_COARSE_MAX) and inverted once on the host, and
 *   z = M^-1 r = D^-1 r + P E^-1 P^T r          (D^-1 = inv_diag, NULL: the identity)
 * costs three small streaming kernels per iteration and no multiply.  The additive form only: z = c + D^-1 (r - A c) costs one
 * more multiply and gave the same iteration counts to within 3 in a prototype.
 *
 * Everything lives in the numbering of the matrix after ehyb_matrix_reorder -- the matrix the plan was built from, with its
 * partBoundary.  The host calls need no GPU; their results do not depend on the number of OpenMP threads (they run on the
 * calling thread's OpenMP setting, capped by ehyb_host_threads()).
 *
 * ehyb_coarse_map: the default map, map_out[i] in [0, *nc_out) for every row i (map_out: n int32 of the caller's).
 *   Growth.  For each partition [pb[p], pb[p+1]) in turn: the seed is the lowest row not yet in an aggregate; grow breadth-first
 *   from it over the entries of the visited rows in stored order, skipping columns outside the partition and rows already taken,
 *   until the aggregate holds agg_rows rows or the queue is empty; repeat until the partition is used up.
 *   Fragments.  Visit the partition's aggregates in order of rising size as grown, ties by number.  One that now holds fewer
 *   than agg_rows / 4 rows (4 rows < agg_rows) joins the aggregate of the same partition that its rows' entries point into most
 *   often (ties: the lowest number) and takes its rows along; one with no such neighbour stays.  The survivors keep their order.
 *   agg_rows <= 0: max(128, ceil(n dof / 1536)) -- the growth leaves about 5-10 % more aggregates than n / agg_rows, and the
 *   headroom keeps nc below EHYB_COARSE_MAX.
 *   dof > 1: the unknown of row i is the pair (aggregate, old(i) mod dof), old(i) the row's index before the reorder
 *   (reorderList inverted): one constant per displacement component of a dof-unknowns-per-node FEM matrix.  Only pairs that
 *   hold a row are numbered, in order of (aggregate, component).
 *   No aggregate crosses a partition boundary, so an unknown's rows lie within a few thousand consecutive indices.
 *   EHYB_ERR_ARG: a null pointer, dof < 1, a matrix without partition data, or nc > EHYB_COARSE_MAX -- the message names an
 *   agg_rows that would fit.
 * ehyb_coarse_create_host: the object for any map (nc in 1 .. EHYB_COARSE_MAX, every entry in range, no unknown empty: else
 *   EHYB_ERR_ARG).  E_cd = sum of a_ij over map[i] = c, map[j] = d: row c takes the entries of its rows, rows rising, in stored
 *   order; the lower triangle is mirrored, so E is symmetric bit for bit (the matrix is taken to be symmetric).  E = L L^T in
 *   fp64, E^-1 = L^-T L^-1 stored full, its lower triangle computed and mirrored; a sum's terms are dealt to eight running
 *   sums by their index and these added pairwise.  A pivot that is not a positive finite number: EHYB_ERR_ARG, "not positive
 *   definite" in ehyb_last_error.
 * ehyb_coarse_upload: MAP, ROW_PTR, ROWS and EINV to the device (EHYB_ERR_NO_DEVICE without one).  ehyb_coarse_destroy releases
 *   both sides; NULL is allowed.
 * ehyb_coarse_host_array: which = EHYB_COARSE_MAP int32[n], _ROW_PTR int32[nc + 1], _ROWS int32[n] (the transpose of MAP: the
 *   rows of unknown c are ROWS[ROW_PTR[c] .. ROW_PTR[c + 1]), rising), _E double[nc * nc], _EINV double[nc * nc] (row-major).
 *
 * ehyb_coarse_apply: z = M^-1 r, three launches on the stream.  One apply at a time per object (it owns T and C).
 *   restrict  T[c] = sum of r over the rows of unknown c        one wave per unknown
 *   solve     C = E^-1 T                                        one wave per row, T staged in LDS
 *   prolong   z[i] = inv_diag[i] r[i] + C[map[i]]               and, inside a solve, the partials of r.z
 *   Every sum runs in a fixed order, without atomics.
 * ehyb_pcg_coarse: x_dev, b_dev, stream, check_every, outputs and stopping as ehyb_pcg_cheb -- it is the same loop with another
 *   preconditioner.  Per iteration: q = A p, p.q, the update kernel of ehyb_pcg without a preconditioner, restrict, solve,
 *   prolong (which leaves the partials of r.z), the direction kernel p = z + beta p.  The multiplies state their walks,
 *   alternating; an even and an odd iteration are replayed from one hipGraph, cfg.graphs = 2 issues the same launches
 *   unrecorded.  With plain storage x, iters_done and rel_residual are the same bits from run to run, for graphs and plain
 *   launches, on any stream.  Breakdown (EHYB_ERR_ARG, "breakdown" in ehyb_last_error, after every output is written,
 *   rel_residual NaN): r.r or r.z NaN at a check point, or an r.z <= 0 there short of convergence.
 *   In this order: EHYB_ERR_ARG for what ehyb_pcg rejects, then for a null coarse object or one with another number of rows;
 *   EHYB_ERR_STATE for a plan, then a coarse object, that was never uploaded.  All before any device work.
 * ehyb_pcg_coarse_multi is ehyb_pcg_multi with this preconditioner (k < 1 and ldb, ldx < n are rejected first); the kernels take
 *   up to four columns per launch and share the index loads and the rows of E^-1.  With plain storage column j equals
 *   ehyb_pcg_coarse on b_j bit for bit -- it is the same driver.
 * ehyb_coarse_restrict_step / _solve_step / _prolong_step: the three kernels one launch at a time with the grids the solver
 *   uses (prolong: slot_doubles / 2 workgroups, as ehyb_cheb_start_step).  t_dev and c_dev hold nc doubles.  rz = -1: no sum,
 *   s_dev is not touched; rz = 0 / 1: the partials of r.z go to r.z slot number rz of ehyb_cg_layout.
 * ehyb_coarse_create_raw (for tests of the kernels): an object from a map and a caller's E^-1 (nc * nc doubles, row-major)
 *   for n rows; its _E array is empty.
 */
#define EHYB_COARSE_MAX 2048
enum { EHYB_COARSE_MAP = 0, EHYB_COARSE_ROW_PTR = 1, EHYB_COARSE_ROWS = 2, EHYB_COARSE_E = 3, EHYB_COARSE_EINV = 4 };
typedef struct ehyb_coarse ehyb_coarse;
int  ehyb_coarse_map(const matrixCOO* m, int agg_rows, int dof, int32_t* map_out, int* nc_out);
int  ehyb_coarse_create_host(const matrixCOO* m, const int32_t* map, int nc, ehyb_coarse** out);
int  ehyb_coarse_upload(ehyb_coarse* c);
void ehyb_coarse_destroy(ehyb_coarse* c);
int  ehyb_coarse_host_array(const ehyb_coarse* c, int which, const void** ptr, int64_t* count);
int  ehyb_coarse_apply(ehyb_coarse* c, const double* inv_diag_dev, const double* r_dev, double* z_dev, void* stream);
int  ehyb_pcg_coarse(ehyb_plan* plan, ehyb_coarse* c, const double* inv_diag_dev, const double* b_dev, double* x_dev, int max_iter,
                     double rtol, int check_every, void* stream, int* iters_done, double* rel_residual);
int  ehyb_pcg_coarse_multi(ehyb_plan* plan, ehyb_coarse* c, const double* inv_diag_dev, const double* B_dev, int64_t ldb, double* X_dev,
                           int64_t ldx, int k, int max_iter, double rtol, int check_every, void* stream, int* iters_done,
                           double* rel_residual);
int  ehyb_coarse_restrict_step(ehyb_coarse* c, const double* r_dev, double* t_dev, void* stream);
int  ehyb_coarse_solve_step(ehyb_coarse* c, const double* t_dev, double* c_dev, void* stream);
int  ehyb_coarse_prolong_step(ehyb_coarse* c, const double* r_dev, const double* inv_diag_dev, const double* c_dev, double* z_dev,
                              double* s_dev, int rz, void* stream);
int  ehyb_coarse_create_raw(int n, const int32_t* map, int nc, const double* einv, ehyb_coarse** out);

/*
 * A coarse space from near-null-space vectors: the tentative prolongator of smoothed-aggregation AMG, not smoothed.  The
 * piecewise-constant P above holds the translations of an elasticity operator and not its rotations; here the caller hands in
 * n x nv vectors B (rigid-body modes, [1, x, y], eigenvectors from ehyb_lobpcg ...) and P is block diagonal over aggregates: the
 * block of an aggregate is the locally orthonormalised restriction of B to its rows.  Everything else -- E = P^T A P, its
 * inverse, z = D^-1 r + P E^-1 P^T r, every solver call above, ehyb_lobpcg and ehyb_lobpcg_gen -- takes such a "vector object"
 * wherever it takes a plain one; objects of the calls above keep every array, every bit and every launch they had.
 *
 * ehyb_coarse_create_host_vecs: m the reordered matrix; agg[i] in [0, nagg) the aggregate of row i, every aggregate holding a
 *   row (ehyb_coarse_map(m, agg_rows, 1, ...) is the intended map); B column-major n x nv with leading dimension ldb >= n, in
 *   the permuted numbering, nv in 1 .. EHYB_COARSE_MAX_VECS.
 *   The local basis.  Per aggregate, its rows rising, the columns v = 0 .. nv - 1 in turn: norm0 = the norm of the restricted
 *   column; it is orthogonalised against the columns already kept by modified Gram-Schmidt, two passes; it is kept, and
 *   normalised, iff norm0 > 0 and the norm afterwards is at least EHYB_COARSE_VEC_CUT norm0 = 2^-20 norm0 (a design constant:
 *   what is left of a column below it is rounding of the columns before it rather than a direction).  Every sum is dealt to
 *   eight running sums by its index, added pairwise; threads share out aggregates, never the terms of a sum: the same bits for
 *   any OpenMP thread count.
 *   Numbering.  Aggregate-major: aggregate a owns the unknowns OFF[a] .. OFF[a + 1), one per kept column, nc = OFF[nagg].  An
 *   aggregate may keep none: its rows get the Jacobi term only.
 *   E = P^T A P, dense: row (a, j) takes the rows i of a, rising, and their entries in stored order; the entry a_ic adds
 *   (W_j[i] a_ic) W_j'[c] to column (agg[c], j'), j' rising.  The lower triangle is mirrored (E symmetric bit for bit) and
 *   inverted as above.  P has orthonormal columns, so E is positive definite whenever A is.
 *   EHYB_ERR_ARG: a null pointer, nv out of range, ldb < n, an agg entry out of range or an aggregate without a row, an entry
 *   of B that is not finite (the message names row and column), nc < 1, nc > EHYB_COARSE_MAX (the message names nc: fewer
 *   aggregates or vectors are needed), E not positive definite.
 * ehyb_coarse_host_array on a vector object: MAP, ROW_PTR and ROWS describe the aggregates (MAP = agg, ROW_PTR int32[nagg + 1]),
 *   _OFF int32[nagg + 1], _W double[nv * n]: column j of the local bases at W + j n, zero where an aggregate kept fewer than
 *   j + 1 columns.  A plain object has neither _OFF nor _W: EHYB_ERR_ARG.
 * ehyb_coarse_upload sends agg, OFF, ROW_PTR, ROWS, W and E^-1.  The solve kernel is the one above (T and C hold nc entries); two
 *   kernels replace restrict and prolong, chosen inside the launches by the kind of the object:
 *   restrict  T[OFF[a] + j] = sum over the rows i of a of W_j[i] r[i]     one wave per aggregate: a lane's terms by fma in rising
 *                                                                        order, then the shuffle tree
 *   prolong   z[i] = inv_diag[i] r[i] + sum_j W_j[i] C[OFF[agg[i]] + j]   by fma from 0 in rising j, over the kept columns only
 *   No atomics, no LDS adds; nothing of T, C or W outside an aggregate's own kept range is read.  The guarantees of
 *   ehyb_pcg_coarse carry over: with plain storage the same bits from run to run, under graph replay, on any stream, for any
 *   check_every, and column j of ehyb_pcg_coarse_multi is the single solve of b_j.
 *   Cost.  W is 8 n nv bytes on the device and is read twice per iteration (restrict and prolong) beside the multiply.  One wave
 *   sums a whole aggregate: a single global aggregate (pure deflation with a handful of vectors) is correct but slow.
 * ehyb_coarse_create_raw_vecs (for tests of the kernels): agg, OFF (OFF[0] = 0, 0 <= OFF[a + 1] - OFF[a] <= nv), W (nv columns,
 *   leading dimension ldw >= n) and E^-1 (nc * nc, nc = OFF[nagg]) as given; its _E array is empty.
 */
#define EHYB_COARSE_MAX_VECS 8
#define EHYB_COARSE_VEC_CUT 9.5367431640625e-07 /* 2^-20 */
enum { EHYB_COARSE_OFF = 5, EHYB_COARSE_W = 6 };
int  ehyb_coarse_create_host_vecs(const matrixCOO* m, const int32_t* agg, int nagg, const double* B, int64_t ldb, int nv,
                                  ehyb_coarse** out);
int  ehyb_coarse_create_raw_vecs(int n, const int32_t* agg, int nagg, const int32_t* off, const double* W, int64_t ldw, int nv,
                                 const double* einv, ehyb_coarse** out);

/*
 * PCG WITH A FACTORISED SPARSE APPROXIMATE INVERSE (FSAI): the incomplete-factorisation-class preconditioner whose apply is
 * two multiplies.  G is lower triangular on the pattern of tril(A) with G A G^T ~ I, M^-1 = G^T G, z = G^T (G r).  An incomplete
 * Cholesky factor would be applied by two triangular solves, chains of dependent levels; G and G^T are applied by the multiply
 * this library is about, on plans of their own.  Everything lives in the numbering of the matrix after ehyb_matrix_reorder,
 * and the matrix is taken to be symmetric: only its lower triangle (columns j <= i of row i) is read.  A column is taken to be
 * stored at most once per row.
 *
 * Definition.
 *   Pattern.  Row i of G holds the columns J_i = { j < i : a_ij is stored } + { i }, in rising order, m_i = |J_i|.  row_cap in
 *   1 .. EHYB_FSAI_MAX_ROW (<= 0: EHYB_FSAI_MAX_ROW, the dense block the factor kernel holds): where m_i > row_cap the row keeps i
 *   and the row_cap - 1 columns j < i of largest |a_ij|, ties to the lower column, still in rising order; such rows are counted.
 *   Values.  S = A[J_i, J_i] from the stored entries of the rows J_i (what is not stored is 0), its lower triangle (row k of S
 *   from row J_i[k] of A) mirrored.  S = L L^T in fp64 and row i of G solves L^T g = e_m: the textbook y / sqrt(y_m) with
 *   S y = e_m, and S g = e_m / g_m.  The order of every sum: the factorisation is right-looking -- for j = 0 .. m - 1 in turn
 *   L[j][j] = sqrt(S[j][j]), L[r][j] = S[r][j] / L[j][j], then S[r][c] <- S[r][c] - L[r][j] L[c][j] for j < c <= r, so an entry
 *   loses its terms in rising j; the solve runs from the last unknown up, g[r] = (e[r] - L[m-1][r] g[m-1] - ... - L[r+1][r] g[r+1]) /
 *   L[r][r], the terms taken off in falling c.  (The host rounds every product and difference; the device may fuse the two.)
 *   Fallback.  A pivot S[j][j] that is not a positive finite number sends the row to its Jacobi form, g_ii = 1 / sqrt(a_ii) and
 *   zeros elsewhere in the row; such rows are counted.  An a_ii that is itself missing or not a positive finite number:
 *   EHYB_ERR_ARG, "not positive definite" in ehyb_last_error.
 *
 * ehyb_fsai_create_host: pattern and values on the host (no GPU needed; the result does not depend on the number of OpenMP
 *   threads: rows are dealt to threads whole), then G as a matrix on m's partitions -- m's partBoundary, no second reorder; its
 *   graph is half of A's -- and its plan(s) from plan_cfg (NULL: the defaults) with sym_pairs off and value_map on.
 *   transpose_mode 0 (the default of the Python layer): a second plan, built from G^T; every sum in a fixed order.
 *   transpose_mode 1: one plan, G^T applied by ehyb_spmv_t on it -- half the device memory, the order of ehyb_spmv_t's atomic
 *   adds; a plan ehyb_spmv_t_supported refuses (cfg.val_f32, a residual in panel form) fails here with that call's words.
 *   plan_cfg->val_f32 = 1 is allowed in mode 0: the preconditioner then lives in fp32 on the device, the CG around it stays fp64.
 *   EHYB_ERR_ARG before any work: a null pointer, row_cap > EHYB_FSAI_MAX_ROW, a transpose_mode other than 0 / 1, a matrix
 *   without partition data.
 * ehyb_fsai_host_array: which = EHYB_FSAI_ROW_PTR int64[n + 1], _COLS int32[nnz(G)], _VALS double[nnz(G)] (G in CSR form, as
 *   create_host computed it: ehyb_fsai_set_values does not refresh it), _COUNTS int64[2] {capped rows, fallback rows} (the
 *   second as of the last numeric phase).
 * ehyb_fsai_plans: the plan of G and that of G^T (NULL in mode 1), for stats; they belong to the object.
 * ehyb_fsai_upload: the plan(s), and for the numeric phase A's row pointers and columns, G's pattern and the entry order of the
 *   G^T plan (the G plan's is the identity): 4 (nnz(A) + 2 nnz(G)) + 8 nnz(G) bytes and a few vectors beside the plans.
 *   ehyb_fsai_destroy releases both sides; NULL is allowed.
 * ehyb_fsai_set_values: the numeric phase again, on the device, for new values of A on the same pattern (the pattern of G stays,
 *   capped rows keep their columns).  values, count, entry_order, on_device: ehyb_plan_set_values' conventions exactly (count =
 *   the entries of A).  ehyb_fsai_factor_kernel gives each row of G to one wave (assembly of the block's lower triangle in LDS
 *   by matching the columns of the rows J_i against J_i, factorisation, solve, g in CSR order, the fallback rule with its count
 *   on the device), then one ehyb_plan_set_values(..., on_device = 1) per plan fills the value streams.  The call drains the
 *   stream once in between to read the counts: a non-positive diagonal entry or an entry_order value out of range is
 *   EHYB_ERR_ARG with the plans untouched.
 * ehyb_fsai_apply: t = G r, z = G^T t on the stream.  One apply at a time per object (it owns t).
 * ehyb_pcg_fsai / ehyb_pcg_fsai_multi: arguments (there is no inv_diag: G carries the scaling), stopping, breakdown, graphs and
 *   outputs as ehyb_pcg_coarse / ehyb_pcg_coarse_multi -- the same loop.  Per iteration: q = A p, p.q, the update kernel without
 *   a preconditioner, T = G R, the partials of r.z = t.t (fsai_tt_kernel, fixed-order sums), Z = G^T T, the direction kernel.
 *   k columns go through ehyb_spmm on G's plans (as wide as ehyb_spmm_max_k of each allows), in mode 1 column by column.  With
 *   plain storage and transpose_mode 0, x, iters_done and rel_residual are the same bits from run to run, for graphs and plain
 *   launches, on any stream and for any check_every, and column j of a k-column solve equals the one-vector solve.  Mode 1
 *   inherits the order of ehyb_spmv_t's atomic adds: reproducible up to the order of summation only.
 *   In this order: EHYB_ERR_ARG for what ehyb_pcg rejects, then for a null object or one with another number of rows;
 *   EHYB_ERR_STATE for a plan, then an object, that was never uploaded.  All before any device work.
 * ehyb_fsai_factor_step (for tests of the kernel): HOST arrays in and out -- A in CSR form (a_ptr int32[n + 1]), a pattern
 *   (g_ptr int64[n + 1], every row 1 .. EHYB_FSAI_MAX_ROW columns, rising, the diagonal last), g_out double[g_ptr[n]]; one launch of
 *   the factor kernel on `stream`, with the LDS of the pattern's longest row.  *fallback_rows (may be NULL): the device's count.
 * ehyb_fsai_tt_step: the partials of t.t (n doubles on the device) into r.z slot number rz (0 / 1) of ehyb_cg_layout, with the
 *   grid of the other *_step calls.
 * Out of scope: adaptive or powered patterns, an unsymmetric FSAI for GMRES and BiCGSTAB, several GPUs.
 */
#define EHYB_FSAI_MAX_ROW 64
enum { EHYB_FSAI_ROW_PTR = 0, EHYB_FSAI_COLS = 1, EHYB_FSAI_VALS = 2, EHYB_FSAI_COUNTS = 3 };
typedef struct ehyb_fsai ehyb_fsai;
int  ehyb_fsai_create_host(const matrixCOO* m, int row_cap, const ehyb_config* plan_cfg, int transpose_mode, ehyb_fsai** out);
int  ehyb_fsai_host_array(const ehyb_fsai* f, int which, const void** ptr, int64_t* count);
int  ehyb_fsai_plans(const ehyb_fsai* f, ehyb_plan** plan_g, ehyb_plan** plan_t);
int  ehyb_fsai_upload(ehyb_fsai* f);
void ehyb_fsai_destroy(ehyb_fsai* f);
int  ehyb_fsai_set_values(ehyb_fsai* f, const double* values, int64_t count, const int32_t* entry_order, int on_device, void* stream);
int  ehyb_fsai_apply(ehyb_fsai* f, const double* r_dev, double* z_dev, void* stream);
int  ehyb_pcg_fsai(ehyb_plan* plan, ehyb_fsai* f, const double* b_dev, double* x_dev, int max_iter, double rtol, int check_every,
                   void* stream, int* iters_done, double* rel_residual);
int  ehyb_pcg_fsai_multi(ehyb_plan* plan, ehyb_fsai* f, const double* B_dev, int64_t ldb, double* X_dev, int64_t ldx, int k, int max_iter,
                         double rtol, int check_every, void* stream, int* iters_done, double* rel_residual);
int  ehyb_fsai_factor_step(int n, const int32_t* a_ptr, const int32_t* a_cols, const double* a_vals, const int64_t* g_ptr,
                           const int32_t* g_cols, double* g_out, int* fallback_rows, void* stream);
int  ehyb_fsai_tt_step(int n, const double* t_dev, double* s_dev, int rz, void* stream);

/*
 * PCG WITH BLOCK INCOMPLETE CHOLESKY (BIC): block Jacobi whose blocks are IC(0) factors -- non-overlapping additive Schwarz --
 * applied as two triangular solves that never leave a workgroup's LDS.  The chains of dependent levels the FSAI section speaks
 * of are long only if the factor spans the matrix; here a factor spans one block of at most EHYB_BIC_MAX_BLOCK rows (what fits
 * the LDS of one workgroup), so a level ends at a workgroup barrier, not at a kernel boundary, and no workgroup waits for
 * another.  M^-1 = P^T (L L^T)^-1 P, L block diagonal.  Everything lives in the numbering of the matrix after
 * ehyb_matrix_reorder, and the matrix is taken to be symmetric: only its lower triangle (columns j <= i of row i) is read.  A
 * column is taken to be stored at most once per row.
 *
 * Definition.
 *   Blocks.  Every partition of m->partBoundary is cut into ceil(rows / cap) runs of consecutive rows of nearly equal length, the
 *   first runs one longer; cap = min(block_rows > 0 ? block_rows : infinity, EHYB_BIC_MAX_BLOCK); block_rows = 0: whole partitions
 *   (of at most EHYB_BIC_MAX_BLOCK rows).  Every block has at least one row (an empty partition gives none).
 *   Local order, internal to the object: PERM[p] is the row at position p; within a block the positions are a permutation of
 *   its rows.  EHYB_BIC_ORDER_STORED: the identity.  EHYB_BIC_ORDER_COLOUR: greedy colouring -- the rows of the block in rising
 *   order take the smallest colour no already-coloured in-block neighbour holds (both triangles count, the diagonal does not),
 *   positions by (colour, row).  Rows of one colour are independent of one another, so the levels never exceed the colours.
 *   Factor.  A_b: the block's entries with row and column inside it, in local order (an entry (i, j), j < i, of the matrix lands
 *   in row max(pos i, pos j), column min).  L on the pattern of tril(A_b), L L^T ~ A_b, row by row with columns c rising:
 *   l_ic = (a_ic - sum_k l_ik l_ck) / l_cc over the k < c present in both rows, rising k; l_ii = sqrt(a_ii - sum_k l_ik^2), rising
 *   k.  The host rounds every product and difference.  DINV[i] = 1 / l_ii is stored, and the solves multiply by it.
 *   Breakdown.  A pivot that is not a positive finite number refactors the WHOLE block from A_b + alpha diag(A_b) (a_ii + alpha
 *   a_ii, rounded twice), alpha = 2^-10, 2^-9, ..., 2^10 in turn; SHIFT[b] is the alpha that worked, 0 where none was needed.  If
 *   none works the block takes its Jacobi form: l_ii = sqrt(a_ii), the stored pattern stays with zero values, SHIFT[b] = -1.  An
 *   a_ii that is missing or not a positive finite number: EHYB_ERR_ARG, "not positive definite" in ehyb_last_error.
 *   Levels.  LEVEL_F[p] = 1 + max LEVEL_F[q] over the strictly lower entries (p, q) of row p, 0 if it has none; LEVEL_B[p] = 1 +
 *   max LEVEL_B[q] over the q > p with l_qp stored, 0 if there is none.
 *
 * ehyb_bic_create_host (no GPU needed; the result does not depend on the number of OpenMP threads: blocks are dealt to threads
 *   whole).  order: EHYB_BIC_ORDER_STORED / _COLOUR.  EHYB_ERR_ARG before any work: a null pointer, block_rows < 0, another
 *   order, a matrix without partition data, a column outside the matrix.
 * ehyb_bic_create_raw (for tests of the kernels): an object from a caller's strictly lower L in CSR form (block-local columns,
 *   rising) and dinv, with the identity order; the levels by the rule above.  EHYB_ERR_ARG: a column >= its row's position or
 *   outside the block, an unsorted row, an empty block or one longer than EHYB_BIC_MAX_BLOCK.
 * ehyb_bic_host_array: which = EHYB_BIC_BLOCK_PTR int32[nb + 1], _PERM int32[n], _ROW_PTR int64[n + 1], _COLS int32[nnz(L)]
 *   (block-local positions), _VALS double[nnz(L)] (L in CSR form in position order, strictly lower part), _DINV double[n],
 *   _LEVEL_F / _LEVEL_B int32[n], _SHIFT double[nb], _COUNTS int64[4] {blocks, shifted blocks, fallback blocks, most levels of
 *   any block in either direction}.
 * ehyb_bic_max_k: min(4, EHYB_BIC_MAX_BLOCK / longest block): the columns one launch of the apply kernel serves.
 * ehyb_bic_upload: two streams, one for the forward solve (the rows of L) and one for the backward solve (the rows of L^T: the
 *   values are stored twice, which keeps atomic adds out of the LDS and every sum in a fixed order).  A stream holds the rows
 *   grouped by level, within a level in falling length, a 16-bit block-local column per entry, laid out [entry][lane] so that
 *   consecutive lanes read consecutive addresses, pass by pass; a pass holds only the rows that reach it (the rows fall in
 *   length: jagged, not padded to the longest row).  Every value and column word is read once per apply: 10 bytes per entry
 *   and what a row lacks of its own last pass, 12 per row and direction, a word per round and per pass.  A row is summed by a
 *   group of g lanes, g a power of two 1 .. 64 chosen per level:
 *   the widest with rows_of_the_level * g <= the workgroup's threads and g <= mean row length of the level / 2 (a narrow level
 *   of long rows gets wide groups, a wide level of short rows one lane per row).  The workgroup has a quarter of the longest
 *   block's rows in threads, in whole waves, 64 .. 1024.  ehyb_bic_destroy releases both sides; NULL is allowed.
 *   ehyb_bic_stream_info: the bytes of the two streams, their entries without padding, the workgroup size.
 * ehyb_bic_apply: Z = P^T (L L^T)^-1 P R for k columns (ldr, ldz >= n) on the stream -- one workgroup per block, most expensive
 *   blocks first, the block's rows x kk doubles in LDS (kk <= ehyb_bic_max_k; wider calls go in passes), loaded through PERM,
 *   solved forward and backward in place, stored through PERM.  The only synchronisation is the workgroup barrier between
 *   levels; every thread executes the same number, taken from the block's record.  Lane j of a group adds its terms in rising
 *   stream order (fused multiply-adds), the group's sums go through a fixed shuffle tree: the bits of a column do not depend on k.
 * ehyb_bic_apply_step (for tests of the kernel): ehyb_bic_apply with the columns' flags, int[k] on the device, as the solver
 *   passes them: a column whose flag is 0 is left as it was.
 * ehyb_pcg_bic / ehyb_pcg_bic_multi: arguments (there is no inv_diag: L carries the scaling), stopping, breakdown, graphs and
 *   outputs as ehyb_pcg_fsai / ehyb_pcg_fsai_multi -- the same loop.  Per iteration: q = A p, p.q, the update kernel without a
 *   preconditioner, Z = M^-1 R (a column whose flag is 0 is left untouched), the partials of r.z (bic_rz_kernel, fixed-order
 *   sums, slot rz of ehyb_cg_layout), the direction kernel.  The plan of A may use any storage; the object reads m, not the
 *   plan.  With plain storage for A, x, iters_done and rel_residual are the same bits from run to run, for graphs and plain
 *   launches, on any stream and for any check_every, and column j of a k-column solve equals the one-vector solve.
 *   In this order: EHYB_ERR_ARG for what ehyb_pcg rejects, then for a null object or one with another number of rows;
 *   EHYB_ERR_STATE for a plan, then an object, that was never uploaded.  All before any device work.
 * Out of scope: fp32 storage of L, a numeric phase on the device, overlapping blocks, several GPUs.  (ILU for GMRES / BiCGSTAB: ehyb_bilu below.)
 */
#define EHYB_BIC_MAX_BLOCK 20480
enum { EHYB_BIC_ORDER_STORED = 0, EHYB_BIC_ORDER_COLOUR = 1 };
enum {
    EHYB_BIC_BLOCK_PTR = 0, EHYB_BIC_PERM = 1, EHYB_BIC_ROW_PTR = 2, EHYB_BIC_COLS = 3, EHYB_BIC_VALS = 4, EHYB_BIC_DINV = 5,
    EHYB_BIC_LEVEL_F = 6, EHYB_BIC_LEVEL_B = 7, EHYB_BIC_SHIFT = 8, EHYB_BIC_COUNTS = 9
};
typedef struct ehyb_bic ehyb_bic;
int  ehyb_bic_create_host(const matrixCOO* m, int block_rows, int order, ehyb_bic** out);
int  ehyb_bic_create_raw(int n, int nb, const int32_t* block_ptr, const int64_t* row_ptr, const int32_t* cols, const double* vals,
                         const double* dinv, ehyb_bic** out);
int  ehyb_bic_host_array(const ehyb_bic* f, int which, const void** ptr, int64_t* count);
int  ehyb_bic_max_k(const ehyb_bic* f);
int  ehyb_bic_upload(ehyb_bic* f);
void ehyb_bic_destroy(ehyb_bic* f);
int  ehyb_bic_stream_info(const ehyb_bic* f, int64_t* bytes, int64_t* entries, int* threads);
int  ehyb_bic_apply(ehyb_bic* f, const double* R_dev, int64_t ldr, double* Z_dev, int64_t ldz, int k, void* stream);
int  ehyb_bic_apply_step(ehyb_bic* f, const double* R_dev, int64_t ldr, double* Z_dev, int64_t ldz, int k, const int* active_dev, void* stream);
int  ehyb_pcg_bic(ehyb_plan* plan, ehyb_bic* f, const double* b_dev, double* x_dev, int max_iter, double rtol, int check_every,
                  void* stream, int* iters_done, double* rel_residual);
int  ehyb_pcg_bic_multi(ehyb_plan* plan, ehyb_bic* f, const double* B_dev, int64_t ldb, double* X_dev, int64_t ldx, int k, int max_iter,
                        double rtol, int check_every, void* stream, int* iters_done, double* rel_residual);

/*
 * BLOCK ILU(0) (BILU) FOR GMRES AND BICGSTAB: the unsymmetric counterpart of BIC.  M^-1 = P^T (L U)^-1 P, L unit lower and U upper,
 * block diagonal, L U ~ A_b on the pattern of every diagonal block A_b.  The blocks and the local order are ehyb_bic's, by the same
 * code (EHYB_BIC_MAX_BLOCK, EHYB_BIC_ORDER_*); the colouring counts every in-block off-diagonal entry (i, j) as an edge, both ways:
 * the pattern of A_b + A_b^T.  The device side is ehyb_bic's too: the same two streams, the same apply kernel
 * x = (x - sum v x[col]) * dinv -- forward with the strictly lower part of L and dinv = 1 (an exact multiply), backward with the
 * strictly upper part of U and dinv = 1 / u_ii --, the same upload, release, max_k and stream_info.
 *
 * Definition.
 *   A_b.  The entries of A with row and column inside the block, in local order (entry (i, j) lands in row pos i, column pos j);
 *   what lies outside the block is dropped (block Jacobi).  A column stored more than once in a row is summed first, in stored order.
 *   The diagonal is always part of the pattern: a row that stores none holds a zero there.  The pattern may be structurally
 *   unsymmetric; a row may lack entries below or above the diagonal.
 *   Factor.  Row-wise IKJ on the pattern, in place: for rows i rising, for the k < i of row i rising: l_ik = w_k / u_kk (a true
 *   division), then for the j > k of row k rising that row i holds: w_j = w_j - l_ik u_kj; what is left of row i right of the
 *   diagonal is U's, w_i = u_ii.  The host rounds every product and difference.  (L U)_ij = a_ij at every (i, j) of the pattern.
 *   U_DINV[i] = 1 / u_ii is stored, and the backward solve multiplies by it.
 *   Pivot rule.  s_i = sum_j |a_ij| over the block row (duplicates summed, columns rising).  u_ii is accepted if it is finite and
 *   |u_ii| > 2^-26 s_i.  Otherwise the WHOLE block is refactored from A_b + alpha diag(s) (a_ii + alpha s_i, rounded twice), alpha =
 *   2^-10, 2^-8, ..., 2^10 in turn -- s rather than a_ii, so a zero diagonal is cured too; SHIFT[b] is the alpha that worked, 0 where
 *   none was needed.  If none works the block takes its Jacobi form: no entries, U_DINV = 1 / a_ii (1 where a_ii is 0 or not
 *   finite), SHIFT[b] = -1.
 *   Levels.  LEVEL_F[p] = 1 + max LEVEL_F[q] over the entries (p, q) of L's row p, 0 if it has none; LEVEL_B[p] = 1 + max
 *   LEVEL_B[q] over the entries (p, q) of U's row p, 0 if it has none.  They differ where the pattern is unsymmetric.
 *
 * ehyb_bilu_create_host (no GPU needed; the same bits for any number of OpenMP threads: blocks are dealt to threads whole):
 *   arguments and EHYB_ERR_ARG as ehyb_bic_create_host, but that no diagonal is refused.
 * ehyb_bilu_create_raw (for tests of the kernels): both triangles in CSR form with block-local columns, rising, and 1 / u_ii; the
 *   identity order.  EHYB_ERR_ARG as ehyb_bic_create_raw, for either triangle.
 * ehyb_bilu_host_array: which = EHYB_BILU_BLOCK_PTR int32[nb + 1], _PERM int32[n], _L_ROW_PTR / _U_ROW_PTR int64[n + 1], _L_COLS /
 *   _U_COLS int32 (block-local positions), _L_VALS / _U_VALS double (the strict triangles in CSR form in position order), _U_DINV
 *   double[n], _LEVEL_F / _LEVEL_B int32[n], _SHIFT double[nb], _COUNTS int64[4] {blocks, shifted blocks, fallback blocks, most
 *   levels of any block in either direction}.
 * ehyb_bilu_max_k, _upload, _destroy, _stream_info, _apply (Z = P^T (L U)^-1 P R), _apply_step: as their ehyb_bic_* namesakes --
 *   the same code on the same streams; the bits of a column do not depend on k.
 *
 * ehyb_gmres_bilu: ehyb_gmres right-preconditioned with M instead of diag(A) -- A M^-1 y = b, x = M^-1 y, so the residual tested
 *   is the true one.  Every rule of ehyb_gmres holds as stated there (stop, breakdown, the counter, NULL outputs, the same bits
 *   from run to run, for graphs and plain launches and on any stream with plain storage).  z = M^-1 v_j is one launch of the apply
 *   kernel that reads column j of the basis where it lies (and returns at once after a stop); no second basis is kept (M is
 *   fixed: this is not flexible GMRES).  At a cycle's end the back substitution writes sum y_i v_i into w, one apply -- whatever
 *   the status -- makes z = M^-1 w, and gmres_add_kernel adds z to x (the pair walk of the other GMRES kernels; nothing if the
 *   cycle counted no step).  A cycle stays one hipGraph.
 * ehyb_bicgstab_bilu / ehyb_bicgstab_bilu_multi: ehyb_bicgstab / _multi in the textbook right-preconditioned form: p^ = M^-1 p,
 *   v = A p^, s = r - alpha v, s^ = M^-1 s, t = A s^, x += alpha p^ + omega s^, r = s - omega t, p = r + beta (p - omega v) on the
 *   unpreconditioned p (one vector more than ehyb_bicgstab).  Two applies per iteration, each ceil(k / ehyb_bilu_max_k) launches
 *   that skip a stopped column as the vector kernels do; the vector kernels are ehyb_bicgstab's with inv_diag = NULL.  Stop, breakdown,
 *   status words, check_every and outputs as ehyb_bicgstab(_multi); with plain storage column j equals the single solve of b_j bit
 *   for bit.
 *   In this order: EHYB_ERR_ARG for what the Jacobi solver rejects, then for a null factor or one with another number of rows;
 *   EHYB_ERR_STATE for a plan, then a factor, that was never uploaded.  All before any device work.
 * ehyb_bilu_gmres_combine_step / ehyb_bilu_gmres_add_step (building blocks, as the other ehyb_gmres_*_step): solve_x with the combination
 *   sum y_i v_i written to comb_dev and no x; x += z if J > 0 (J as in solve_x).  comb_dev, z_dev, x_dev 16-byte aligned.
 * Out of scope: a numeric phase on the device for new values on an unchanged pattern, ILU(k), ILUT, fp32 factors, overlapping
 * blocks, ehyb_gmres_t (it needs M^-T), MINRES and LSQR, several GPUs.
 */
enum {
    EHYB_BILU_BLOCK_PTR = 0, EHYB_BILU_PERM = 1, EHYB_BILU_L_ROW_PTR = 2, EHYB_BILU_L_COLS = 3, EHYB_BILU_L_VALS = 4,
    EHYB_BILU_U_ROW_PTR = 5, EHYB_BILU_U_COLS = 6, EHYB_BILU_U_VALS = 7, EHYB_BILU_U_DINV = 8, EHYB_BILU_LEVEL_F = 9,
    EHYB_BILU_LEVEL_B = 10, EHYB_BILU_SHIFT = 11, EHYB_BILU_COUNTS = 12
};
typedef struct ehyb_bilu ehyb_bilu;
int  ehyb_bilu_create_host(const matrixCOO* m, int block_rows, int order, ehyb_bilu** out);
int  ehyb_bilu_create_raw(int n, int nb, const int32_t* block_ptr, const int64_t* l_row_ptr, const int32_t* l_cols, const double* l_vals,
                          const int64_t* u_row_ptr, const int32_t* u_cols, const double* u_vals, const double* u_dinv, ehyb_bilu** out);
int  ehyb_bilu_host_array(const ehyb_bilu* f, int which, const void** ptr, int64_t* count);
int  ehyb_bilu_max_k(const ehyb_bilu* f);
int  ehyb_bilu_upload(ehyb_bilu* f);
void ehyb_bilu_destroy(ehyb_bilu* f);
int  ehyb_bilu_stream_info(const ehyb_bilu* f, int64_t* bytes, int64_t* entries, int* threads);
int  ehyb_bilu_apply(ehyb_bilu* f, const double* R_dev, int64_t ldr, double* Z_dev, int64_t ldz, int k, void* stream);
int  ehyb_bilu_apply_step(ehyb_bilu* f, const double* R_dev, int64_t ldr, double* Z_dev, int64_t ldz, int k, const int* active_dev, void* stream);
int  ehyb_gmres_bilu(ehyb_plan* plan, ehyb_bilu* f, const double* b_dev, double* x_dev, int restart, int ortho_passes, int max_iter,
                     double rtol, void* stream, int* iters_done, double* rel_residual);
int  ehyb_bicgstab_bilu(ehyb_plan* plan, ehyb_bilu* f, const double* b_dev, double* x_dev, int max_iter, double rtol, int check_every,
                        void* stream, int* iters_done, double* rel_residual);
int  ehyb_bicgstab_bilu_multi(ehyb_plan* plan, ehyb_bilu* f, const double* B_dev, int64_t ldb, double* X_dev, int64_t ldx, int k, int max_iter,
                              double rtol, int check_every, void* stream, int* iters_done, double* rel_residual);
int  ehyb_bilu_gmres_combine_step(int n, int64_t ld, const double* V_dev, double* comb_dev, double* s_dev, void* stream);
int  ehyb_bilu_gmres_add_step(int n, const double* z_dev, double* x_dev, double* s_dev, void* stream);

/*
 * The vector kernels of ehyb_pcg as building blocks for a caller that owns the loop -- the multi-GPU CG of
 * ehyb_spmv_gpu_amd/dist.py (HaloCG), where q = A p goes through the halo exchange.  s is the partial-sum
 * array: `slots` slots of `slot_doubles` doubles (ehyb_cg_layout).  Every rank launches the same grid, so an
 * all-reduce (sum) of a slot makes every rank's partials the element-wise global ones and the kernel that
 * needs the scalar adds them up as in the single-GPU solve.  cur (0/1) says which of the two r.z slots
 * holds the current r.z (number c lives in slot rz0 + 2 c, r.r in the slot between them, so what an
 * iteration writes is one contiguous range): it alternates from iteration to iteration.  All
 * asynchronous on `stream`.
 */
int ehyb_cg_layout(int* slots, int* slot_doubles, int* slot_bb, int* slot_pq, int* slot_rr, int* slot_rz0);
/* r = b - q, p = M^-1 r; partials of r.z (slot rz0), r.r, b.b */
int ehyb_cg_init_step(int n, const double* b_dev, const double* q_dev, const double* inv_diag_dev, double* r_dev, double* p_dev,
                      double* s_dev, void* stream);
/* partials of p.q */
int ehyb_cg_dot_step(int n, const double* p_dev, const double* q_dev, double* s_dev, void* stream);
/* alpha = r.z[cur] / p.q;  x += alpha p;  r -= alpha q;  partials of the new r.z (number cur ^ 1) and r.r */
int ehyb_cg_update_step(int n, const double* p_dev, const double* q_dev, const double* inv_diag_dev, double* x_dev, double* r_dev,
                        double* s_dev, int cur, void* stream);
/* beta = r.z[cur ^ 1] / r.z[cur];  p = M^-1 r + beta p   (the reference's kernelMyxpy, kernel.cu:288-296) */
int ehyb_cg_direction_step(int n, const double* r_dev, const double* inv_diag_dev, double* p_dev, const double* s_dev, int cur,
                           void* stream);

/*
 * The six vector kernels of ehyb_bicgstab as building blocks, one launch each with slot_doubles / 2 workgroups, for a caller
 * that issues the multiplies itself -- and the seam through which the tests look at one kernel at a time.  s_dev: `slots`
 * slots of `slot_doubles` doubles and one more double behind them whose ints are the flags: the status word at int
 * flag_status and the iteration counter at int flag_iters of (int*)(s_dev + slots * slot_doubles).  rho = rh.r number c (0/1)
 * lives in slot rho0 + 2 c, r.r in the slot between the two; cur (0/1, masked with & 1) says which holds the current rho.
 * thr = rtol^2.  Every step but init returns at once, writing nothing, when the status is not status_running on entry; a
 * step that sets the status writes nothing else.
 *   init       r = b - q, rh = r, p^ = M^-1 r; partials of rho (slot rho0), r.r, b.b.  Takes no flags: the caller zeroes them.
 *   dot        partials of rh.v
 *   s          alpha = rho[cur] / rh.v; a non-finite rho or alpha, a zero or non-finite rh.v: breakdown.  Else s = r - alpha v,
 *              s^ = M^-1 s, partials of s.s
 *   dot2       partials of t.s and t.t
 *   update     s.s <= thr b.b (b.b = 0: 1): the half step x += alpha p^, r = s, partials of r.r, counter + 1; the status stays.
 *              Else omega = t.s / t.t; a zero or non-finite t.t or a non-finite omega: breakdown.  Else x += alpha p^ + omega s^,
 *              r = s - omega t, partials of rho[cur ^ 1] and r.r, counter + 1
 *   direction  s.s <= thr b.b or r.r <= thr b.b: converged.  Else beta = (rho[cur ^ 1] / rho[cur]) (alpha / omega); a zero or
 *              non-finite rho[cur] or omega, a non-finite rho[cur ^ 1] or beta: breakdown.  Else
 *              p^ = M^-1 r + beta (p^ - omega M^-1 v)
 * Every scalar is recomputed from the partials in their slots: a kernel adds the first slot_doubles / 2 entries of a slot
 * and never looks at the rest.  All asynchronous on `stream`.
 */
typedef struct ehyb_bicgstab_slots {
    int32_t slots, slot_doubles;
    int32_t slot_bb, slot_rv, slot_ss, slot_ts, slot_tt, slot_rho0, slot_rr;
    int32_t flag_status, flag_iters, flag_count;
    int32_t status_running, status_converged, status_breakdown;
} ehyb_bicgstab_slots;
int ehyb_bicgstab_layout(ehyb_bicgstab_slots* out);
int ehyb_bicgstab_init_step(int n, const double* b_dev, const double* q_dev, const double* inv_diag_dev, double* r_dev, double* rh_dev,
                            double* p_dev, double* s_dev, void* stream);
int ehyb_bicgstab_dot_step(int n, const double* rh_dev, const double* v_dev, double* s_dev, void* stream);
int ehyb_bicgstab_s_step(int n, const double* r_dev, const double* v_dev, const double* inv_diag_dev, double* s_vec_dev,
                         double* sh_dev, double* s_dev, int cur, void* stream);
int ehyb_bicgstab_dot2_step(int n, const double* t_dev, const double* s_vec_dev, double* s_dev, void* stream);
int ehyb_bicgstab_update_step(int n, const double* p_dev, const double* sh_dev, const double* s_vec_dev, const double* t_dev,
                              const double* rh_dev, double* x_dev, double* r_dev, double* s_dev, int cur, double thr, void* stream);
int ehyb_bicgstab_direction_step(int n, const double* r_dev, const double* v_dev, const double* inv_diag_dev, double* p_dev,
                                 double* s_dev, int cur, double thr, void* stream);

/*
 * MINRES (Paige-Saunders) for a SYMMETRIC, possibly indefinite A x = b on the plan's matrix, entirely on the device -- the
 * solver for [H A^T; A 0] (ehyb_gen_kkt3d), where CG is not a method and BiCGSTAB pays two multiplies and can break down.  The
 * matrix must be symmetric; as for ehyb_cg the library does not check.  It runs on symmetric pair storage (cfg.sym_pairs).
 * inv_diag_dev: an optional POSITIVE diagonal preconditioner M^-1 = diag(inv_diag) in the permuted numbering -- MINRES needs an
 * SPD preconditioner, so a caller passes 1 / |a_ii|, and 1 where a_ii = 0; NULL = none.  Arguments, stream, check_every and
 * outputs as ehyb_bicgstab: x_dev holds the initial guess on entry and the solution on return, stream NULL = a private stream,
 * check_every <= 0 = 10 (odd values rounded up to even), outputs may be NULL, the plan must cover all rows.
 * Stored per column: x, two Lanczos residuals, two directions, z and q.  ra: the current residual, rb: the one before,
 * z = M^-1 ra; start: ra = b - A x0, beta_1^2 = ra.z, bb = b.M^-1 b (0: 1 in its place), the carried state
 * (dbar, eps, phibar, cs, sn, beta_old) = (0, 0, beta_1, -1, 0, 0).  Per iteration:
 *   q = A z;  alpha = (z.q) / beta^2;  r_new = q / beta - (alpha / beta) ra - (beta / beta_old) rb  (written over rb; the rb term
 *   is absent in the first iteration, which beta_old = 0 marks);  z = M^-1 r_new;  beta_new^2 = r_new.z
 *   delta = cs dbar + sn alpha;  gbar = sn dbar - cs alpha;  eps' = sn beta_new;  dbar' = -cs beta_new;
 *   gamma = sqrt(gbar^2 + beta_new^2);  cs' = gbar / gamma;  sn' = beta_new / gamma;  phi = cs' phibar;  phibar' = sn' phibar
 *   v = M^-1 ra / beta;  w_new = (v - eps wb - delta wa) / gamma  (written over wb);  x += phi w_new;  beta_old' = beta
 * and (ra, rb), (wa, wb) swap roles.  One multiply (walks alternating) and three vector kernels per iteration -- dot, lanczos,
 * update --; an even and an odd iteration are replayed from one hipGraph (cfg.graphs = 2: plain launches; cfg.cg_fused_dot is
 * ignored).  Sums are re-added from per-workgroup partials in a fixed order; the state is carried in two copies per column,
 * one per parity: an iteration of parity c reads copy c and workgroup 0 of its update kernel writes copy c ^ 1, so no launch
 * reads a word that it writes.  (beta_old is carried because beta_new^2 is written to the slot that held beta_old^2.)
 * Stopping and breakdown are decided on the device, by the rules of ehyb_bicgstab.  Converged: phibar^2 <= rtol^2 bb; phibar is
 * the recurrence for ||r|| in the M^-1 norm, the norm of bb (both 2-norms without a preconditioner), and rel_residual =
 * phibar / sqrt(bb).  The test is made at the start (0 iterations) and after every update: the update kernel leaves the status
 * alone, the dot kernel of the next iteration sees the same phibar and sets it, and at max_iter the host applies the same test
 * to what it read.  Breakdown: a non-finite bb, beta_1^2, z.q, beta_new^2 or gamma, a negative beta^2 (the preconditioner is not
 * positive), a beta_1^2 <= 0 or a zero gamma short of convergence -- the convergence test comes first.  (beta_new = 0 with
 * gamma != 0 is the last update: phibar' = 0.)  The kernel that meets a breakdown changes nothing and every later one returns at
 * once: x is the last iterate whose update had finite scalars, iters_done the device's counter.  With plain storage x, iters_done
 * and rel_residual are the same bits for every check_every, for graphs and plain launches, for a given or a private stream, and
 * from run to run.  A breakdown returns EHYB_ERR_ARG ("breakdown" in ehyb_last_error) after every output is written; so does a
 * NaN in b or x0, with x unchanged.  EHYB_ERR_ARG for a null plan, b or x, max_iter < 0, a negative or NaN rtol or a plan not over
 * all rows; EHYB_ERR_STATE on a plan never uploaded -- all before any device work.
 *
 * ehyb_minres_multi: k INDEPENDENT such solves that share the multiply (ehyb_spmm of the k columns of z) and run the three
 * vector kernels up to four columns wide.  B, X, ldb, ldx, k, iters_done, rel_residual as ehyb_bicgstab_multi; every column has
 * its own slots, state copies, status word and counter, and a column whose status is set is skipped by every vector kernel while
 * the others go on.  With plain storage column j equals ehyb_minres on b_j bit for bit -- x, iters_done and rel_residual -- for
 * every k, every check_every, graphs and plain launches, and whatever the other columns do, but for rows the residual splits
 * into several segments (ehyb_spmm); with symmetric pair storage or a panel-form residual up to the order of summation.  If any
 * column broke down the call returns EHYB_ERR_ARG after every output is written.  EHYB_ERR_ARG for k < 1, ldb or ldx < n, then
 * what ehyb_minres rejects, in this order; then EHYB_ERR_STATE -- all before any device work.
 *
 * The four vector kernels as building blocks, one launch each with slot_doubles / 2 workgroups, as the ehyb_bicgstab_*_step
 * calls.  s_dev: `slots` slots of `slot_doubles` doubles and tail_doubles more behind them: at double state_doubles * c +
 * state_* of the tail the state of parity c, at double flags_at the two ints of the flags (flag_status, flag_iters).  beta^2
 * number c (0/1) lives in slot slot_beta0 + c; cur (0/1, masked with & 1) is the parity of the iteration.  thr = rtol^2.
 * Every step but init returns at once, writing nothing, when the status is not status_running on entry; a step that sets the
 * status writes nothing else.
 *   init     r = b - q, z = M^-1 r; partials of r.z (slot beta0) and of b.M^-1 b.  Takes no tail: the caller plants the first
 *            state (phibar = sqrt of the sum of slot beta0) and the flags.
 *   dot      phibar[cur]^2 <= thr bb (bb = 0: 1): converged.  Else partials of z.q
 *   lanczos  a non-finite z.q, beta^2[cur] or alpha / beta, a beta^2[cur] <= 0, a non-finite beta / beta_old: breakdown.  Else
 *            r_new over rb, z = M^-1 r_new, partials of beta^2[cur ^ 1]
 *   update   the same conditions on z.q and beta^2[cur], a negative or non-finite beta^2[cur ^ 1], a zero or non-finite gamma,
 *            a non-finite delta or phi: breakdown.  Else w_new over wb, x += phi w_new, state copy cur ^ 1, counter + 1
 * All asynchronous on `stream`.
 */
int ehyb_minres(ehyb_plan* plan, const double* inv_diag_dev, const double* b_dev, double* x_dev, int max_iter, double rtol,
                int check_every, void* stream, int* iters_done, double* rel_residual);
int ehyb_minres_multi(ehyb_plan* plan, const double* inv_diag_dev, const double* B_dev, int64_t ldb, double* X_dev, int64_t ldx,
                      int k, int max_iter, double rtol, int check_every, void* stream, int* iters_done, double* rel_residual);
typedef struct ehyb_minres_slots {
    int32_t slots, slot_doubles;
    int32_t slot_bb, slot_zq, slot_beta0;
    int32_t tail_doubles, state_doubles;
    int32_t state_dbar, state_eps, state_phibar, state_cs, state_sn, state_beta_old;
    int32_t flags_at, flag_status, flag_iters, flag_count;
    int32_t status_running, status_converged, status_breakdown;
} ehyb_minres_slots;
int ehyb_minres_layout(ehyb_minres_slots* out);
int ehyb_minres_init_step(int n, const double* b_dev, const double* q_dev, const double* inv_diag_dev, double* r_dev, double* z_dev,
                          double* s_dev, void* stream);
int ehyb_minres_dot_step(int n, const double* z_dev, const double* q_dev, double* s_dev, int cur, double thr, void* stream);
int ehyb_minres_lanczos_step(int n, const double* q_dev, const double* ra_dev, double* rb_dev, const double* inv_diag_dev,
                             double* z_dev, double* s_dev, int cur, void* stream);
int ehyb_minres_update_step(int n, const double* ra_dev, const double* inv_diag_dev, const double* wa_dev, double* wb_dev,
                            double* x_dev, double* s_dev, int cur, void* stream);

/*
 * LSQR (Paige-Saunders) for min ||b - A x||_2 on the plan's matrix, entirely on the device: the solver for over- and
 * under-determined, inconsistent and singular systems (the minimum-norm solution) and, with damp > 0, for the Tikhonov problem
 * min ||b - A x||^2 + damp^2 ||x - x0||^2 -- what scipy.sparse.linalg.lsqr covers.  The plan is square: an m x n matrix is padded
 * with empty rows or columns to max(m, n) and b with zeros; the padded entries of every vector stay +0.0 throughout, so LSQR on
 * the padded system is LSQR on the rectangular one.  The method multiplies by A and by A^T:
 *   plan_t == NULL  every A^T multiply is ehyb_spmv_t(plan).  What ehyb_spmv_t_supported refuses is refused here with its message,
 *                   before any device work.  That multiply adds with atomics: results are reproducible up to the order of
 *                   summation only.
 *   plan_t          a plan of A^T in the numbering of `plan` (ehyb_matrix_reorder_like of the transpose of the unpermuted matrix,
 *                   then a plan with symmetric pairs off); same number of rows, over all rows.  The multiply is ehyb_spmv_walk /
 *                   ehyb_spmm on it, in a fixed order of summation.
 *   plan_t == plan  the caller's statement that A is symmetric; the only way to run on symmetric pair storage.
 * b_dev, x_dev, stream, check_every as ehyb_minres: x_dev holds the initial guess x0 on entry and the solution on return, stream
 * NULL = a private stream, check_every <= 0 = 10 (odd values rounded up to even).  info may be NULL.
 * Stored per column: x, the Lanczos vectors unnormalised -- U = beta u, V = alpha v, as ehyb_minres stores its residuals, so no
 * pass scales a vector --, the direction w and one product vector t.  Start:
 *   U = b - A x0;  beta_1^2 = U.U;  bnorm = beta_1;  t = A^T U;  V = t / beta_1;  alpha_1^2 = V.V;  w = V / alpha_1
 *   the carried state (rhobar, phibar, cs2, sn2, z, xxnorm, res2, anorm^2) = (alpha_1, beta_1, -1, 0, 0, 0, 0, 0) and the numbers
 *   of the stop tests (rnorm, arnorm, xnorm, bnorm) = (beta_1, alpha_1 beta_1, 0, beta_1).
 * Per iteration, with alpha, beta of the iteration before:
 *   t = A V;  U = t / alpha - (alpha / beta) U;  beta'^2 = U.U;  anorm^2 += alpha^2 + beta'^2 + damp^2
 *   beta' > 0:  t = A^T U;  V = t / beta' - (beta' / alpha) V;  alpha'^2 = V.V.   beta' = 0:  alpha' = 0, V untouched
 *   rhobar1 = hypot(rhobar, damp);  cs1 = rhobar / rhobar1;  sn1 = damp / rhobar1;  psi = sn1 phibar;  phibar = cs1 phibar
 *   rho = hypot(rhobar1, beta');  cs = rhobar1 / rho;  sn = beta' / rho;  theta = sn alpha';  rhobar' = -cs alpha'
 *   phi = cs phibar;  phibar' = sn phibar;  tau = sn phi
 *   x += (phi / rho) w;   alpha' > 0:  w = V / alpha' - (theta / rho) w
 *   delta = sn2 rho;  gbar = -cs2 rho;  rhs = phi - delta z;  zbar = rhs / gbar;  xnorm = sqrt(xxnorm + zbar^2)
 *   gamma = hypot(gbar, theta);  cs2' = gbar / gamma;  sn2' = theta / gamma;  z' = rhs / gamma;  xxnorm' = xxnorm + z'^2
 *   res2' = res2 + psi^2;  rnorm = sqrt(phibar'^2 + res2')  (phibar may be negative);  arnorm = alpha' |tau|
 * Two multiplies and three vector kernels per iteration -- ustep, vstep, update --; alpha^2 and beta^2 of iterations of parity c live
 * in slots of their own, so an even and an odd iteration differ in arguments only and are replayed from one hipGraph
 * (cfg.graphs = 2: plain launches).  Sums are re-added from per-workgroup partials in a fixed order, no atomics; the state is
 * carried in two copies per column, one per parity: an iteration of parity c reads copy c and workgroup 0 of its update kernel
 * writes copy c ^ 1, so no launch reads a word that it writes.
 * Stopping is decided on the device after every iteration, by the rules of ehyb_minres: the update kernel leaves the status alone,
 * the ustep kernel of the next iteration makes the tests on the state copy it reads, and the host makes the same tests on what
 * it read (at the start and at max_iter too).  In this order:
 *   test 1  rnorm <= btol bnorm + atol anorm xnorm       (anorm = sqrt(anorm^2): the Frobenius-norm estimate of [A; damp I])
 *   test 2  arnorm <= atol anorm rnorm
 * istop: 0 = beta_1 = 0 or alpha_1 = 0, x0 already solves, x untouched; 1, 2 = the test that held (at the start only test 1 with
 * btol >= 1 can hold); 7 = max_iter iterations done; -1 = breakdown.  beta' = 0 or alpha' = 0 is the lucky end, not a breakdown:
 * the update still runs and then arnorm = 0, so test 2 holds.  There is no condition-number limit (scipy's conlim).
 * Breakdown: a non-finite b.b, beta^2, alpha^2, rho or phi / rho, or a zero rho -- the convergence tests come first.  The kernel that
 * meets a breakdown changes nothing and every later one returns at once: x is the last iterate whose update had finite scalars,
 * iters the device's counter.  A breakdown returns EHYB_ERR_ARG ("breakdown" in ehyb_last_error) after every output is written; so
 * does a NaN in b or x0, with x unchanged.  With a plan_t in plain storage x and every field of info are the same bits for every
 * check_every, for graphs and plain launches, for a given or a private stream, and from run to run.
 * EHYB_ERR_ARG, in this order: a null plan, b or x; max_iter < 0; a negative or NaN damp, atol or btol; a plan not over all rows; a
 * plan_t of another dimension or not over all rows; with plan_t NULL what ehyb_spmv_t_supported refuses.  Then EHYB_ERR_STATE for
 * a plan, then a plan_t, never uploaded -- all before any device work.
 *
 * ehyb_lsqr_multi: k INDEPENDENT such solves that share the multiplies: ehyb_spmm on plan and on plan_t, as wide as
 * ehyb_spmm_max_k of each allows; with plan_t NULL the transposed side runs column by column.  The vector kernels run up to four
 * columns wide; every column has its own slots, state copies, status word and counter, and a column whose status is set is skipped
 * by every vector kernel while the others go on.  info: k entries or NULL.  With a plan_t in plain storage column j equals
 * ehyb_lsqr on b_j bit for bit, but for rows the residual splits into several segments (ehyb_spmm).  If any column broke down the
 * call returns EHYB_ERR_ARG after every output is written.  EHYB_ERR_ARG for k < 1, ldb or ldx < n, then what ehyb_lsqr rejects,
 * in its order.
 *
 * The six vector kernels as building blocks, one launch each with slot_doubles / 2 workgroups on k = 1 .. 4 columns of leading
 * dimension n.  s_dev: k sets of `slots` slots of `slot_doubles` doubles, column j's set at j * slots * slot_doubles, and behind
 * the last set k tails of tail_doubles: in column j's tail at double state_doubles * c + state_* the state of parity c, at double
 * flags_at the two ints of the flags (flag_status, flag_iters).  beta^2 and alpha^2 number c (0/1) live in slots slot_beta0 + c and
 * slot_alpha0 + c; cur (0/1, masked with & 1) is the parity of the iteration.  Every step but init and start returns at once,
 * writing nothing, when the status is not status_running on entry; a step that sets the status writes nothing else.
 *   init     U = b - t (t = A x0); partials of U.U (slot beta0) and of b.b.  Takes no tail
 *   start    V = t / beta_1 (t = A^T U, beta_1^2 from slot beta0); partials of V.V (slot alpha0).  A beta_1^2 that is zero or not
 *            finite: nothing is written.  Takes no tail: the caller plants the first state and the flags
 *   wstart   w = V / alpha_1 (slot alpha0); a zero or non-finite alpha_1^2: breakdown
 *   ustep    the stop tests on state copy cur: converged.  Else a non-finite or non-positive alpha^2[cur] or beta^2[cur] or a
 *            non-finite alpha / beta: breakdown.  Else U over U, partials of beta^2[cur ^ 1]
 *   vstep    the same conditions on alpha^2[cur], a non-finite beta^2[cur ^ 1] or beta' / alpha: breakdown.  beta^2[cur ^ 1] = 0:
 *            nothing.  Else V over V, partials of alpha^2[cur ^ 1]
 *   update   a non-finite beta^2[cur ^ 1] or (beta' > 0) alpha^2[cur ^ 1], a zero or non-finite rho, a non-finite phi / rho or
 *            theta / rho: breakdown.  Else x, w (alpha' > 0), state copy cur ^ 1, counter + 1
 * EHYB_ERR_ARG for n < 0, a null pointer, k outside 1 .. 4.  All asynchronous on `stream`.
 */
typedef struct ehyb_lsqr_info {
    int32_t istop;    /* 0 = x0 already solves (beta_1 = 0 or alpha_1 = 0), 1 = test 1, 2 = test 2, 7 = max_iter, -1 = breakdown */
    int32_t iters;    /* the device's counter */
    double  rnorm;    /* sqrt(||b - A x||^2 + damp^2 ||x - x0||^2) by the recurrence */
    double  arnorm;   /* estimate of ||A^T r - damp^2 (x - x0)|| */
    double  anorm;    /* Frobenius-norm estimate of [A; damp I] */
    double  xnorm;    /* estimate of ||x - x0|| */
} ehyb_lsqr_info;
int ehyb_lsqr(ehyb_plan* plan, ehyb_plan* plan_t, const double* b_dev, double* x_dev, double damp, double atol, double btol,
              int max_iter, int check_every, void* stream, ehyb_lsqr_info* info);
int ehyb_lsqr_multi(ehyb_plan* plan, ehyb_plan* plan_t, const double* B_dev, int64_t ldb, double* X_dev, int64_t ldx, int k,
                    double damp, double atol, double btol, int max_iter, int check_every, void* stream, ehyb_lsqr_info* info);
typedef struct ehyb_lsqr_slots {
    int32_t slots, slot_doubles;
    int32_t slot_bb, slot_beta0, slot_alpha0;
    int32_t tail_doubles, state_doubles;
    int32_t state_rhobar, state_phibar, state_cs2, state_sn2, state_z, state_xxnorm, state_res2, state_anorm2;
    int32_t state_rnorm, state_arnorm, state_xnorm, state_bnorm;
    int32_t flags_at, flag_status, flag_iters, flag_count;
    int32_t status_running, status_converged, status_breakdown;
} ehyb_lsqr_slots;
int ehyb_lsqr_layout(ehyb_lsqr_slots* out);
int ehyb_lsqr_init_step(int n, int k, const double* b_dev, const double* t_dev, double* u_dev, double* s_dev, void* stream);
int ehyb_lsqr_start_step(int n, int k, const double* t_dev, double* v_dev, double* s_dev, void* stream);
int ehyb_lsqr_wstart_step(int n, int k, const double* v_dev, double* w_dev, double* s_dev, void* stream);
int ehyb_lsqr_ustep_step(int n, int k, const double* t_dev, double* u_dev, double* s_dev, int cur, double atol, double btol,
                         void* stream);
int ehyb_lsqr_vstep_step(int n, int k, const double* t_dev, double* v_dev, double* s_dev, int cur, void* stream);
int ehyb_lsqr_update_step(int n, int k, const double* v_dev, double* w_dev, double* x_dev, double* s_dev, int cur, double damp,
                          void* stream);

/*
 * Restarted GMRES(restart) for a general (unsymmetric) A x = b on the plan's matrix, entirely on the device, right-preconditioned
 * with M = diag(A) -- the solver for the systems on which ehyb_bicgstab breaks down or diverges: its residual never grows, and it
 * breaks down only on a singular system.  inv_diag_dev, b_dev, x_dev, stream and the outputs as ehyb_bicgstab: inv_diag_dev NULL =
 * no preconditioner, x_dev holds the initial guess on entry and the solution on return, stream NULL = a private stream, outputs may
 * be NULL, the plan must cover all rows.  restart: 0 = 30, else 1 .. EHYB_GMRES_MAX_RESTART.  ortho_passes: 0 or 2 = classical
 * Gram-Schmidt applied twice (the default), 1 = one pass.  There is no check_every: the host looks once per restart cycle.
 * Stored: the basis V, column-major, restart + 1 columns with a leading dimension of n rounded up to even; z = M^-1 v_j, the
 * multiply's input; w, its output.  bb = b.b (0: 1 in its place), thr = rtol^2; every rule is decided on the device.
 *   Cycle start: w = A x; w = b - w; rr = w.w.  A non-finite bb or rr: breakdown (x unchanged if this is the first cycle).
 *     rr <= thr bb: converged.  Else beta = sqrt(rr), v_0 = w / beta, g~_0 = beta.
 *   Step j = 0 .. restart - 1: w = A (M^-1 v_j).  Per pass: c_i = v_i.w for i <= j, all from the same w; w -= sum c_i v_i;
 *     h_i += c_i.  h_{j+1} = sqrt(w.w).  Any non-finite h: breakdown.  The rotations i = 0 .. j-1 on the column:
 *     t = cs_i h_i + sn_i h_{i+1}; h_{i+1} = -sn_i h_i + cs_i h_{i+1}; h_i = t.  gamma = hypot(h_j, h_{j+1}); zero or non-finite:
 *     breakdown.  cs_j = h_j / gamma, sn_j = h_{j+1} / gamma, R[0 .. j, j] = (h_0 .. h_{j-1}, gamma), g~_{j+1} = -sn_j g~_j,
 *     g_j = cs_j g~_j; the step counts (counter + 1).  Then, in this order: g~_{j+1}^2 <= thr bb: converged; the unrotated
 *     h_{j+1} = 0: breakdown (a singular system); else v_{j+1} = w / h_{j+1}, a true division.
 *   Cycle end -- after `restart` steps, at convergence, at a breakdown, or when the counter reaches max_iter --, with J steps
 *     counted in the cycle: R y = g[0 .. J) by back substitution, x += M^-1 (sum y_i v_i).  Steps before a breakdown are applied:
 *     x is always the last iterate with finite scalars.
 * iters_done is the device's counter (never above max_iter), rel_residual = sqrt(rho / bb) with rho the latest of rr at a cycle
 * start and g~_{j+1}^2 after a step.  A breakdown, or a NaN in b or x0 (x then unchanged), returns EHYB_ERR_ARG ("breakdown" in
 * ehyb_last_error) after every output is written.
 * One multiply (walks alternating) and 2 * passes + 1 vector kernels per step -- dots, update per pass, then next.  The host knows
 * j for every launch of a cycle, so a whole cycle is captured once as a linear hipGraph and replayed per cycle (cfg.graphs = 2:
 * plain launches); a last partial cycle, when max_iter is not a multiple of restart, is issued as plain launches.  After a stop
 * inside a cycle the remaining vector kernels of the cycle return at once; its multiplies still run.  Sums are re-added from
 * per-workgroup partials in a fixed order, no atomics; no launch reads a word that it writes (but the counter, which one
 * workgroup owns); the rotation state is written by one workgroup only.  With plain storage x, iters_done and rel_residual are
 * the same bits from run to run, for a given or a private stream, and for graphs and plain launches; with symmetric pair storage
 * or a panel-form residual up to the order of summation.  The solver only calls the multiply, so every plan form works.
 * EHYB_ERR_ARG for what ehyb_bicgstab rejects, in its order (a null plan, b or x, max_iter < 0, a negative or NaN rtol, a plan
 * not over all rows), then for a restart outside 0 .. EHYB_GMRES_MAX_RESTART or ortho_passes outside 0 .. 2; then EHYB_ERR_STATE
 * on a plan never uploaded -- all before any device work.
 *
 * The five vector kernels as building blocks, one launch each with slot_doubles / 2 workgroups, as the ehyb_minres_*_step calls.
 * s_dev: `slots` slots of `slot_doubles` doubles and tail_doubles more behind them (ehyb_gmres_layout).  c_i lives in slot
 * slot_c0 + i; slot_ww holds the partials of r.r after start and of w.w after the last update.  The tail, in doubles: at
 * flags_at the ints status (flag_status) and counter (flag_iters); at cycle_at the int counter at the cycle start; rho_at, bb_at;
 * cs_at + i, sn_at + i, g_at + i (i < max_restart); gt_at + i: g~_i (i <= max_restart); h_at + p h_stride + i: the Hessenberg
 * column after pass p; r_at + j r_stride + i: R[i, j].  V_dev: basis column i at V_dev + i ld, ld even and >= n; V_dev, w_dev,
 * z_dev, x_dev and inv_diag_dev 16-byte aligned.  Every step but solve_x returns at once, writing nothing, when the status is not
 * status_running on entry.
 *   start    w = b - w (w = A x on entry); partials of w.w (slot_ww) and b.b (slot_bb)
 *   dots     partials of c_i = v_i.w for i < count (1 .. max_restart + 1), the columns in register groups of 8
 *   update   w -= sum_{i < count} c_i v_i, c_i from the partials; Hessenberg copy `pass` (0 / 1) = copy pass - 1 + c (pass 0: c);
 *            last != 0: the partials of w.w
 *   next     j = -1: the cycle start's tests on slot_ww and slot_bb; v_0 = w / sqrt(w.w), z = M^-1 v_0; g~_0, rho, bb and the
 *            counter at the cycle start.  j = 0 .. max_restart - 1: step j's column from Hessenberg copy passes - 1 and slot_ww,
 *            rotation, g, R, rho, counter and tests as stated above; v_{j+1} = w / h_{j+1} into column j + 1, z = M^-1 v_{j+1}
 *   solve_x  J = counter - counter at the cycle start (J <= 0: nothing); R y = g[0 .. J), x += M^-1 (sum_{i < J} y_i v_i).  Does
 *            not look at the status: the steps counted before a stop are applied.
 * EHYB_ERR_ARG for n < 0, a null pointer that would be used, a count, pass, j or passes outside its range, an odd ld or one
 * below n, a misaligned vector.  All asynchronous on `stream`.
 */
#define EHYB_GMRES_MAX_RESTART 64
int ehyb_gmres(ehyb_plan* plan, const double* inv_diag_dev, const double* b_dev, double* x_dev, int restart, int ortho_passes,
               int max_iter, double rtol, void* stream, int* iters_done, double* rel_residual);
/*
 * The same solver for the ADJOINT system A^T x = b on the plan of A: every argument, rule, output and error as ehyb_gmres, every
 * multiply an ehyb_spmv_t.  The diagonal of A^T is that of A, so inv_diag_dev means the same.  A cycle stays one hipGraph (the
 * multiply's memset node and launches in it).  What ehyb_spmv_t refuses (symmetric pair storage, a residual in panel form,
 * cfg.val_f32, column segments) is refused here with EHYB_ERR_ARG and the form named, after ehyb_gmres's own argument checks and
 * before any device work.  The multiply adds with atomics, so x, iters_done and rel_residual are reproducible only up to the order
 * of summation, from run to run and between graphs and plain launches.
 */
int ehyb_gmres_t(ehyb_plan* plan, const double* inv_diag_dev, const double* b_dev, double* x_dev, int restart, int ortho_passes,
                 int max_iter, double rtol, void* stream, int* iters_done, double* rel_residual);
typedef struct ehyb_gmres_slots {
    int32_t slots, slot_doubles;
    int32_t slot_bb, slot_ww, slot_c0;
    int32_t max_restart, tail_doubles;
    int32_t flags_at, flag_status, flag_iters, flag_count;
    int32_t cycle_at, rho_at, bb_at, cs_at, sn_at, gt_at, g_at, h_at, h_stride, r_at, r_stride;
    int32_t status_running, status_converged, status_breakdown;
} ehyb_gmres_slots;
int ehyb_gmres_layout(ehyb_gmres_slots* out);
int ehyb_gmres_start_step(int n, const double* b_dev, double* w_dev, double* s_dev, void* stream);
int ehyb_gmres_dots_step(int n, int64_t ld, const double* V_dev, const double* w_dev, int count, double* s_dev, void* stream);
int ehyb_gmres_update_step(int n, int64_t ld, const double* V_dev, double* w_dev, int count, double* s_dev, int pass, int last,
                           void* stream);
int ehyb_gmres_next_step(int n, int64_t ld, double* V_dev, const double* w_dev, const double* inv_diag_dev, double* z_dev,
                         double* s_dev, int j, int passes, double thr, void* stream);
int ehyb_gmres_solve_x_step(int n, int64_t ld, const double* V_dev, const double* inv_diag_dev, double* x_dev, double* s_dev,
                            void* stream);

/*
 * The nev largest or smallest (algebraic) eigenvalues of the plan's SYMMETRIC matrix and their eigenvectors, by thick-restart
 * Lanczos with full reorthogonalisation (classical Gram-Schmidt twice: the two passes of ehyb_gmres), the vectors on the device.
 * With scale_dev the operator is S A S, S = diag(scale) -- scale = 1 / sqrt(diag) gives the spectrum of D^-1 A.  The host looks
 * once per restart cycle: it solves the projected problem (at most 64 x 64, ehyb_sym_eig), decides convergence and uploads the
 * rotation.  Ritz values approach the ends of the spectrum from inside.  A MULTIPLE eigenvalue is found ONCE: this is Lanczos
 * from one start vector, whose Krylov space holds one vector of every eigenspace; no locking and no block version exist
 * (ehyb_lobpcg below is the block method for the smallest end; rounding can bring a second copy in after several restarts).
 *   nev 1 .. EHYB_EIGSH_MAX_NEV; which EHYB_EIG_LARGEST / _SMALLEST; basis 0 = min(max(2 nev + 1, 20), 64), else
 *   nev + 2 .. EHYB_EIGSH_MAX_BASIS; the effective basis m = min(basis, n); keep = nev + (m - nev) / 2 (ehyb_eigsh_basis).
 *   Start vector: v0_dev, NULL = that of ehyb_lambda_max, v_i = 1 + (i mod 7) / 8; normalised to v_0.  A zero or non-finite
 *     norm: breakdown.
 *   Step j (the basis holds v_0 .. v_j; k kept vectors, 0 in the first cycle; j = k .. m - 1): z = scale o v_j, w = A z,
 *     w = scale o w (the scalings only with scale_dev).  Twice: c_i = v_i.w for i <= j, all from the same w; w -= sum c_i v_i;
 *     h_i += c_i.  beta^2 = w.w.  Column j of the projected matrix: T[i, j] = T[j, i] = h_i.  Any non-finite h or beta^2:
 *     breakdown.  beta^2 <= 2^-90 (h.h + beta^2) -- the orthogonalisation removed all but 2^-45 of w --: an invariant subspace;
 *     the step counts, the cycle ends with J = j + 1 basis vectors and beta = 0, no v_{j+1} is written.  Else
 *     v_{j+1} = w / beta, a true division.
 *   Cycle end, J basis vectors (m unless invariant), on the host: the eigenpairs (theta, Y) of T[:J, :J], sorted from the wanted
 *     end (falling for LARGEST, rising for SMALLEST); res_i = |beta Y[J-1, i]|; want = min(nev, J); nconv = the number of
 *     leading pairs with res_i <= tol max_l |theta_l|, counting stops at the first that fails.  Stop when nconv == want, the
 *     subspace was invariant, or max_restarts restarts have been made.
 *   Restart: kk = min(keep, J - 1); new v_i = sum_l Y[l, i] v_l for i < kk, new v_kk = old v_J; T = diag(theta_0 .. theta_{kk-1});
 *     the next cycle starts at j = kk and its first column re-measures the arrow entries c_i ~ beta Y[J-1, i] through the full
 *     orthogonalisation: the host never plants them.
 * Outputs: evals[i] = theta_i for i < want; evecs_dev column i (at evecs_dev + i ldv) = sum_l Y[l, i] v_l, unit length, in the
 * permuted numbering; resid[i] = res_i; *found = want; *nconv, *multiplies (the number of A z), *restarts.  Host outputs may be
 * NULL, evecs_dev may be NULL (values only); ldv even and >= n, evecs_dev, scale_dev and v0_dev 16-byte aligned.  stream NULL = a
 * private stream.  EHYB_OK also when nconv < nev after max_restarts (as the solvers at max_iter) and when an invariant subspace
 * holds fewer than nev pairs.  A non-finite quantity: EHYB_ERR_ARG with "breakdown" in ehyb_last_error after every output is
 * written -- found = nconv = 0, evecs_dev untouched.
 * Per step: one multiply (walks alternating), with scale_dev one streaming kernel w = scale o w, then dots, update, dots, update
 * (the kernels of ehyb_gmres on its slots and tail) and next.  The first cycle (j = 0 .. m - 1) and a cycle after a short restart
 * (kk < keep) are plain launches; the steady cycle (j = keep .. m - 1) is captured once as a linear hipGraph and replayed
 * (cfg.graphs = 2: plain launches).  After a stop inside a cycle the remaining vector kernels return at once.  A restart is one
 * launch of the rotation kernel into a second buffer of keep + 1 columns and one device-to-device copy back; the final Ritz
 * vectors are the same kernel writing into evecs_dev.  The host arithmetic is deterministic and every device sum is re-added
 * from per-workgroup partials in a fixed order: with plain storage every output is the same bits from run to run, for graphs and
 * plain launches, for a given or a private stream; with symmetric pair storage or a panel-form residual up to the order of
 * summation.  The solver only calls the multiply, so every plan form works, cfg.val_f32 included.
 * EHYB_ERR_ARG, in this order and before any device work: a null plan; nev, which, basis outside their ranges or
 * max_restarts < 0; a negative or NaN tol; a plan not over all rows; an odd ldv or one below n with a non-NULL evecs_dev; a
 * misaligned evecs_dev, scale_dev or v0_dev.  Then EHYB_ERR_STATE on a plan never uploaded.
 *
 * ehyb_eigsh_basis (host only): *m = the effective basis for (nev, basis, n), *keep = nev + max(m - nev, 0) / 2; either may be
 * NULL.  No argument check.
 *
 * ehyb_sym_eig (host only, no device): the eigenpairs of the dense symmetric m x m matrix T (column-major, leading dimension
 * ldt, only the upper triangle i <= j is read), 1 <= m <= EHYB_EIGSH_MAX_BASIS + 1.  evals rising; Y column-major with leading
 * dimension m, orthonormal, column i the vector of evals[i].  Cyclic Jacobi in a fixed order: the same input gives the same bits.
 * EHYB_ERR_ARG for m out of range, ldt < m, a null pointer or a non-finite entry.
 *
 * The three new kernels one launch each with slot_doubles / 2 workgroups, on the slots and tail of ehyb_gmres_layout; vectors and
 * leading dimensions as the ehyb_gmres_*_step calls.  next and scale return at once, writing nothing, when the status is not
 * status_running; rotate does not look at it.
 *   next    j = -1: w.w from slot_ww; zero or non-finite: status_breakdown; else gt_at + 0 = sqrt(w.w), v_0 = w / sqrt(w.w) into
 *           column 0, z = scale o v_0 (scale_dev NULL: z = v_0).  j = 0 .. 63: beta^2 from slot_ww, h_0 .. h_j from Hessenberg
 *           copy 1; the rules of step j above: R[0 .. j, j] = h, gt_at + j + 1 = beta (0 if invariant), counter + 1; invariant
 *           sets status_converged, breakdown sets status_breakdown and writes nothing else; else column j + 1 and z.
 *   scale   w = scale o w
 *   rotate  dst[:, c] = sum_{l < mc} Y[l, c] src[:, l] for c < kc, the sum in rising l; mc 1 .. 65, kc 1 .. 64; Y_dev column-major
 *           with leading dimension mc; src and dst must not overlap, each with its own even leading dimension >= n.
 * EHYB_ERR_ARG for n < 0, a null pointer that would be used, j, mc or kc outside its range, an odd leading dimension or one
 * below n, a misaligned vector.  All asynchronous on `stream`.
 */
#define EHYB_EIGSH_MAX_BASIS 64
#define EHYB_EIGSH_MAX_NEV 16
enum { EHYB_EIG_LARGEST = 0, EHYB_EIG_SMALLEST = 1 };
int ehyb_eigsh(ehyb_plan* plan, const double* scale_dev, const double* v0_dev, int nev, int which, int basis, int max_restarts,
               double tol, double* evals, double* evecs_dev, int64_t ldv, void* stream, int* found, int* nconv, int* multiplies,
               int* restarts, double* resid);
int ehyb_eigsh_basis(int nev, int basis, int n, int* m, int* keep);
int ehyb_sym_eig(int m, const double* T, int ldt, double* evals, double* Y);
int ehyb_eigsh_next_step(int n, int64_t ld, double* V_dev, const double* w_dev, const double* scale_dev, double* z_dev,
                         double* s_dev, int j, void* stream);
int ehyb_eigsh_scale_step(int n, const double* scale_dev, double* w_dev, double* s_dev, void* stream);
int ehyb_eigsh_rotate_step(int n, int64_t ld_src, const double* src_dev, int64_t ld_dst, double* dst_dev, const double* Y_dev,
                           int mc, int kc, void* stream);

/*
 * The nsv LARGEST singular values of the plan's matrix with their left and right singular vectors -- what
 * scipy.sparse.linalg.svds(which="LM") covers --, by Golub-Kahan-Lanczos bidiagonalisation with full two-sided
 * reorthogonalisation (classical Gram-Schmidt twice on each side: the two passes of ehyb_gmres) and a thick restart with Ritz
 * vectors (Baglama and Reichel 2005, restarted as ehyb_eigsh restarts), the vectors on the device.  It works on A and A^T
 * directly: eigsh of A^T A would square the condition number, eigsh of [0 A; A^T 0] would double every vector and find every
 * sigma twice.  The host looks once per restart cycle: it takes the SVD of the projected matrix B (at most 64 x 64,
 * ehyb_small_svd), decides convergence and uploads the two rotations.  Ritz values approach the singular values from inside:
 * sigma_0 is never above ||A||_2 in exact arithmetic.  A MULTIPLE sigma is found ONCE, as ehyb_eigsh finds a multiple eigenvalue
 * once.  NOT covered: the smallest singular values (plain Ritz values converge too slowly there; harmonic Ritz values or
 * shift-and-invert would be needed), a block version, one-sided reorthogonalisation, more than one column per pass.
 * Setting.  The plan is over all rows and square: an m x n matrix goes in padded with empty rows or columns to max(m, n), as
 *   ehyb_lsqr takes it; the padded entries of every u and v are then 0 but for the start vector's share of a null space.  plan_t,
 *   plan_t == plan and plan_t == NULL mean what they mean for ehyb_lsqr: a plan of A^T in the numbering of `plan`; the caller's
 *   statement that A is symmetric (the only way to run on symmetric pair storage); every A^T multiply is ehyb_spmv_t(plan).
 *   nsv 1 .. EHYB_SVDS_MAX_NSV; basis 0 = min(max(2 nsv + 1, 20), 64), else nsv + 2 .. EHYB_SVDS_MAX_BASIS; the effective basis
 *   m = min(basis, n); keep = nsv + (m - nsv) / 2 (ehyb_svds_basis: the rule of ehyb_eigsh_basis, nsv for nev).
 *   Start vector: v0_dev, NULL = v_i = 1 + (i mod 7) / 8; normalised to p_0.  A zero or non-finite norm: breakdown.
 * Bases.  P holds the right vectors, m + 1 columns starting with p_0 = v0 / ||v0||; Q holds the left vectors, m columns; both
 *   column-major with leading dimension n + (n & 1).  The multiplies read their input straight from a basis column.
 * Step j, for j = k .. m - 1, where k kept triplets exist (0 in the first cycle):
 *   Left half.  w = A p_j.  Twice: c_i = q_i.w for i < j, all from the same w; w -= sum c_i q_i; h_i += c_i (at j = 0 only the norm
 *     is taken).  alpha^2 = w.w.  Column j of the projected matrix: B[i, j] = h_i for i < j.  A non-finite h or alpha^2:
 *     breakdown.  alpha^2 <= 2^-90 (h.h + alpha^2): a LEFT COLLAPSE -- A p_j lies in the span of Q.  The multiply counts; the cycle
 *     ends with J = j + 1 right vectors, Jl = j left vectors and beta = 0; no q_j is written.  Else B[j, j] = alpha = sqrt(alpha^2)
 *     and q_j = w / alpha, a true division.
 *   Right half.  w = A^T q_j.  Twice: dots and update against p_0 .. p_j.  Its coefficients g are checked for finiteness and
 *     otherwise discarded: B is measured by the left halves only.  beta^2 = w.w.  beta^2 <= 2^-90 (g.g + beta^2): an invariant
 *     subspace (a right collapse), J = Jl = j + 1 and beta = 0.  Else p_{j+1} = w / beta.
 *   The counter counts multiplies, two per full step.  After a collapse the remaining launches of the cycle return at once.  The
 *   host tells a left collapse from a right one by the parity of the multiplies the cycle made.
 *   The collapse rules are a net for EXACT cases (a zero matrix, an identity, a start vector in an invariant subspace): they ask
 *   that the orthogonalisation removed all but 2^-45 of w.  On a matrix that is rank-deficient only to rounding (a dense 12 x 12
 *   of rank 5) what is left of w is noise of relative size 1e-13, above the threshold: the solve runs on through noise vectors
 *   and still returns correct triplets, the extra ones with sigma near zero.
 * Cycle end, on the host.  B[:Jl, :J] = X Sigma Y^T by ehyb_small_svd, sigma falling.  res_i = |beta X[Jl - 1, i]|, which is
 *   ||A^T u_i - sigma_i v_i||; A v_i = sigma_i u_i holds by construction.  want = min(nsv, Jl).  nconv = the number of leading
 *   triplets with res_i <= tol sigma_0; counting stops at the first that fails.  Stop when nconv == want, on a collapse of either
 *   kind, or after max_restarts restarts.  A zero matrix collapses at j = 0 with Jl = 0: found = 0 and EHYB_OK.
 * Restart.  kk = min(keep, J - 1).  New p_i = P y_i and new q_i = Q x_i for i < kk; new p_kk = old p_J.  B = diag(sigma_0 ..
 *   sigma_{kk-1}).  The next cycle starts at j = kk; the left half of that step re-measures the arrow column beta X[J-1, i] through
 *   the full orthogonalisation: the host never plants it.  Two launches of the rotation kernel of ehyb_eigsh, P then Q, go through
 *   one spare buffer of keep + 1 columns, each with its device-to-device copy back; the final U and V are the same kernel writing
 *   into the caller's arrays.  Device vectors in all: 2 m + keep + 3.
 * Outputs: svals[i] = sigma_i for i < want; U_dev column i (at U_dev + i ldu) = Q x_i and V_dev column i (at V_dev + i ldv) = P y_i,
 * unit length, in the permuted numbering; resid[i] = res_i; *found = want; *nconv, *multiplies (A and A^T together), *restarts.
 * Any of the host outputs, U_dev and V_dev may be NULL; ldu (ldv) even and >= n where U_dev (V_dev) is given; U_dev, V_dev and
 * v0_dev 16-byte aligned.  stream NULL = a private stream.  EHYB_OK also when nconv < nsv after max_restarts and when a collapse
 * leaves fewer than nsv triplets.  A non-finite quantity: EHYB_ERR_ARG with "breakdown" in ehyb_last_error after every scalar
 * output is written -- found = nconv = 0, U_dev and V_dev untouched.
 * Per full step: two multiplies (A and A^T walk in opposite directions, alternating), four dots, four updates (the kernels of
 * ehyb_gmres on its slots and tail) and two launches of the one new kernel.  The first cycle and a cycle after a short restart
 * (kk < keep) are plain launches; the steady cycle (j = keep .. m - 1) is captured once as a linear hipGraph and replayed
 * (cfg.graphs = 2: plain launches).  The host arithmetic is deterministic and every device sum is re-added from per-workgroup
 * partials in a fixed order: with a plan_t in plain storage every output is the same bits from run to run, for graphs and plain
 * launches, for a given or a private stream; through ehyb_spmv_t (plan_t NULL: atomic adds), symmetric pair storage or a
 * panel-form residual up to the order of summation.
 * EHYB_ERR_ARG, in this order and before any device work: a null plan; nsv or basis outside its range or max_restarts < 0; a
 * negative or NaN tol; a plan not over all rows; a plan_t of another dimension or not over all rows; with plan_t NULL what
 * ehyb_spmv_t_supported refuses (the texts of ehyb_lsqr under the name ehyb_svds); an odd ldu or ldv or one below n with a
 * non-NULL array; a misaligned U_dev, V_dev or v0_dev.  Then EHYB_ERR_STATE for a plan, then a plan_t, never uploaded.
 *
 * ehyb_svds_basis (host only): ehyb_eigsh_basis with nsv for nev.  No argument check.
 *
 * ehyb_small_svd (host only, no device): M = X Sigma Y^T for the dense rows x cols matrix M (column-major, leading dimension ldm),
 * 1 <= cols <= rows <= EHYB_SVDS_MAX_BASIS + 1, by one-sided (Hestenes) cyclic Jacobi with a fixed pair order and a fixed sweep
 * limit: the same input gives the same bits.  sigma (cols) falling; X rows x cols, column-major with leading dimension rows,
 * orthonormal columns; Y cols x cols, leading dimension cols, orthogonal.  A zero sigma gets a completed orthonormal column of X.
 * Each factor ends with one Newton-Schulz step, Z += Z (I - Z^T Z) / 2, so that its defect is a few ulps whatever the rotations left.
 * The matrix itself is rotated, never M^T M, so a small sigma keeps its digits.  ehyb_svds hands it B^T -- tall when the collapse
 * was a left one -- and swaps the factors.  EHYB_ERR_ARG for sizes out of range, ldm < rows, a null pointer or a non-finite entry.
 *
 * The new kernel one launch with slot_doubles / 2 workgroups, on the slots and tail of ehyb_gmres_layout; dst_dev a basis with the
 * even leading dimension ld_dst >= n, dst_dev and w_dev 16-byte aligned.  It returns at once, writing nothing, when the status is
 * not status_running; a breakdown sets status_breakdown and writes nothing else.
 *   side 0 (left), j = 0 .. 63: alpha^2 from slot_ww, h_0 .. h_{j-1} from Hessenberg copy 1; the rules of the left half above:
 *           R[0 .. j - 1, j] = h, R[j, j] = alpha (0 at a collapse), counter + 1; a collapse sets status_converged and writes no
 *           vector; else column j of dst_dev (Q) = w / alpha.
 *   side 1 (right), j = 0 .. 63: beta^2 from slot_ww, g_0 .. g_j from Hessenberg copy 1, read for the tests only;
 *           gt_at + j + 1 = beta (0 at a collapse), counter + 1; else column j + 1 of dst_dev (P) = w / beta.
 *   side 1, j = -1: the start.  w.w zero or non-finite: status_breakdown; else gt_at + 0 = sqrt(w.w), column 0 = w / sqrt(w.w);
 *           the counter stays.
 * EHYB_ERR_ARG for n < 0 or a null pointer; then side or j outside its range; then an odd ld_dst or one below n, a misaligned
 * vector.  Asynchronous on `stream`.
 */
#define EHYB_SVDS_MAX_BASIS 64
#define EHYB_SVDS_MAX_NSV 16
int ehyb_svds(ehyb_plan* plan, ehyb_plan* plan_t, const double* v0_dev, int nsv, int basis, int max_restarts, double tol,
              double* svals, double* U_dev, int64_t ldu, double* V_dev, int64_t ldv, void* stream, int* found, int* nconv,
              int* multiplies, int* restarts, double* resid);
int ehyb_svds_basis(int nsv, int basis, int n, int* m, int* keep);
int ehyb_small_svd(int rows, int cols, const double* M, int ldm, double* sigma, double* X, double* Y);
int ehyb_svds_next_step(int n, int64_t ld_dst, double* dst_dev, const double* w_dev, double* s_dev, int side, int j, void* stream);

/*
 * The nev SMALLEST eigenpairs of the plan's SYMMETRIC matrix by LOBPCG (locally optimal block preconditioned conjugate gradients),
 * the vectors on the device.  Where ehyb_eigsh finds a multiple eigenvalue once and is slowest at the low end of a stiffness-like
 * spectrum, this is a block method (a block of nb vectors finds up to nb copies of an eigenvalue) that takes a preconditioner.
 * On a matrix whose wanted end is well separated ehyb_eigsh needs fewer multiplies (36 against 116 on the planted grid of the
 * tests): prefer it there, and for the largest end, which this solver does not do.
 *   Sizes.  nb = block, 0 = nev; 1 <= nev <= nb <= EHYB_LOBPCG_MAX_BLOCK = 8; nb <= n.  The trial basis S = [X (nb) | P (nb,
 *     absent in the first iteration) | W (na)] has mc = nb or 2 nb, + na <= 24 columns, column-major with the leading dimension
 *     ld = n rounded up to even, beside its image AS.  A second pair (S, AS) receives the rotation and the pairs swap by pointer:
 *     the solve allocates 12 nb vectors of ld doubles, nb more with a coarse object, and 2.3 MB of partial sums.
 *   Preconditioner.  T r = ehyb_coarse_apply(coarse, inv_diag_dev, r) with a coarse object, inv_diag o r with inv_diag_dev
 *     alone, r with neither.
 *   Start.  X = X0_dev (nb columns, column j at X0_dev + j ldx0), NULL: x_ij = ((h & 2047) - 1023.5) / 1024 for row i, column j
 *     with, in 32-bit unsigned arithmetic, h = (i + 1) 2654435761 + (j + 1) 40503; h ^= h >> 15; h *= 2246822519; h ^= h >> 13.
 *     AX = A X is one ehyb_spmm of nb columns; one Rayleigh-Ritz step on [X] alone gives theta and an orthonormal X.
 *   Iteration it = 0, 1, ...
 *     1. R_i = AX_i - theta_i X_i and res_i = ||R_i||_2 for all nb columns; nrm = max(max_l |theta_l|, anorm); column i is
 *        converged iff res_i <= tol nrm; nconv = the number of leading converged columns among the first nev.  Stop when
 *        nconv == nev or it == max_iter.
 *     2. Soft locking: the active columns are all non-converged columns of the block (a column may re-enter).  W = T R[:, active],
 *        na columns; AW = A W is one ehyb_spmm of na columns; multiplies += na.
 *     3. G = S^T S and H = S^T AS, mc x mc, on the device in one pass over the 2 mc columns.
 *     4. ehyb_lobpcg_rr on the host: theta (nb values, rising) and Y (mc x nb).  Yp = Y with its first nb rows zeroed.
 *     5. [X | P] = S [Y | Yp], [AX | AP] = AS [Y | Yp]: two launches of the rotation kernel of ehyb_eigsh with kc = 2 nb.
 *   The whole Gram matrix is used, its X-X block included, so a drift of X^T X is absorbed at every step; there is no separate
 *   orthogonalisation.  The host looks twice per iteration (after the residual norms, after the Gram matrices), so there is no
 *   hipGraph and cfg.graphs does not matter.  The solver only calls ehyb_spmm, so every plan form works; a plan built with
 *   cfg.lds_doubles = EHYB_LDS_MAX_DOUBLES / 4 multiplies four columns per pass, any other plan makes passes of width 1
 *   (ehyb_spmm_max_k).  Every device sum is re-added from per-workgroup partials in a fixed order on a grid that depends on n
 *   alone and the host arithmetic is deterministic: with plain storage every output is the same bits from run to run, on a given
 *   or a private stream.
 * Outputs: evals[i] = theta_i and resid[i] = res_i for i < nev; evecs_dev column i (at evecs_dev + i ldv) = X_i, nev columns;
 * *nconv, *iters_done = it at the stop, *multiplies (columns multiplied, the nb of the start included).  Host outputs and
 * evecs_dev may be NULL.  ldv and ldx0 even and >= n; evecs_dev, inv_diag_dev, X0_dev 16-byte aligned.  stream NULL = a private
 * stream.  max_iter = 0 is allowed: one multiply of nb columns, the first Rayleigh-Ritz step, the residuals.  EHYB_OK also when
 * nconv < nev at max_iter.  Breakdown -- a non-finite theta, res, G or H, or a basis of rank < nb in step 4 --: EHYB_ERR_ARG with
 * "breakdown" in ehyb_last_error after every output is written: nconv = 0, evals and resid NaN, iters_done and multiplies as they
 * stand, evecs_dev untouched.
 * EHYB_ERR_ARG, in this order and before any device work: a null plan; nev, block outside their ranges or max_iter < 0; a negative
 * or NaN tol, a negative or non-finite anorm; a plan not over all rows; nb > n; an odd ldv (ldx0) or one below n with a non-NULL
 * evecs_dev (X0_dev); a misaligned evecs_dev, inv_diag_dev or X0_dev; a coarse object with another number of rows.  Then
 * EHYB_ERR_STATE on a plan, then a coarse object, that was never uploaded.
 * Out of scope: the largest end, hard locking, nev > 8, several GPUs.  A mass matrix (K x = lambda M x) is ehyb_lobpcg_gen below.
 *
 * ehyb_lobpcg_rr (host only, no device, deterministic): the Rayleigh-Ritz step for the pencil (H, G), both mc x mc (1 .. 24),
 * column-major with leading dimension mc, only the upper triangles i <= j read; 1 <= nb <= min(8, mc).
 *   1. A non-finite entry or a negative G_ii: EHYB_ERR_ARG.
 *   2. Columns with G_ii == 0 are dropped; their rows of Y are 0.
 *   3. d_i = 1 / sqrt(G_ii), G^ = d G d with a unit diagonal.
 *   4. (sigma, U) = ehyb_sym_eig(G^); keep sigma_l > 2^-40 sigma_max; *rank = their count (may be NULL); fewer than nb:
 *      EHYB_ERR_ARG with "rank" in ehyb_last_error.
 *   5. Q = D U_keep Sigma^-1/2.    6. (theta, Z) = ehyb_sym_eig(Q^T H Q).    7. Y = Q Z[:, :nb], theta = theta[:nb].
 *   Every sum runs in rising index order.  theta: nb doubles, rising; Y: mc x nb, column-major with leading dimension mc,
 *   Y^T G Y = I.
 *
 * The two new kernels, each with its fixed-order sum, one call each; vectors and leading dimensions as the ehyb_gmres_*_step calls.
 *   gram   G = S^T S and H = S^T AS for the first mc (1 .. 24) columns, each of the 2 mc columns read once; the upper triangles
 *          are computed and mirrored bit for bit.  G_dev, H_dev: mc x mc, column-major with leading dimension mc.  min(ceil(n /
 *          128), 256) workgroups of 768 threads write their partial sums to slots of their own in scratch_dev
 *          (EHYB_LOBPCG_SCRATCH_DOUBLES doubles) and a second launch adds the slots in rising order.
 *   resid  R_c = AX_c - theta_c X_c for c < nb (1 .. 8), theta_dev nb doubles on the device; res2_dev[c] = R_c . R_c; for every
 *          bit c of active_mask (within the low nb bits) W column number (set bits of the mask below c) = inv_diag o R_c
 *          (inv_diag_dev NULL: R_c), column a at W_dev + a ldw.  Columns of W not listed and everything else stay untouched.
 *          slot_doubles / 2 workgroups leave partial sums in scratch_dev (4096 doubles); a second launch adds them in rising order.
 * EHYB_ERR_ARG for n < 0, a null pointer that would be used, mc, nb or the mask outside its range, an odd leading dimension or
 * one below n, a misaligned vector.  All asynchronous on `stream`.
 */
#define EHYB_LOBPCG_MAX_BLOCK 8
#define EHYB_LOBPCG_SCRATCH_DOUBLES 294912   /* 256 workgroups x 2 matrices x 24 x 24 */
int ehyb_lobpcg(ehyb_plan* plan, ehyb_coarse* coarse, const double* inv_diag_dev, const double* X0_dev, int64_t ldx0, int nev, int block,
                int max_iter, double tol, double anorm, double* evals, double* evecs_dev, int64_t ldv, void* stream, int* nconv,
                int* iters_done, int* multiplies, double* resid);
int ehyb_lobpcg_rr(int mc, const double* G, const double* H, int nb, double* theta, double* Y, int* rank);
int ehyb_lobpcg_gram_step(int n, int64_t ld, const double* S_dev, const double* AS_dev, int mc, double* G_dev, double* H_dev,
                          double* scratch_dev, void* stream);
int ehyb_lobpcg_resid_step(int n, int64_t ld, const double* X_dev, const double* AX_dev, int nb, const double* theta_dev,
                           const double* inv_diag_dev, unsigned int active_mask, int64_t ldw, double* W_dev, double* res2_dev,
                           double* scratch_dev, void* stream);

/*
 * The nev SMALLEST eigenpairs of the pencil K x = lambda M x: `plan` holds the symmetric K, M is symmetric positive definite and
 * given in exactly one of two forms:
 *   mass_plan      a consistent mass: an uploaded plan over all rows of a matrix with the same n in the same numbering (build
 *                  it from ehyb_matrix_reorder_like(M, K));
 *   mass_diag_dev  a lumped mass: n doubles on the device, 16-byte aligned, M = diag(mass_diag_dev).
 * The rules are ehyb_lobpcg's, with these changes and no others.
 *   Third image.  Beside S and AS the solve keeps BS = M S.  With a mass plan BS is stored: BX is one ehyb_spmm on the mass plan
 *     at the start, BW one ehyb_spmm of na columns per iteration (passes of the mass plan's own ehyb_spmm_max_k, the walk
 *     direction alternating from multiply to multiply as for K), [BX | BP] = BS [Y | Yp] a third launch of the rotation kernel.
 *     With a lumped mass BS is never stored: every kernel forms m o s (one rounding) where it reads s.
 *   Allocation.  With a mass plan 18 nb vectors of ld doubles, with a lumped mass 12 nb; nb more with a coarse object in either
 *     case; 2.3 MB of partial sums.
 *   Gram matrices.  G = S^T BS and H = S^T AS, upper triangles computed and mirrored, handed to the unchanged ehyb_lobpcg_rr: the
 *     Ritz vectors come out M-orthonormal, X^T M X = I.
 *   Residual.  R_i = AX_i - theta_i BX_i, res_i = ||R_i||_2 (the plain 2-norm).
 *   Convergence.  Column i is converged iff res_i <= tol max(bnorm max_l |theta_l|, anorm); bnorm is the caller's scale of ||M||,
 *     0 = 1.0.  With bnorm = 1 the rule is ehyb_lobpcg's.
 *   Preconditioner.  It acts on R and is built from K alone: a coarse object, inv_diag_dev, or neither.
 *   A mass that is not positive definite shows as a negative G_ii or a rank below nb in ehyb_lobpcg_rr: the breakdown of
 *     ehyb_lobpcg with its outputs.
 *   Counters.  *multiplies = columns multiplied by K, *mass_multiplies = columns multiplied by M (0 with a lumped mass).
 *   Every device sum keeps a fixed order: with plain storage of both plans every output is the same bits from run to run, on a
 *     given or a private stream.  With mass_diag_dev all 1.0 and bnorm = 1 every output is ehyb_lobpcg's, bit for bit.
 * EHYB_ERR_ARG in ehyb_lobpcg's order (a negative or non-finite bnorm beside anorm), with these after "a plan not over all rows":
 * both or neither of mass_plan and mass_diag_dev; a mass plan not over all rows or of another n; a misaligned mass_diag_dev.
 * Then EHYB_ERR_STATE on a plan, then a mass plan, then a coarse object, that was never uploaded.
 *
 * The two kernels of ehyb_lobpcg with a mass -- each is one body, built for no mass, a stored and a lumped one --, one call each with
 * the fixed-order second launch and the argument checks of ehyb_lobpcg_gram_step and ehyb_lobpcg_resid_step; exactly one of BS_dev
 * (BX_dev) and mass_diag_dev is given, else EHYB_ERR_ARG.
 *   gram_b   G = S^T BS and H = S^T AS with BS_dev, or BS = mass_diag o S formed on the way into the tile.  One pass: every
 *            column of S, AS and (if stored) BS is read once; scratch_dev as ehyb_lobpcg_gram_step
 *            (EHYB_LOBPCG_SCRATCH_DOUBLES).  Rows per lane, tile order, shuffle tree and grid are ehyb_lobpcg_gram_step's: with
 *            BS_dev equal to S_dev bit for bit, G and H are that call's bits.
 *   resid_b  R_c = AX_c - theta_c BX_c with BX_dev, or BX = mass_diag o X; everything else as ehyb_lobpcg_resid_step, whose
 *            bits come out with BX_dev equal to X_dev or a mass_diag of 1.0.
 */
int ehyb_lobpcg_gen(ehyb_plan* plan, ehyb_plan* mass_plan, const double* mass_diag_dev, ehyb_coarse* coarse,
                    const double* inv_diag_dev, const double* X0_dev, int64_t ldx0, int nev, int block, int max_iter, double tol,
                    double anorm, double bnorm, double* evals, double* evecs_dev, int64_t ldv, void* stream, int* nconv,
                    int* iters_done, int* multiplies, int* mass_multiplies, double* resid);
int ehyb_lobpcg_gram_b_step(int n, int64_t ld, const double* S_dev, const double* AS_dev, const double* BS_dev,
                            const double* mass_diag_dev, int mc, double* G_dev, double* H_dev, double* scratch_dev, void* stream);
int ehyb_lobpcg_resid_b_step(int n, int64_t ld, const double* X_dev, const double* AX_dev, const double* BX_dev,
                             const double* mass_diag_dev, int nb, const double* theta_dev, const double* inv_diag_dev,
                             unsigned int active_mask, int64_t ldw, double* W_dev, double* res2_dev, double* scratch_dev,
                             void* stream);

/* -------------------------------------------- harness pieces (solver_test.c) */

/*
 * Read ./path as Matrix Market coordinate real/integer/pattern, general or symmetric,
 * into a row-grouped COO exactly as matrixRead_unsym (solver_test.c:31-126: file order
 * kept) or matrixRead_sym (solver_test.c:127-265: lower triangle mirrored, totalNum =
 * 2*stored - dimension) build it, including rowIdx/numInRow/maxCol.  nParts,
 * vectorCacheSize and kernelPerPart are filled by ehyb_sizing.  pattern entries get 1.0.
 * All arrays are malloc()ed; release with ehyb_matrix_free.
 */
int ehyb_mm_read(const char* path, const ehyb_config* cfg, matrixCOO* out, int* is_symmetric);
int ehyb_mm_write(const char* path, const matrixCOO* m, int symmetric_lower_only);
/* Copy a CSR matrix (rowptr[n+1], cols, vals; 0-based) into a freshly malloc()ed row-grouped
 * matrixCOO, entry order preserved; sizing fields filled by ehyb_sizing. */
int ehyb_matrix_from_csr(int n, const int64_t* rowptr, const int* cols, const double* vals,
                         const ehyb_config* cfg, matrixCOO* out);
void ehyb_matrix_free(matrixCOO* m);
/*
 * Multi-GPU, rank-local build (no reference counterpart -- the reference is single-GPU).
 * m is a rank's square diagonal block after ehyb_matrix_reorder.  It grows n_ghost columns, one
 * per x entry the rank receives from other ranks, and the nnz_g coupling entries (gi[k] = row in
 * m's current numbering, gj[k] in [0, n_ghost), gv[k]); the n_ghost new rows stay empty and the
 * partition data is kept.  A plan over rows [0, old dimension) with cfg.n_top > 1 then multiplies
 * the ghost columns in phase 2 from x = [local x | receive buffer].
 */
int ehyb_matrix_append_ghosts(matrixCOO* m, int n_ghost, int64_t nnz_g,
                              const int* gi, const int* gj, const double* gv);
/*
 * The other direction (exchange "cover"): rows [row0, row0 + n_rows) of m -- empty so far, at or behind the last partition
 * boundary, inside the dimension ehyb_matrix_append_ghosts gave the matrix -- receive nnz entries (ri[k] in [0, n_rows) ascending,
 * cj[k] any column of m, v[k]): the FOREIGN rows of a rank, whose entries another rank handed over because shipping one partial sum
 * per row is cheaper than shipping the x entries of their columns.  They form new partitions of at most rows_per_part rows behind
 * the existing ones (nParts and partBoundary grow; rows_per_part <= 0: m->vectorCacheSize).  A plan over rows [0, row0 + n_rows) with
 * cfg.row_split = row0 then multiplies them with everything else.
 */
int ehyb_matrix_append_rows(matrixCOO* m, int row0, int n_rows, int64_t nnz, const int* ri, const int* cj, const double* v, int rows_per_part);

/* x[i]: srand(i); (rand()%200-100)/1000.0  -- solver_test.c:89-92, 228-231 (glibc rand). */
void ehyb_x_glibc(int n, double* x);

/*
 * Synthetic matrices (no .mtx files exist offline).  All deterministic,
 * integer-hash values v = ((h mod 200) - 100)/1000 with 0 replaced by 0.001.
 * Each fills a row-grouped, column-sorted matrixCOO like ehyb_mm_read does.
 */
/* config 3: block-circulant band, `band` entries per row inside blocks of `block` rows */
int ehyb_gen_banded(int n, int band, int block, const ehyb_config* cfg, matrixCOO* out);
/* audikw_1-like: nodes of a 3-D grid (truncated to n/dof nodes), dof unknowns per node,
 * 27-point node coupling plus hashed second-shell couplings with probability extra_ppm/1e6,
 * symmetric values; scramble != 0 applies a random relabelling of the nodes.            */
int ehyb_gen_fem3d(int n, int dof, int nx, int ny, int extra_ppm, int scramble, uint64_t seed,
                   const ehyb_config* cfg, matrixCOO* out);
/* audikw_1-like with a graded mesh: a smooth density field over the grid decides how many couplings a node
 * keeps (first shell: probability near_min + (1 - near_min) * g; second shell: far_max * g^3; g in [0,1] at the
 * sparser end of the coupling; both in parts per million), so row lengths spread like those of an
 * unstructured mesh -- (250000, 900000) with 3 unknowns per node: about 21 to 345 entries per row. */
int ehyb_gen_fem3d_graded(int n, int dof, int nx, int ny, int near_min_ppm, int far_max_ppm, int scramble, uint64_t seed,
                          const ehyb_config* cfg, matrixCOO* out);
/* The rows of block `block` of n_blocks such grids stacked along z (weak scaling: one block per
 * GPU, each rank generates only its own rows): dimension n*n_blocks, rows outside
 * [block*n, (block+1)*n) empty, every block labelled (scrambled) on its own, couplings reach two
 * grid layers into the neighbouring blocks.  (block, n_blocks) = (0, 1) is ehyb_gen_fem3d. */
int ehyb_gen_fem3d_block(int n, int dof, int nx, int ny, int extra_ppm, int scramble, uint64_t seed,
                         int block, int n_blocks, const ehyb_config* cfg, matrixCOO* out);
/* R-MAT (a,b,c,d)=(.57,.19,.19,.05), 2^scale rows, `edges` samples, duplicates merged */
int ehyb_gen_rmat(int scale, int64_t edges, uint64_t seed, const ehyb_config* cfg, matrixCOO* out);
/* The rows of row block `block` of n_blocks of that same matrix, for a process that owns one block (strong
 * scaling, one process per GPU): contiguous row ranges of about equal cost (edge samples + 2 per row); cuts
 * (n_blocks+1 ints, out) are the same on every process.  Dimension 2^scale, rows outside the block empty. */
int ehyb_gen_rmat_block(int scale, int64_t edges, uint64_t seed, int block, int n_blocks, int* cuts, const ehyb_config* cfg,
                        matrixCOO* out);
/* The same with the cost the cuts balance named: 0 = ehyb_gen_rmat_block's (a row costs its samples + 2); 1 = the cost under the "cover"
 * exchange (ehyb_halo_set_partials), where an entry is multiplied by the owner of its row if its column has the higher degree of the two
 * (the column's x entry travels) and by the owner of its column otherwise (a partial sum travels back): hub rows then cost their owner
 * little and the blocks of hub rows get more rows (work max / mean at 8 ranks 1.24 -> 1.05). */
int ehyb_gen_rmat_block_cost(int scale, int64_t edges, uint64_t seed, int block, int n_blocks, int cost_model, int* cuts, const ehyb_config* cfg,
                             matrixCOO* out);
/* The rows [row0, row1) of that same matrix, for a process whose row range was decided elsewhere (bench.py re-cuts the ranks' rows once
 * the cost of the "cover" exchange is known).  Dimension 2^scale, rows outside the range empty. */
int ehyb_gen_rmat_rows(int scale, int64_t edges, uint64_t seed, int row0, int row1, const ehyb_config* cfg, matrixCOO* out);
/* 2-D 5/9-point stencil plus `extra` random symmetric couplings (small test inputs) */
int ehyb_gen_stencil2d(int nx, int ny, int points, int extra, uint64_t seed,
                       const ehyb_config* cfg, matrixCOO* out);
/* unstructured-mesh stand-in: ceil(n/dof) random points in the unit cube (x, y = u^(grade_permille/1000): denser towards
 * one corner; 0 = uniform), every node coupled to its knn nearest neighbours, made symmetric, dof unknowns per node;
 * random labels, row lengths between (knn+1)*dof and ~2*knn*dof -- a check that thresholds fitted on lattices hold */
int ehyb_gen_mesh3d(int n, int dof, int knn, int grade_permille, uint64_t seed, const ehyb_config* cfg, matrixCOO* out);
/* nlpkkt-like 3-D KKT system: [H A^T; A 0] on an nx^3 grid */
int ehyb_gen_kkt3d(int nx, const ehyb_config* cfg, matrixCOO* out);

#ifdef __cplusplus
}
#endif
#endif /* EHYB_H */
