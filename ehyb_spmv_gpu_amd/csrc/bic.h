// The object behind ehyb_bic (include/ehyb.h): the block incomplete Cholesky preconditioner of ehyb_pcg_bic.  bic.cpp builds the
// host side (blocks, local order, the IC(0) factor of every diagonal block, levels, and the two device streams as host arrays; no
// GPU needed), ehyb_bic.hip uploads the streams, applies them and releases them.
#pragma once
#include <cstdint>
#include <vector>

#include "ehyb.h"

struct ehyb_bic;

namespace ehyb {

// What the apply kernel reads of one block.  Direction 0: the forward solve with L, 1: the backward solve with L^T.
struct BicBlock {
    int32_t row0, rows;  // the block's first position and its length
    int32_t nlev[2];     // levels of the direction: the barriers every thread of the workgroup executes
    int32_t nround[2];   // rounds of the direction (a level of more rows than the workgroup has lane groups takes several)
    int32_t rnd0[2];     // the block's first word in BicStreams::rounds
    int64_t cnt0[2];     // the block's first word in BicStreams::cnt
    int64_t ent0[2];     // the block's first entry in BicStreams::cols / vals
};

// The two streams, both directions in one set of arrays (direction 1 behind direction 0 of the same block).
//   rounds one word per round: rows of the round (bits 0-10) | log2(lanes per row) << 11 | last round of its level << 14 |
//          passes of the round's longest row << 15
//   cnt    one word per (round, pass): the rows of the round that still have entries in that pass -- the rows of a round fall
//          in length, so they are its first rows
//   meta   one word per (direction, position slot), slot = dir * n + row0 + the row's rank in its block's (level, falling
//          length, rising row) order: block-local row | row length << 16
//   dinv   1 / l_ii in slot order
//   cols, vals   per round, pass by pass, cnt * g entries: entry q = pass * g + lane of the round's row number `grp` at
//          [pass][grp * g + lane] -- consecutive lanes read consecutive addresses, and a pass holds no row that has run out
//          (jagged, not padded to the longest row); what a row lacks of its own last pass is the column kBicNoEntry
struct BicStreams {
    int threads = 0;  // the workgroup size the layout was made for
    std::vector<BicBlock> blocks;
    std::vector<int32_t> launch_order;  // blocks, most expensive first
    std::vector<uint32_t> rounds, cnt, meta;
    std::vector<double> dinv, vals;
    std::vector<uint16_t> cols;
    int64_t real_entries = 0;  // entries that are not padding, both directions
    int64_t bytes() const
    {
        return (int64_t)(vals.size() * 10 + meta.size() * 12 + (rounds.size() + cnt.size()) * 4 + blocks.size() * sizeof(BicBlock));
    }
};
constexpr uint16_t kBicNoEntry = 0xFFFF;

// the workgroup size for a longest block, and the lanes per row (log2) of a level of w rows whose lengths add up to `entries`
int bic_threads(int longest_block);
int bic_group_log2(int threads, int w, int64_t entries);
// One triangle of a block-diagonal factor, strictly off the diagonal, in CSR form over all positions (row_ptr [n + 1], cols
// block-local and rising in a row), the number its solve multiplies a row by (dinv [n]), and the levels of its solve (level [n]).
struct BicTriangle {
    const int64_t* row_ptr;
    const int32_t* cols;
    const double* vals;
    const double* dinv;
    const int32_t* level;
};
// The streams for workgroups of `threads` (bic_threads(longest block) at upload): tri[0] the strictly lower triangle of the forward
// solve, tri[1] the strictly upper one of the backward solve, each  x = (x - sum v x[col]) * dinv.  IC passes L, L^T and 1 / l_ii
// twice (the overload on ehyb_bic), ILU passes L with ones and U with 1 / u_ii (bilu.cpp).
void bic_build_streams(int n, int nb, const int32_t* block_ptr, const BicTriangle (&tri)[2], int threads, BicStreams* out);
void bic_build_streams(const ehyb_bic& f, int threads, BicStreams* out);

// What ehyb_bic and ehyb_bilu share of the host side (bic.cpp): the checks of *_create_host on the matrix, its blocks (block_ptr,
// nb, max_block of f), and the local order of one block -- perm[r0 .. r1) and pos[r0 .. r1), the block-local position of a row.
// both_triangles: the colouring counts every in-block off-diagonal entry as an edge (the pattern of A_b + A_b^T), not only
// those of the lower triangle (a symmetric matrix: the same graph).
int bic_check_matrix(const char* who, const matrixCOO* m, int block_rows, int order);
void bic_cut_blocks(const matrixCOO* m, int block_rows, ehyb_bic* f);
void bic_block_order(const matrixCOO* m, int r0, int r1, int order, bool both_triangles, int32_t* perm, int32_t* pos);
int bic_host_threads();

// What they share of the device side (ehyb_bic.hip): the streams S of f's blocks onto the device (f->perm with them), the apply
// on them -- k columns in passes of ehyb_bic_max_k; active NULL: every column, else column c is served where the int at
// active[c * astride] is nonzero (inverted: zero -- a solver's status word, 0 while the column runs) --, and the release.
int bic_upload_streams(const char* who, ehyb_bic* f, const BicStreams& S);
int bic_apply_columns(const ehyb_bic* f, void* stream, const double* R, long long ldr, double* Z, long long ldz, int k, const int* active,
                      int astride = 1, bool inverted = false);
void bic_release_device(ehyb_bic* f);

}  // namespace ehyb

struct ehyb_bic {
    int n = 0, nb = 0;
    int order = 0;      // EHYB_BIC_ORDER_*
    int max_block = 0;  // the longest block
    int64_t counts[4] = {0, 0, 0, 0};  // blocks, shifted blocks, fallback blocks, most levels of any block (EHYB_BIC_COUNTS)
    std::vector<int32_t> block_ptr;    // [nb + 1]
    std::vector<int32_t> perm;         // [n] the row at position p
    std::vector<int64_t> row_ptr;      // [n + 1] L in CSR form in position order, strictly lower part
    std::vector<int32_t> cols;         // [nnz(L)] block-local positions, rising in a row
    std::vector<double> vals;          // [nnz(L)]
    std::vector<double> dinv;          // [n] 1 / l_ii
    std::vector<int32_t> level_f, level_b;  // [n]
    std::vector<double> shift;         // [nb] the alpha that worked (0: none needed; -1: the block fell back)
    // ---- the device side (ehyb_bic.hip)
    bool uploaded = false;
    int threads = 0;
    int64_t stream_bytes = 0, stream_entries = 0;
    ehyb::BicBlock* d_blocks = nullptr;
    int32_t* d_order = nullptr;
    int32_t* d_perm = nullptr;
    uint32_t* d_rounds = nullptr;
    uint32_t* d_cnt = nullptr;
    uint32_t* d_meta = nullptr;
    double* d_dinv = nullptr;
    uint16_t* d_cols = nullptr;
    double* d_vals = nullptr;
};
