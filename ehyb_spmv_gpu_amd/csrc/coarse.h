// The object behind ehyb_coarse (include/ehyb.h): the aggregate coarse space of the two-level preconditioner.  coarse.cpp
// builds the host side (no GPU needed), ehyb_coarse.hip uploads it, applies it and releases it.
#pragma once
#include <cstdint>
#include <vector>

struct ehyb_coarse {
    int n = 0;   // rows of the matrix
    int nc = 0;  // coarse unknowns
    int ld = 0;  // doubles per row of d_einv: nc rounded up to even, so that every row starts on 16 bytes
    std::vector<int32_t> map;      // [n] coarse unknown of every row
    std::vector<int32_t> row_ptr;  // [nc + 1]
    std::vector<int32_t> rows;     // [n] the transpose of map, rows rising inside an unknown
    std::vector<double> E;         // [nc * nc] P^T A P (empty: ehyb_coarse_create_raw)
    std::vector<double> Einv;      // [nc * nc]
    // A vector object (ehyb_coarse_create_host_vecs, _raw_vecs; nv > 0): map, row_ptr and rows describe the nagg aggregates,
    // aggregate a owns the unknowns off[a] .. off[a + 1), one per kept column of its local basis.  A plain object: nv = 0, empty.
    int nv = 0;                    // columns handed in
    int nagg = 0;                  // aggregates
    std::vector<int32_t> off;      // [nagg + 1], off[nagg] = nc
    std::vector<double> W;         // [nv * n] column j of the local bases at W + j n, zero where an aggregate kept fewer
    bool uploaded = false;
    int32_t* d_map = nullptr;
    int32_t* d_row_ptr = nullptr;
    int32_t* d_rows = nullptr;
    int32_t* d_off = nullptr;     // vector object only
    double* d_w = nullptr;        // vector object only: [nv * n]
    double* d_einv = nullptr;   // [nc * ld], the pad column zero
    double* d_scratch = nullptr;  // [2 * nc] T and C of ehyb_coarse_apply: one apply at a time per object
};

namespace ehyb {
// rows of every group (unknown; aggregate of a vector object) from the map, `groups` of them (counting sort: rising inside a
// group); false: an entry out of range or an empty group
bool coarse_transpose(ehyb_coarse* c, int groups, int* bad_row, int* empty_unknown);
}  // namespace ehyb
