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
    bool uploaded = false;
    int32_t* d_map = nullptr;
    int32_t* d_row_ptr = nullptr;
    int32_t* d_rows = nullptr;
    double* d_einv = nullptr;   // [nc * ld], the pad column zero
    double* d_scratch = nullptr;  // [2 * nc] T and C of ehyb_coarse_apply: one apply at a time per object
};

namespace ehyb {
// rows of every unknown from the map (counting sort: rising inside an unknown); false: an entry out of range or an empty unknown
bool coarse_transpose(ehyb_coarse* c, int* bad_row, int* empty_unknown);
}  // namespace ehyb
