// The cell of a particle in the uniform grid of hnb_effect_export_binned (include/hanabi_amd_binned.h): plain C++ that a host
// compiler and hipcc both take, so that the host-side tests state the cells with the function the kernels call. Every f32 operation is a statement
// of its own, in the order the header writes it; nothing may be contracted into a fused multiply-add (the pragma for clang / hipcc; a host compiler
// builds this with -ffp-contract=off). A comparison with a NaN is false: the particle is outside.
#pragma once
#include <stdint.h>

#include "hnb_sort_key.h"

namespace hnb {

constexpr uint32_t kBinMaxCells = 1u << 24;   // HNB_BIN_MAX_CELLS: every dims[c] is at most this, so (float)dims[c] is exact

struct BinGrid {
    uint32_t dims[3];       // cells along x, y, z: each >= 1
    uint32_t n_cells;       // their product, <= kBinMaxCells: the key of the outside bin
    float origin[3];        // the grid's lowest corner
    float inv_cell[3];      // 1 / cell edge per axis
};

// dims -> their product in 64 bits; 0: a dimension is 0 or the product is above kBinMaxCells (the grid is refused)
HNB_SORT_KEY_FN uint32_t bin_cell_count(const uint32_t* dims) {
    uint64_t n = 1;
    for (int c = 0; c < 3; ++c) {
        if (dims[c] == 0u) return 0u;
        n *= dims[c];                                       // (at most 2^24 times a 32-bit factor: below 2^56)
        if (n > kBinMaxCells) return 0u;
    }
    return (uint32_t)n;
}

// Per axis c: t = (p[c] - origin[c]) * inv_cell[c]; inside iff t >= 0 and t < (float)dims[c] (-0 is inside, a NaN or an infinity is not);
// i[c] = (uint32_t)t, converted only behind the range test: t is then in [0, 2^24) and the conversion is exact truncation.
// cell = (i[2] * dims[1] + i[1]) * dims[0] + i[0], or n_cells - the outside bin - when an axis is not inside.
HNB_SORT_KEY_FN uint32_t bin_cell_of(const BinGrid& g, float x, float y, float z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p[3] = {x, y, z};
    uint32_t i[3] = {0u, 0u, 0u};
    bool inside = true;
    for (int c = 0; c < 3; ++c) {
        const float d = p[c] - g.origin[c];
        const float t = d * g.inv_cell[c];
        const bool in = t >= 0.0f && t < (float)g.dims[c];
        i[c] = in ? (uint32_t)t : 0u;
        inside = inside && in;
    }
    return inside ? (i[2] * g.dims[1] + i[1]) * g.dims[0] + i[0] : g.n_cells;
}

}  // namespace hnb
