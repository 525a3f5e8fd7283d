// The neighbour list (hnb_effect_pairs; include/hanabi_amd_pairs.h), shared by the kernels' translation unit (hnb_pairs.hip: a code object of its
// own) and the runtime that loads and launches them (hanabi_amd.hip): over the pair rule and the walk of hnb_neighbours.h - neighbour_d2,
// neighbour_range, neighbour_candidates, neighbour_cell_xyz - the two per-row bodies both kernels call (pairs_row_count, pairs_row_fill), the clamp
// of an offset, the kernels' argument block, the kernels by name (PairsKernel), the check of a description (pairs_check_desc), the scratch layout
// and the launches of a call (pairs_launch_plan). Plain C++: a host compiler takes it, so the tests drive whole states through the kernels' own
// row bodies and check the refusals, the layout and the plan without a GPU. Nothing may be contracted into a fused multiply-add (the pragma for
// clang / hipcc; a host compiler builds this with -ffp-contract=off).
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd_pairs.h"
#include "hnb_neighbours.h"

namespace hnb {

constexpr uint32_t kPairsBlock = 256;               // lanes per workgroup: one sorted row per lane; a tile is the rows of one workgroup
constexpr uint32_t kPairsStatsWords = 8;

// A record of the snapshot k_neighbours_pack writes: the position's bits and the slot of sorted row r, 16 bytes, read as one
struct alignas(16) PairsSnap { uint32_t x, y, z, slot; };
static_assert(sizeof(PairsSnap) == 16, "one 16-byte record per row");

// ---- the per-row bodies ---------------------------------------------------------------------------------------------------------------------------
// Sorted inside row r in cell `cell`: crowded -> lists nothing. Otherwise the length of its run: the candidates j != r of the nine ranges with
// d2 < r2 and, under HNB_PAIRS_HALF, slot_j > slot_r. At most candidate_limit rounds over all nine ranges together.
struct PairsRowCount { uint32_t count, crowded; };
HNB_SORT_KEY_FN PairsRowCount pairs_row_count(const PairsSnap* snap, const uint32_t* cell_start, const uint32_t* dims, uint32_t r, uint32_t cell, uint32_t candidate_limit, float r2,
                                              bool half) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    PairsRowCount out = {0u, 0u};
    const NeighbourCell c = neighbour_cell_xyz(dims, cell);
    if (neighbour_candidates(cell_start, dims, c) > candidate_limit) { out.crowded = 1u; return out; }
    const PairsSnap own = snap[r];
    const float xi = neighbour_f32(own.x), yi = neighbour_f32(own.y), zi = neighbour_f32(own.z);
    for (uint32_t i = 0; i < 9u; ++i) {
        const NeighbourRange rg = neighbour_range(cell_start, dims, c, i);
        for (uint32_t j = rg.lo; j < rg.hi; ++j) {
            if (j == r) continue;                                         // the particle itself; a coincident one is another row
            const PairsSnap o = snap[j];
            const float d2 = neighbour_d2(xi, yi, zi, neighbour_f32(o.x), neighbour_f32(o.y), neighbour_f32(o.z));
            if (!(d2 < r2)) continue;
            if (half && !(o.slot > own.slot)) continue;
            ++out.count;
        }
    }
    return out;
}

// The same walk of a row that is not crowded, storing: neighbour k of the run goes to index base + k of out_pairs (and its d2 to out_d2 when given)
// while that index is below pair_capacity - every index stored to is below pair_capacity. -> the run's length (what pairs_row_count gave).
HNB_SORT_KEY_FN uint32_t pairs_row_fill(const PairsSnap* snap, const uint32_t* cell_start, const uint32_t* dims, uint32_t r, uint32_t cell, float r2, bool half, uint64_t base,
                                        uint32_t pair_capacity, uint32_t* out_pairs, float* out_d2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const NeighbourCell c = neighbour_cell_xyz(dims, cell);
    const PairsSnap own = snap[r];
    const float xi = neighbour_f32(own.x), yi = neighbour_f32(own.y), zi = neighbour_f32(own.z);
    uint32_t k = 0;
    for (uint32_t i = 0; i < 9u; ++i) {
        const NeighbourRange rg = neighbour_range(cell_start, dims, c, i);
        for (uint32_t j = rg.lo; j < rg.hi; ++j) {
            if (j == r) continue;
            const PairsSnap o = snap[j];
            const float d2 = neighbour_d2(xi, yi, zi, neighbour_f32(o.x), neighbour_f32(o.y), neighbour_f32(o.z));
            if (!(d2 < r2)) continue;
            if (half && !(o.slot > own.slot)) continue;
            const uint64_t g = base + k;
            if (g < (uint64_t)pair_capacity) {
                out_pairs[g] = o.slot;
                if (out_d2) out_d2[g] = d2;
            }
            ++k;
        }
    }
    return k;
}

// out_start[r] of T[r], and the pairs written of the true total
HNB_SORT_KEY_FN uint32_t pairs_clamp(uint64_t T, uint32_t pair_capacity) { return T < (uint64_t)pair_capacity ? (uint32_t)T : pair_capacity; }

// ---- the kernels' argument block ------------------------------------------------------------------------------------------------------------------
struct PairsArgs {
    const HnbDeviceMeta* meta;      // [1] the instance's row after the frames enqueued so far
    const uint32_t* keys;           // the sort's [2][pitch] cells, ping-pong: the state words say which half holds the order
    const ExportSortState* state;
    const PairsSnap* snap;          // [pitch]: (x, y, z, slot) of sorted row r (k_neighbours_pack's)
    const uint32_t* cell_start;     // [n_cells + 2]
    uint32_t* count;                // [pitch]: the run length of row r
    uint64_t* tile;                 // [tiles + 1]: the tile's run lengths summed; after the scan the sum of the tiles in front, and the total at [tiles]
    uint32_t* out_rows;             // [capacity]
    uint32_t* out_start;            // [capacity + 1]
    uint32_t* out_pairs;            // [pair_capacity] (NULL iff pair_capacity == 0)
    float* out_d2;                  // [pair_capacity] or NULL
    uint32_t* stats;                // [8] or NULL
    BinGrid grid;
    uint32_t capacity, pitch, tiles, candidate_limit, pair_capacity, half;
    float r2;
    uint32_t reserved;
};
static_assert(sizeof(HnbPairsDesc) == 96, "HnbPairsDesc layout");
static_assert(sizeof(PairsArgs) == 168, "one PairsArgs by value");

// ---- the check of a description -------------------------------------------------------------------------------------------------------------------
enum PairsDescError : uint32_t {
    kPairsOk, kPairsErrStructSize, kPairsErrFlags, kPairsErrDims, kPairsErrOrigin, kPairsErrInvCell, kPairsErrRadius, kPairsErrCoverage, kPairsErrRadiusSquared,
    kPairsErrCandidateLimit, kPairsErrNoPosition, kPairsErrCapacity, kPairsErrNullRows, kPairsErrNullStart, kPairsErrNullPairs, kPairsErrAlign, kPairsErrStats, kPairsErrOverlap,
    kPairsDescErrorCount
};
HNB_SORT_KEY_FN const char* pairs_error_text(uint32_t e) {
    switch (e) {
        case kPairsOk: return "ok";
        case kPairsErrStructSize: return "struct_size is not this library's sizeof(HnbPairsDesc)";
        case kPairsErrFlags: return "flags: 0 or HNB_PAIRS_HALF";
        case kPairsErrDims: return neighbour_error_text(kNeighbourErrDims);
        case kPairsErrOrigin: return neighbour_error_text(kNeighbourErrOrigin);
        case kPairsErrInvCell: return neighbour_error_text(kNeighbourErrInvCell);
        case kPairsErrRadius: return neighbour_error_text(kNeighbourErrRadius);
        case kPairsErrCoverage: return neighbour_error_text(kNeighbourErrCoverage);
        case kPairsErrRadiusSquared: return neighbour_error_text(kNeighbourErrRadiusSquared);
        case kPairsErrCandidateLimit: return neighbour_error_text(kNeighbourErrCandidateLimit);
        case kPairsErrNoPosition: return neighbour_error_text(kNeighbourErrNoPosition);
        case kPairsErrCapacity: return neighbour_error_text(kNeighbourErrCapacity);
        case kPairsErrNullRows: return "out_rows is NULL";
        case kPairsErrNullStart: return "out_start is NULL";
        case kPairsErrNullPairs: return "out_pairs is NULL with pair_capacity above 0";
        case kPairsErrAlign: return "out_rows, out_start, out_pairs or out_d2 is not 4-byte aligned";
        case kPairsErrStats: return "out_stats: NULL or a 16-byte aligned device pointer";
        case kPairsErrOverlap: return "two destination ranges overlap";
        default: return "?";
    }
}
// The destinations of a call as byte ranges, in the order out_rows, out_start, out_pairs, out_d2, out_stats; bytes == 0: not written
struct PairsRange { uint64_t lo, bytes; };
constexpr uint32_t kPairsDestinations = 5;
HNB_SORT_KEY_FN void pairs_destinations(const HnbPairsDesc& d, uint32_t capacity, PairsRange* out) {
    out[0] = {(uint64_t)(uintptr_t)d.out_rows, (uint64_t)capacity * 4u};
    out[1] = {(uint64_t)(uintptr_t)d.out_start, ((uint64_t)capacity + 1u) * 4u};
    out[2] = {(uint64_t)(uintptr_t)d.out_pairs, d.out_pairs ? (uint64_t)d.pair_capacity * 4u : 0u};
    out[3] = {(uint64_t)(uintptr_t)d.out_d2, d.out_d2 ? (uint64_t)d.pair_capacity * 4u : 0u};
    out[4] = {(uint64_t)(uintptr_t)d.out_stats, d.out_stats ? (uint64_t)kPairsStatsWords * 4u : 0u};
}
struct PairsCheck {
    uint32_t error, index;          // a PairsDescError and, for an axis's or a destination's, its index (an overlap: the later of the two)
    uint32_t n_cells;
    uint32_t position_index;        // the layout's entry of POSITION
    float r2;                       // radius * radius in f32
};
// The refusals of include/hanabi_amd_pairs.h "Errors" but the NULL arguments, in the order listed there
HNB_SORT_KEY_FN PairsCheck pairs_check_desc(const HnbPairsDesc& d, const NeighbourLayoutAttr* layout, uint32_t n_layout, uint32_t capacity) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    PairsCheck c = {};
    const auto fail = [&c](uint32_t e, uint32_t k) { c.error = e; c.index = k; return c; };
    if (d.struct_size != sizeof(HnbPairsDesc)) return fail(kPairsErrStructSize, 0);
    if ((d.flags & ~HNB_PAIRS_HALF) != 0u) return fail(kPairsErrFlags, 0);
    c.n_cells = bin_cell_count(d.dims);
    if (c.n_cells == 0u) return fail(kPairsErrDims, 0);
    for (uint32_t a = 0; a < 3u; ++a) {
        if (!neighbour_is_finite(d.origin[a])) return fail(kPairsErrOrigin, a);
        if (!neighbour_is_finite(d.inv_cell[a]) || !(d.inv_cell[a] > 0.0f)) return fail(kPairsErrInvCell, a);
    }
    if (!neighbour_is_finite(d.radius) || !(d.radius > 0.0f)) return fail(kPairsErrRadius, 0);
    for (uint32_t a = 0; a < 3u; ++a)
        if (!((double)d.radius * (double)d.inv_cell[a] <= 1.0)) return fail(kPairsErrCoverage, a);
    c.r2 = d.radius * d.radius;
    const float inv_r2 = 1.0f / c.r2;
    if (!neighbour_is_finite(c.r2) || !neighbour_is_finite(inv_r2) || !(c.r2 >= 1.17549435e-38f)) return fail(kPairsErrRadiusSquared, 0);
    if (d.candidate_limit == 0u || d.candidate_limit > HNB_NEIGHBOUR_MAX_CANDIDATES) return fail(kPairsErrCandidateLimit, 0);
    uint32_t p = 0;
    while (p < n_layout && layout[p].attr != HNB_ATTR_POSITION) ++p;
    if (p == n_layout || !layout[p].is_f32 || layout[p].ncomp != 3u) return fail(kPairsErrNoPosition, 0);
    c.position_index = p;
    if (export_sort_scratch_layout(1u, capacity, HNB_SORT_SCOPE_INSTANCE).rows == 0u) return fail(kPairsErrCapacity, 0);
    if (d.out_rows == nullptr) return fail(kPairsErrNullRows, 0);
    if (d.out_start == nullptr) return fail(kPairsErrNullStart, 1);
    if (d.out_pairs == nullptr && d.pair_capacity > 0u) return fail(kPairsErrNullPairs, 2);
    PairsRange dst[kPairsDestinations];
    pairs_destinations(d, capacity, dst);
    for (uint32_t i = 0; i < 4u; ++i)
        if ((dst[i].lo & 3u) != 0u) return fail(kPairsErrAlign, i);
    if ((dst[4].lo & 15u) != 0u) return fail(kPairsErrStats, 4);
    for (uint32_t i = 1; i < kPairsDestinations; ++i)
        for (uint32_t e = 0; e < i; ++e)
            if (dst[i].bytes != 0u && dst[e].bytes != 0u && dst[i].lo < dst[e].lo + dst[e].bytes && dst[e].lo < dst[i].lo + dst[i].bytes) return fail(kPairsErrOverlap, i);
    return c;
}

// ---- the scratch ----------------------------------------------------------------------------------------------------------------------------------
// One allocation per effect; every section starts on a 256-byte boundary: the sorted export's layout of one instance (the cells as keys, the slots
// as values, the digit tables), then the snapshot - 16 bytes per row of the sort's pitch -, then 4 bytes per row for the run lengths, then 8 bytes
// per tile of kPairsBlock rows and 8 more for the total, then the cell_start table of n_cells + 2 words. sort.rows == 0: more than 0xFFFFFF00
// slots (refused).
HNB_SORT_KEY_FN uint32_t pairs_tiles(uint32_t capacity) {
    const uint32_t t = (uint32_t)(((uint64_t)capacity + kPairsBlock - 1u) / kPairsBlock);
    return t ? t : 1u;
}
struct PairsScratch { ExportSortScratch sort; uint32_t tiles; uint64_t snap_off, snap_bytes, count_off, count_bytes, tile_off, tile_bytes, cells_off, cells_bytes, total; };
HNB_SORT_KEY_FN PairsScratch pairs_scratch_layout(uint32_t capacity, uint32_t n_cells) {
    PairsScratch l = {};
    const uint64_t align = 255u;
    l.sort = export_sort_scratch_layout(1u, capacity, HNB_SORT_SCOPE_INSTANCE);
    l.tiles = pairs_tiles(capacity);
    l.snap_off = (l.sort.total + align) & ~align;
    l.snap_bytes = (uint64_t)l.sort.pitch * 16u;
    l.count_off = (l.snap_off + l.snap_bytes + align) & ~align;
    l.count_bytes = (uint64_t)l.sort.pitch * 4u;
    l.tile_off = (l.count_off + l.count_bytes + align) & ~align;
    l.tile_bytes = ((uint64_t)l.tiles + 1u) * 8u;
    l.cells_off = (l.tile_off + l.tile_bytes + align) & ~align;
    l.cells_bytes = (uint64_t)export_bin_entries(n_cells) * 4u;
    l.total = (l.cells_off + l.cells_bytes + align) & ~align;
    return l;
}

// ---- the launches of a call -----------------------------------------------------------------------------------------------------------------------
// The kernels of hnb_pairs.hip: the index of a kernel's handle in the context. Numbered apart from every other unit's.
enum PairsKernel : uint32_t { kPairsKCount, kPairsKScan, kPairsKFill, kPairsKernelCount };
struct PairsKernelName { uint32_t kernel; const char* name; };
constexpr PairsKernelName kPairsKernelNames[kPairsKernelCount] = {{kPairsKCount, "k_pairs_count"}, {kPairsKScan, "k_pairs_scan"}, {kPairsKFill, "k_pairs_fill"}};

struct PairsPlan {
    ExportPlan sort;                // the binned export's launches but its gather: (one workgroup | memset + keys + the sort's passes) + the table
    uint32_t pack_grid;             // k_neighbours_pack: a lane per row of the capacity
    uint32_t count_grid;            // k_pairs_count: a workgroup per tile
    uint32_t scan_grid;             // k_pairs_scan: 1
    uint32_t fill_grid;             // k_pairs_fill: capacity + 1 lanes - the table has one entry more than there are rows
    uint64_t clear_stats_bytes;     // what the call zeroes in front when out_stats is given
};
// A capacity must fit a sort (pairs_check_desc). Decides; hanabi_amd.hip run_pairs executes: the sort's part through run_export_plan.
HNB_SORT_KEY_FN PairsPlan pairs_launch_plan(uint32_t capacity, uint32_t n_cells) {
    PairsPlan pl = {};
    pl.sort = export_bin_launch_plan(capacity, 16u, n_cells);
    pl.sort.n -= 1u;                // (the last launch is the binned export's gather of records: there are none here)
    pl.pack_grid = pairs_tiles(capacity);
    pl.count_grid = pairs_tiles(capacity);
    pl.scan_grid = 1u;
    pl.fill_grid = (uint32_t)(((uint64_t)capacity + 1u + kPairsBlock - 1u) / kPairsBlock);     // <= tiles + 1
    pl.clear_stats_bytes = kPairsStatsWords * 4u;
    return pl;
}

}  // namespace hnb
