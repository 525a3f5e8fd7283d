// The neighbour list across two effects (hnb_effect_pairs_from; include/hanabi_amd_pairs_from.h), shared by the kernels' translation unit
// (hnb_pairs_from.hip: a code object of its own) and the runtime that loads and launches them (hanabi_amd.hip): over the pair rule and the walk of
// hnb_neighbours.h - neighbour_d2, neighbour_range, neighbour_candidates, neighbour_cell_xyz -, the snapshot record, the clamp and the tiles of
// hnb_pairs.h and the two sides of hnb_neighbours_from.h: the two per-query bodies both kernels call (pairs_from_row_count, pairs_from_row_fill),
// the kernels' argument block, the kernels by name (PairsFromKernel), the check of a description against BOTH effects (pairs_from_check_desc), the
// scratch layout and the launches of a call (pairs_from_launch_plan). Plain C++: a host compiler takes it, so the tests drive whole states through
// the kernels' own row bodies and check the refusals, the layout and the plan without a GPU. Nothing may be contracted into a fused multiply-add
// (the pragma for clang / hipcc; a host compiler builds this with -ffp-contract=off).
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd_pairs_from.h"
#include "hnb_neighbours.h"
#include "hnb_neighbours_from.h"
#include "hnb_pairs.h"

namespace hnb {

constexpr uint32_t kPairsFromBlock = 256;           // lanes per workgroup: one sorted query row per lane; a tile is the rows of one workgroup
constexpr uint32_t kPairsFromStatsWords = 8;
static_assert(kPairsFromBlock == kPairsBlock, "the borrowed k_pairs_scan and pairs_tiles count tiles of kPairsBlock rows");

// ---- the per-query bodies -------------------------------------------------------------------------------------------------------------------------
// A query INSIDE the grid, in cell `cell` (< n_cells), at (xi, yi, zi). The nine ranges are formed in the SOURCE's cell_start; their lengths give
// candidates(i) before any pair is tested: crowded -> lists nothing. Otherwise the length of its run: the source rows j of the nine ranges with
// d2 < r2 - every one: the rows are another effect's, so no row is the query itself and no slot order means anything. At most candidate_limit rounds
// over all nine ranges together. Snapshot rows read are below cell_start[n_cells]; table entries read are at most n_cells.
struct PairsFromRowCount { uint32_t count, crowded; };
HNB_SORT_KEY_FN PairsFromRowCount pairs_from_row_count(const PairsSnap* snap, const uint32_t* cell_start, const uint32_t* dims, uint32_t cell, float xi, float yi, float zi,
                                                       uint32_t candidate_limit, float r2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    PairsFromRowCount out = {0u, 0u};
    const NeighbourCell c = neighbour_cell_xyz(dims, cell);
    if (neighbour_candidates(cell_start, dims, c) > candidate_limit) { out.crowded = 1u; return out; }
    for (uint32_t i = 0; i < 9u; ++i) {
        const NeighbourRange rg = neighbour_range(cell_start, dims, c, i);
        for (uint32_t j = rg.lo; j < rg.hi; ++j) {
            const PairsSnap o = snap[j];
            const float d2 = neighbour_d2(xi, yi, zi, neighbour_f32(o.x), neighbour_f32(o.y), neighbour_f32(o.z));
            if (d2 < r2) ++out.count;
        }
    }
    return out;
}

// The same walk of a query that is not crowded, storing: neighbour k of the run - a SOURCE slot - goes to index base + k of out_pairs (and its d2
// to out_d2 when given) while that index is below pair_capacity - every index stored to is below pair_capacity. -> the run's length (what
// pairs_from_row_count gave).
HNB_SORT_KEY_FN uint32_t pairs_from_row_fill(const PairsSnap* snap, const uint32_t* cell_start, const uint32_t* dims, uint32_t cell, float xi, float yi, float zi, float r2,
                                             uint64_t base, uint32_t pair_capacity, uint32_t* out_pairs, float* out_d2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const NeighbourCell c = neighbour_cell_xyz(dims, cell);
    uint32_t k = 0;
    for (uint32_t i = 0; i < 9u; ++i) {
        const NeighbourRange rg = neighbour_range(cell_start, dims, c, i);
        for (uint32_t j = rg.lo; j < rg.hi; ++j) {
            const PairsSnap o = snap[j];
            const float d2 = neighbour_d2(xi, yi, zi, neighbour_f32(o.x), neighbour_f32(o.y), neighbour_f32(o.z));
            if (!(d2 < r2)) continue;
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

// ---- the kernels' argument block ------------------------------------------------------------------------------------------------------------------
struct PairsFromArgs {
    const uint64_t* q_slab;         // [1] fx's slab base address
    const HnbDeviceMeta* q_meta;    // [1] fx's row after the frames enqueued so far
    const uint32_t* q_keys;         // fx's sort: [2][q_pitch] cells and
    const uint32_t* q_vals;         //   slots, ping-pong: the state words say which half holds the order
    const ExportSortState* q_state;
    const PairsSnap* snap;          // [s_pitch]: (x, y, z, slot) of sorted SOURCE row j (k_neighbours_pack's)
    const uint32_t* cell_start;     // [n_cells + 2]: the SOURCE's table
    uint32_t* count;                // [q_pitch]: the run length of query row r
    uint64_t* tile;                 // [tiles + 1]: as PairsArgs::tile - k_pairs_scan works on it
    uint32_t* out_rows;             // [q_capacity]
    uint32_t* out_start;            // [q_capacity + 1]
    uint32_t* out_pairs;            // [pair_capacity] (NULL iff pair_capacity == 0)
    float* out_d2;                  // [pair_capacity] or NULL
    uint32_t* stats;                // [8] or NULL
    uint64_t q_pos_off;             // bytes from fx's slab base: POSITION, 12 bytes per slot
    BinGrid grid;
    uint32_t q_capacity, q_pitch, tiles, candidate_limit, pair_capacity;
    float r2;
};
static_assert(sizeof(PairsFromArgs) == 184, "one PairsFromArgs by value");

// ---- the check of a description -------------------------------------------------------------------------------------------------------------------
// In front: the two effects. Then pairs_check_desc's refusals in its order up to the crowding limit, with this call's flags rule. Then POSITION and
// the capacity of either side, fx first. Behind: pairs_check_desc's refusals of the destinations, sized from FX's capacity.
enum PairsFromDescError : uint32_t {
    kPairsFromOk, kPairsFromErrSameEffect, kPairsFromErrContexts, kPairsFromErrStructSize, kPairsFromErrHalf, kPairsFromErrFlags, kPairsFromErrDims, kPairsFromErrOrigin,
    kPairsFromErrInvCell, kPairsFromErrRadius, kPairsFromErrCoverage, kPairsFromErrRadiusSquared, kPairsFromErrCandidateLimit, kPairsFromErrNoPosition, kPairsFromErrSourceNoPosition,
    kPairsFromErrCapacity, kPairsFromErrSourceCapacity, kPairsFromErrNullRows, kPairsFromErrNullStart, kPairsFromErrNullPairs, kPairsFromErrAlign, kPairsFromErrStats,
    kPairsFromErrOverlap, kPairsFromDescErrorCount
};
HNB_SORT_KEY_FN const char* pairs_from_error_text(uint32_t e) {
    switch (e) {
        case kPairsFromOk: return "ok";
        case kPairsFromErrSameEffect: return "fx and source are one effect: the list within one effect is hnb_effect_pairs'";
        case kPairsFromErrContexts: return neighbours_from_error_text(kNbFromErrContexts);
        case kPairsFromErrStructSize: return pairs_error_text(kPairsErrStructSize);
        case kPairsFromErrHalf: return "flags: HNB_PAIRS_HALF orders the slots of ONE effect; a slot order across two effects means nothing";
        case kPairsFromErrFlags: return "flags must be 0";
        case kPairsFromErrDims: return pairs_error_text(kPairsErrDims);
        case kPairsFromErrOrigin: return pairs_error_text(kPairsErrOrigin);
        case kPairsFromErrInvCell: return pairs_error_text(kPairsErrInvCell);
        case kPairsFromErrRadius: return pairs_error_text(kPairsErrRadius);
        case kPairsFromErrCoverage: return pairs_error_text(kPairsErrCoverage);
        case kPairsFromErrRadiusSquared: return pairs_error_text(kPairsErrRadiusSquared);
        case kPairsFromErrCandidateLimit: return pairs_error_text(kPairsErrCandidateLimit);
        case kPairsFromErrNoPosition: return neighbours_from_error_text(kNbFromErrNoPosition);
        case kPairsFromErrSourceNoPosition: return neighbours_from_error_text(kNbFromErrSourceNoPosition);
        case kPairsFromErrCapacity: return neighbours_from_error_text(kNbFromErrCapacity);
        case kPairsFromErrSourceCapacity: return neighbours_from_error_text(kNbFromErrSourceCapacity);
        case kPairsFromErrNullRows: return pairs_error_text(kPairsErrNullRows);
        case kPairsFromErrNullStart: return pairs_error_text(kPairsErrNullStart);
        case kPairsFromErrNullPairs: return pairs_error_text(kPairsErrNullPairs);
        case kPairsFromErrAlign: return pairs_error_text(kPairsErrAlign);
        case kPairsFromErrStats: return pairs_error_text(kPairsErrStats);
        case kPairsFromErrOverlap: return pairs_error_text(kPairsErrOverlap);
        default: return "?";
    }
}
// The destinations of a call as byte ranges, in pairs_destinations' order; out_rows and out_start are sized from FX's capacity
HNB_SORT_KEY_FN void pairs_from_destinations(const HnbPairsDesc& d, uint32_t q_capacity, PairsRange* out) { pairs_destinations(d, q_capacity, out); }
struct PairsFromCheck {
    uint32_t error, index;          // a PairsFromDescError and, for an axis's or a destination's, its index (an overlap: the later of the two)
    uint32_t n_cells;
    uint32_t q_position_index, s_position_index;   // the entries of POSITION in fx's and in the source's layout
    float r2;                       // radius * radius in f32
};
// The refusals of include/hanabi_amd_pairs_from.h "Errors" but the NULL arguments, in the order listed there
HNB_SORT_KEY_FN PairsFromCheck pairs_from_check_desc(const HnbPairsDesc& d, const NeighboursFromSide& fx, const NeighboursFromSide& source, bool same_effect, bool same_context) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    PairsFromCheck c = {};
    const auto fail = [&c](uint32_t e, uint32_t k) { c.error = e; c.index = k; return c; };
    if (same_effect) return fail(kPairsFromErrSameEffect, 0);
    if (!same_context) return fail(kPairsFromErrContexts, 0);
    if (d.struct_size != sizeof(HnbPairsDesc)) return fail(kPairsFromErrStructSize, 0);
    if ((d.flags & HNB_PAIRS_HALF) != 0u) return fail(kPairsFromErrHalf, 0);
    if (d.flags != 0u) return fail(kPairsFromErrFlags, 0);
    c.n_cells = bin_cell_count(d.dims);
    if (c.n_cells == 0u) return fail(kPairsFromErrDims, 0);
    for (uint32_t a = 0; a < 3u; ++a) {
        if (!neighbour_is_finite(d.origin[a])) return fail(kPairsFromErrOrigin, a);
        if (!neighbour_is_finite(d.inv_cell[a]) || !(d.inv_cell[a] > 0.0f)) return fail(kPairsFromErrInvCell, a);
    }
    if (!neighbour_is_finite(d.radius) || !(d.radius > 0.0f)) return fail(kPairsFromErrRadius, 0);
    for (uint32_t a = 0; a < 3u; ++a)
        if (!((double)d.radius * (double)d.inv_cell[a] <= 1.0)) return fail(kPairsFromErrCoverage, a);
    c.r2 = d.radius * d.radius;
    const float inv_r2 = 1.0f / c.r2;
    if (!neighbour_is_finite(c.r2) || !neighbour_is_finite(inv_r2) || !(c.r2 >= 1.17549435e-38f)) return fail(kPairsFromErrRadiusSquared, 0);
    if (d.candidate_limit == 0u || d.candidate_limit > HNB_NEIGHBOUR_MAX_CANDIDATES) return fail(kPairsFromErrCandidateLimit, 0);
    const NeighboursFromSide* side[2] = {&fx, &source};
    for (uint32_t s = 0; s < 2u; ++s) {
        const uint32_t p = neighbours_from_find(*side[s], HNB_ATTR_POSITION);
        if (p == side[s]->n_layout || !side[s]->layout[p].is_f32 || side[s]->layout[p].ncomp != 3u) return fail(s ? kPairsFromErrSourceNoPosition : kPairsFromErrNoPosition, 0);
        (s ? c.s_position_index : c.q_position_index) = p;
    }
    for (uint32_t s = 0; s < 2u; ++s)
        if (export_sort_scratch_layout(1u, side[s]->capacity, HNB_SORT_SCOPE_INSTANCE).rows == 0u) return fail(s ? kPairsFromErrSourceCapacity : kPairsFromErrCapacity, 0);
    if (d.out_rows == nullptr) return fail(kPairsFromErrNullRows, 0);
    if (d.out_start == nullptr) return fail(kPairsFromErrNullStart, 1);
    if (d.out_pairs == nullptr && d.pair_capacity > 0u) return fail(kPairsFromErrNullPairs, 2);
    PairsRange dst[kPairsDestinations];
    pairs_from_destinations(d, fx.capacity, dst);
    for (uint32_t i = 0; i < 4u; ++i)
        if ((dst[i].lo & 3u) != 0u) return fail(kPairsFromErrAlign, i);
    if ((dst[4].lo & 15u) != 0u) return fail(kPairsFromErrStats, 4);
    for (uint32_t i = 1; i < kPairsDestinations; ++i)
        for (uint32_t e = 0; e < i; ++e)
            if (dst[i].bytes != 0u && dst[e].bytes != 0u && dst[i].lo < dst[e].lo + dst[e].bytes && dst[e].lo < dst[i].lo + dst[i].bytes) return fail(kPairsFromErrOverlap, i);
    return c;
}

// ---- the scratch ----------------------------------------------------------------------------------------------------------------------------------
// One allocation, owned by fx and apart from its d_neighbours, d_pairs and d_neighbours_from; every section starts on a 256-byte boundary: the
// sorted export's layout of one instance for the SOURCE's capacity (the cells as keys, the slots as values, the digit tables), the same for FX's
// capacity, then the snapshot - 16 bytes per row of the source sort's pitch -, then 4 bytes per row of fx's pitch for the run lengths, then 8 bytes
// per tile of kPairsFromBlock query rows and 8 more for the total, then the source's cell_start table of n_cells + 2 words. s_sort.rows == 0 or
// q_sort.rows == 0: more than 0xFFFFFF00 slots (refused).
struct PairsFromScratch {
    ExportSortScratch s_sort, q_sort;
    uint32_t tiles;
    uint64_t q_sort_off, snap_off, snap_bytes, count_off, count_bytes, tile_off, tile_bytes, cells_off, cells_bytes, total;
};
HNB_SORT_KEY_FN PairsFromScratch pairs_from_scratch_layout(uint32_t q_capacity, uint32_t s_capacity, uint32_t n_cells) {
    PairsFromScratch l = {};
    const uint64_t align = 255u;
    l.s_sort = export_sort_scratch_layout(1u, s_capacity, HNB_SORT_SCOPE_INSTANCE);
    l.q_sort = export_sort_scratch_layout(1u, q_capacity, HNB_SORT_SCOPE_INSTANCE);
    l.tiles = pairs_tiles(q_capacity);
    l.q_sort_off = (l.s_sort.total + align) & ~align;
    l.snap_off = (l.q_sort_off + l.q_sort.total + align) & ~align;
    l.snap_bytes = (uint64_t)l.s_sort.pitch * 16u;
    l.count_off = (l.snap_off + l.snap_bytes + align) & ~align;
    l.count_bytes = (uint64_t)l.q_sort.pitch * 4u;
    l.tile_off = (l.count_off + l.count_bytes + align) & ~align;
    l.tile_bytes = ((uint64_t)l.tiles + 1u) * 8u;
    l.cells_off = (l.tile_off + l.tile_bytes + align) & ~align;
    l.cells_bytes = (uint64_t)export_bin_entries(n_cells) * 4u;
    l.total = (l.cells_off + l.cells_bytes + align) & ~align;
    return l;
}

// ---- the launches of a call -----------------------------------------------------------------------------------------------------------------------
// The kernels of hnb_pairs_from.hip: the index of a kernel's handle in the context. Numbered apart from every other unit's. (The scan between them
// is hnb_pairs.hip's k_pairs_scan, borrowed: kPairsKScan of that unit's table.)
enum PairsFromKernel : uint32_t { kPairsFromKCount, kPairsFromKFill, kPairsFromKernelCount };
struct PairsFromKernelName { uint32_t kernel; const char* name; };
constexpr PairsFromKernelName kPairsFromKernelNames[kPairsFromKernelCount] = {{kPairsFromKCount, "k_pairs_from_count"}, {kPairsFromKFill, "k_pairs_from_fill"}};

struct PairsFromPlan {
    ExportPlan source_sort;         // the binned export's launches but its gather: (one workgroup | memset + keys + the sort's passes) + the table
    ExportPlan query_sort;          //   ... and but the table as well: the queries' order alone, into the second sort section (zero_off is within it)
    uint32_t pack_grid;             // k_neighbours_pack bound to the source: a lane per row of the source's capacity
    uint32_t count_grid;            // k_pairs_from_count: a workgroup per tile of fx's capacity
    uint32_t scan_grid;             // k_pairs_scan: 1
    uint32_t fill_grid;             // k_pairs_from_fill: q_capacity + 1 lanes - the table has one entry more than there are rows
    uint64_t clear_stats_bytes;     // what the call zeroes in front when out_stats is given
};
// Both capacities must fit a sort (pairs_from_check_desc). Decides; hanabi_amd.hip run_pairs_from executes: the sorts through run_export_plan, each
// with the base of its own section.
HNB_SORT_KEY_FN PairsFromPlan pairs_from_launch_plan(uint32_t q_capacity, uint32_t s_capacity, uint32_t n_cells) {
    PairsFromPlan pl = {};
    pl.source_sort = export_bin_launch_plan(s_capacity, 16u, n_cells);
    pl.source_sort.n -= 1u;         // (the last launch is the binned export's gather of records: there are none here)
    pl.query_sort = export_bin_launch_plan(q_capacity, 16u, n_cells);
    pl.query_sort.n -= 2u;          // (... and the one in front of it the table: the queries are looked up in the source's)
    pl.pack_grid = pairs_tiles(s_capacity);
    pl.count_grid = pairs_tiles(q_capacity);
    pl.scan_grid = 1u;
    pl.fill_grid = (uint32_t)(((uint64_t)q_capacity + 1u + kPairsFromBlock - 1u) / kPairsFromBlock);   // <= tiles + 1
    pl.clear_stats_bytes = kPairsFromStatsWords * 4u;
    return pl;
}

}  // namespace hnb
