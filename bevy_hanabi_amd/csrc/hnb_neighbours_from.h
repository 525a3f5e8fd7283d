// The neighbour sums across two effects (hnb_effect_neighbours_from; include/hanabi_amd_neighbours_from.h), shared by the kernel's translation unit
// (hnb_neighbours_from.hip: a code object of its own) and the runtime that loads and launches it (hanabi_amd.hip): over the pair rule, the store and
// the walk of hnb_neighbours.h - neighbour_d2, neighbour_weight, neighbour_contribution, neighbour_store, neighbour_range, neighbour_candidates,
// neighbour_cell_xyz - the per-query body the kernel calls (neighbours_from_row), the kernel's argument block, the kernel by name
// (NeighboursFromKernel), the check of a description against BOTH layouts (neighbours_from_check_desc), the scratch layout and the launches of a
// call (neighbours_from_launch_plan). Plain C++: a host compiler takes it, so the tests drive whole states through the kernel's own row body and
// check the refusals, the layout and the plan without a GPU. Nothing may be contracted into a fused multiply-add (the pragma for clang / hipcc; a
// host compiler builds this with -ffp-contract=off).
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd_neighbours_from.h"
#include "hnb_neighbours.h"

namespace hnb {

constexpr uint32_t kNeighboursFromBlock = 256;      // lanes per workgroup: one sorted query row per lane
constexpr uint32_t kNeighboursFromStatsWords = 8;

// A record of the snapshot k_neighbours_pack writes of the SOURCE: the position's bits and the slot of sorted source row j, 16 bytes, read as one
struct alignas(16) NeighboursFromSnap { uint32_t x, y, z, slot; };
static_assert(sizeof(NeighboursFromSnap) == 16, "one 16-byte record per row");

// ---- the kernel's argument block ------------------------------------------------------------------------------------------------------------------
// ch[k].src_plane_off / src_packed's ncomp and comp: the QUERY's own plane of a DIFF channel's attribute (v_i), in fx's layout - not read without
// the flag; the one / diff / frac_bits fields are the channel's. ch[k].dst_*: fx's destination. The source's stored values come from srcv.
struct NeighboursFromArgs {
    const uint64_t* q_slab;         // [1] fx's slab base address
    const HnbDeviceMeta* q_meta;    // [1] fx's row after the frames enqueued so far
    const HnbDeviceMeta* s_meta;    // [1] the source's
    const uint32_t* q_keys;         // fx's sort: [2][q_pitch] cells and
    const uint32_t* q_vals;         //   slots, ping-pong: the state words say which half holds the order
    const ExportSortState* q_state;
    const NeighboursFromSnap* snap; // [s_pitch]: (x, y, z, slot) of sorted source row j
    const uint32_t* srcv;           // [n_channels][s_pitch]: channel k's stored source of sorted source row j
    const uint32_t* cell_start;     // [n_cells + 2]: the SOURCE's table
    uint32_t* stats;                // [8] or NULL
    uint64_t q_pos_off;             // bytes from fx's slab base: POSITION, 12 bytes per slot
    BinGrid grid;
    uint32_t q_capacity, q_pitch, s_capacity, s_pitch, n_channels, weight, candidate_limit;
    float r2, inv_r2, scale;
    NeighbourChannelArg ch[HNB_NEIGHBOUR_MAX_CHANNELS];
};
static_assert(sizeof(NeighboursFromArgs) == 264, "one NeighboursFromArgs by value");

// ---- the per-query body ---------------------------------------------------------------------------------------------------------------------------
// A query INSIDE the grid, in cell `cell` (< n_cells), at (xi, yi, zi), whose own stored values of the channels are vi[k] (read for DIFF channels
// only). The nine ranges are formed in the source's cell_start; their lengths give candidates(i) before any pair is tested: crowded -> nothing is
// summed. Otherwise every source row of the ranges with d2 < r2 contributes - there is no self-exclusion: the rows are another effect's. At most
// candidate_limit rounds over all nine ranges together. Snapshot rows read are below cell_start[n_cells]; table entries read are at most n_cells.
struct NeighboursFromRow { int64_t S[HNB_NEIGHBOUR_MAX_CHANNELS]; uint32_t crowded, rejected; };
HNB_SORT_KEY_FN NeighboursFromRow neighbours_from_row(const NeighboursFromSnap* snap, const uint32_t* srcv, uint32_t s_pitch, const uint32_t* cell_start, const uint32_t* dims, uint32_t cell,
                                                      float xi, float yi, float zi, const uint32_t* vi, const NeighbourChannelArg* ch, uint32_t n_channels, uint32_t weight,
                                                      uint32_t candidate_limit, float r2, float inv_r2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    NeighboursFromRow out = {};
    const NeighbourCell c = neighbour_cell_xyz(dims, cell);
    if (neighbour_candidates(cell_start, dims, c) > candidate_limit) { out.crowded = 1u; return out; }
    for (uint32_t i = 0; i < 9u; ++i) {
        const NeighbourRange rg = neighbour_range(cell_start, dims, c, i);
        for (uint32_t j = rg.lo; j < rg.hi; ++j) {                        // (all nine together: at most candidate_limit rounds)
            const NeighboursFromSnap o = snap[j];
            const float d2 = neighbour_d2(xi, yi, zi, neighbour_f32(o.x), neighbour_f32(o.y), neighbour_f32(o.z));
            if (!(d2 < r2)) continue;
            const float W = neighbour_weight(weight, d2, inv_r2);
#if defined(__clang__)
#pragma unroll
#endif
            for (uint32_t k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
                if (k >= n_channels) break;
                const uint32_t sp = ch[k].src_packed;
                const uint32_t vj = (sp & kNeighbourSrcOne) ? kNeighbourOneBits : srcv[(size_t)k * s_pitch + j];
                const DepositQuant q = neighbour_contribution(vj, vi[k], (sp & kNeighbourSrcDiff) != 0u, weight, W, sp >> 24);
                out.S[k] = (int64_t)((uint64_t)out.S[k] + (uint64_t)q.q);  // modulo 2^64 (0 when rejected)
                out.rejected += q.ok ? 0u : 1u;
            }
        }
    }
    return out;
}

// ---- the check of a description -------------------------------------------------------------------------------------------------------------------
// neighbour_check_desc's refusals in its order, told apart by side: a channel's source is looked up in the SOURCE's layout, its destination - and the
// attribute of a DIFF channel, whose v_i is the query's own - in FX's. In front: the two effects. Behind: POSITION and the capacity of either side.
enum NeighboursFromDescError : uint32_t {
    kNbFromOk, kNbFromErrSameEffect, kNbFromErrContexts, kNbFromErrStructSize, kNbFromErrFlags, kNbFromErrDims, kNbFromErrOrigin, kNbFromErrInvCell, kNbFromErrRadius, kNbFromErrCoverage,
    kNbFromErrRadiusSquared, kNbFromErrWeight, kNbFromErrCandidateLimit, kNbFromErrChannelCount, kNbFromErrSrcAttr, kNbFromErrSrcComp, kNbFromErrChannelFlags, kNbFromErrDiffOne,
    kNbFromErrDiffAttr, kNbFromErrFracBits, kNbFromErrDstAttr, kNbFromErrDstComp, kNbFromErrOp, kNbFromErrChannelReserved, kNbFromErrDuplicate, kNbFromErrUnusedChannel, kNbFromErrScale,
    kNbFromErrStats, kNbFromErrNoPosition, kNbFromErrSourceNoPosition, kNbFromErrCapacity, kNbFromErrSourceCapacity, kNbFromDescErrorCount
};
HNB_SORT_KEY_FN const char* neighbours_from_error_text(uint32_t e) {
    switch (e) {
        case kNbFromOk: return "ok";
        case kNbFromErrSameEffect: return "fx and source are one effect: the sums within one effect are hnb_effect_neighbours'";
        case kNbFromErrContexts: return "fx and source belong to different contexts: the call is ordered on one context's stream";
        case kNbFromErrStructSize: return neighbour_error_text(kNeighbourErrStructSize);
        case kNbFromErrFlags: return neighbour_error_text(kNeighbourErrFlags);
        case kNbFromErrDims: return neighbour_error_text(kNeighbourErrDims);
        case kNbFromErrOrigin: return neighbour_error_text(kNeighbourErrOrigin);
        case kNbFromErrInvCell: return neighbour_error_text(kNeighbourErrInvCell);
        case kNbFromErrRadius: return neighbour_error_text(kNeighbourErrRadius);
        case kNbFromErrCoverage: return neighbour_error_text(kNeighbourErrCoverage);
        case kNbFromErrRadiusSquared: return neighbour_error_text(kNeighbourErrRadiusSquared);
        case kNbFromErrWeight: return neighbour_error_text(kNeighbourErrWeight);
        case kNbFromErrCandidateLimit: return neighbour_error_text(kNeighbourErrCandidateLimit);
        case kNbFromErrChannelCount: return neighbour_error_text(kNeighbourErrChannelCount);
        case kNbFromErrSrcAttr: return "the channel's src_attr is not HNB_SPLAT_ATTR_ONE or an f32 attribute of 1..4 components of the source's particle layout";
        case kNbFromErrSrcComp: return neighbour_error_text(kNeighbourErrSrcComp);
        case kNbFromErrChannelFlags: return neighbour_error_text(kNeighbourErrChannelFlags);
        case kNbFromErrDiffOne: return neighbour_error_text(kNeighbourErrDiffOne);
        case kNbFromErrDiffAttr: return "the channel's flags: HNB_NEIGHBOUR_DIFF of an attribute that is not an f32 attribute of fx's particle layout with src_comp below its component count";
        case kNbFromErrFracBits: return neighbour_error_text(kNeighbourErrFracBits);
        case kNbFromErrDstAttr: return "the channel's dst_attr is not an f32 attribute of 1..4 components of fx's particle layout other than AGE";
        case kNbFromErrDstComp: return neighbour_error_text(kNeighbourErrDstComp);
        case kNbFromErrOp: return neighbour_error_text(kNeighbourErrOp);
        case kNbFromErrChannelReserved: return neighbour_error_text(kNeighbourErrChannelReserved);
        case kNbFromErrDuplicate: return neighbour_error_text(kNeighbourErrDuplicate);
        case kNbFromErrUnusedChannel: return neighbour_error_text(kNeighbourErrUnusedChannel);
        case kNbFromErrScale: return neighbour_error_text(kNeighbourErrScale);
        case kNbFromErrStats: return neighbour_error_text(kNeighbourErrStats);
        case kNbFromErrNoPosition: return "fx's particle layout has no POSITION of 3 f32 components";
        case kNbFromErrSourceNoPosition: return "the source's particle layout has no POSITION of 3 f32 components";
        case kNbFromErrCapacity: return "fx has more than 0xFFFFFF00 slots";
        case kNbFromErrSourceCapacity: return "the source has more than 0xFFFFFF00 slots";
        default: return "?";
    }
}
struct NeighboursFromSide { const NeighbourLayoutAttr* layout; uint32_t n_layout, capacity; };   // what the check is told of one effect
struct NeighboursFromCheck {
    uint32_t error, channel;        // a NeighboursFromDescError and, for a channel's or an axis's, its index
    uint32_t n_cells;
    uint32_t q_position_index, s_position_index;   // the entries of POSITION in fx's and in the source's layout
    uint32_t src_index[HNB_NEIGHBOUR_MAX_CHANNELS];     // in the SOURCE's layout, or kNeighbourLayoutOne
    uint32_t own_index[HNB_NEIGHBOUR_MAX_CHANNELS];     // a DIFF channel's attribute in FX's layout (kNeighbourLayoutOne without the flag)
    uint32_t dst_index[HNB_NEIGHBOUR_MAX_CHANNELS];     // in FX's layout
    float r2, inv_r2;               // radius * radius and 1.0f / r2, in f32
    bool source_age, own_age;       // a channel reads AGE: stale ages are materialised first on the source; and, that channel being DIFF, on fx
};
HNB_SORT_KEY_FN uint32_t neighbours_from_find(const NeighboursFromSide& s, uint32_t attr) {
    uint32_t i = 0;
    while (i < s.n_layout && s.layout[i].attr != attr) ++i;
    return i;
}
HNB_SORT_KEY_FN bool neighbours_from_f32_attr(const NeighboursFromSide& s, uint32_t attr, uint32_t i) {
    return neighbour_storable_attr(attr) && i != s.n_layout && s.layout[i].is_f32 && s.layout[i].ncomp >= 1u && s.layout[i].ncomp <= 4u;
}
// The refusals of include/hanabi_amd_neighbours_from.h "Errors" but the NULL arguments, in the order listed there
HNB_SORT_KEY_FN NeighboursFromCheck neighbours_from_check_desc(const HnbNeighbourDesc& d, const NeighboursFromSide& fx, const NeighboursFromSide& source, bool same_effect,
                                                               bool same_context) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    NeighboursFromCheck c = {};
    const auto fail = [&c](uint32_t e, uint32_t k) { c.error = e; c.channel = k; return c; };
    if (same_effect) return fail(kNbFromErrSameEffect, 0);
    if (!same_context) return fail(kNbFromErrContexts, 0);
    if (d.struct_size != sizeof(HnbNeighbourDesc)) return fail(kNbFromErrStructSize, 0);
    if (d.flags != 0u) return fail(kNbFromErrFlags, 0);
    c.n_cells = bin_cell_count(d.dims);
    if (c.n_cells == 0u) return fail(kNbFromErrDims, 0);
    for (uint32_t a = 0; a < 3u; ++a) {
        if (!neighbour_is_finite(d.origin[a])) return fail(kNbFromErrOrigin, a);
        if (!neighbour_is_finite(d.inv_cell[a]) || !(d.inv_cell[a] > 0.0f)) return fail(kNbFromErrInvCell, a);
    }
    if (!neighbour_is_finite(d.radius) || !(d.radius > 0.0f)) return fail(kNbFromErrRadius, 0);
    for (uint32_t a = 0; a < 3u; ++a)
        if (!((double)d.radius * (double)d.inv_cell[a] <= 1.0)) return fail(kNbFromErrCoverage, a);
    c.r2 = d.radius * d.radius;
    c.inv_r2 = 1.0f / c.r2;
    if (!neighbour_is_finite(c.r2) || !neighbour_is_finite(c.inv_r2) || !(c.r2 >= 1.17549435e-38f)) return fail(kNbFromErrRadiusSquared, 0);
    if (d.weight > HNB_NEIGHBOUR_W_U3) return fail(kNbFromErrWeight, 0);
    if (d.candidate_limit == 0u || d.candidate_limit > HNB_NEIGHBOUR_MAX_CANDIDATES) return fail(kNbFromErrCandidateLimit, 0);
    if (d.n_channels == 0u || d.n_channels > HNB_NEIGHBOUR_MAX_CHANNELS) return fail(kNbFromErrChannelCount, 0);
    for (uint32_t k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
        const HnbNeighbourChannel& ch = d.channels[k];
        if (k >= d.n_channels) {
            if (ch.src_attr != 0u || ch.src_comp != 0u || ch.flags != 0u || ch.frac_bits != 0u || ch.dst_attr != 0u || ch.dst_comp != 0u || ch.op != 0u || ch.reserved != 0u)
                return fail(kNbFromErrUnusedChannel, k);
            continue;
        }
        c.own_index[k] = kNeighbourLayoutOne;
        if (ch.src_attr == HNB_SPLAT_ATTR_ONE) {
            if (ch.src_comp != 0u) return fail(kNbFromErrSrcComp, k);
            c.src_index[k] = kNeighbourLayoutOne;
        } else {
            const uint32_t i = neighbours_from_find(source, ch.src_attr);
            if (!neighbours_from_f32_attr(source, ch.src_attr, i)) return fail(kNbFromErrSrcAttr, k);
            if (ch.src_comp >= source.layout[i].ncomp) return fail(kNbFromErrSrcComp, k);
            c.src_index[k] = i;
        }
        if ((ch.flags & ~HNB_NEIGHBOUR_DIFF) != 0u) return fail(kNbFromErrChannelFlags, k);
        if (ch.flags != 0u && ch.src_attr == HNB_SPLAT_ATTR_ONE) return fail(kNbFromErrDiffOne, k);
        if (ch.flags != 0u) {                                              // v_i is the query's own stored value: the attribute is fx's as well
            const uint32_t i = neighbours_from_find(fx, ch.src_attr);
            if (!neighbours_from_f32_attr(fx, ch.src_attr, i) || ch.src_comp >= fx.layout[i].ncomp) return fail(kNbFromErrDiffAttr, k);
            c.own_index[k] = i;
        }
        if (ch.frac_bits > kDepositMaxFracBits) return fail(kNbFromErrFracBits, k);
        const uint32_t i = neighbours_from_find(fx, ch.dst_attr);
        if (ch.dst_attr == HNB_ATTR_AGE || !neighbours_from_f32_attr(fx, ch.dst_attr, i)) return fail(kNbFromErrDstAttr, k);
        if (ch.dst_comp >= fx.layout[i].ncomp) return fail(kNbFromErrDstComp, k);
        if (ch.op != HNB_SAMPLE_SET && ch.op != HNB_SAMPLE_ADD) return fail(kNbFromErrOp, k);
        if (ch.reserved != 0u) return fail(kNbFromErrChannelReserved, k);
        for (uint32_t e = 0; e < k; ++e)
            if (d.channels[e].dst_attr == ch.dst_attr && d.channels[e].dst_comp == ch.dst_comp) return fail(kNbFromErrDuplicate, k);
        c.dst_index[k] = i;
        if (ch.src_attr == HNB_ATTR_AGE) {
            c.source_age = true;
            if (ch.flags != 0u) c.own_age = true;
        }
    }
    if (!neighbour_is_finite(d.scale)) return fail(kNbFromErrScale, 0);
    if (((uintptr_t)d.out_stats & 15u) != 0u) return fail(kNbFromErrStats, 0);
    const NeighboursFromSide* side[2] = {&fx, &source};
    for (uint32_t s = 0; s < 2u; ++s) {
        const uint32_t p = neighbours_from_find(*side[s], HNB_ATTR_POSITION);
        if (p == side[s]->n_layout || !side[s]->layout[p].is_f32 || side[s]->layout[p].ncomp != 3u) return fail(s ? kNbFromErrSourceNoPosition : kNbFromErrNoPosition, 0);
        (s ? c.s_position_index : c.q_position_index) = p;
    }
    for (uint32_t s = 0; s < 2u; ++s)
        if (export_sort_scratch_layout(1u, side[s]->capacity, HNB_SORT_SCOPE_INSTANCE).rows == 0u) return fail(s ? kNbFromErrSourceCapacity : kNbFromErrCapacity, 0);
    return c;
}

// ---- the scratch ----------------------------------------------------------------------------------------------------------------------------------
// One allocation, owned by fx and apart from its d_neighbours and d_pairs; every section starts on a 256-byte boundary: the sorted export's layout of
// one instance for the SOURCE's capacity (the cells as keys, the slots as values, the digit tables), the same for FX's capacity, then the snapshot -
// 16 bytes per row of the source sort's pitch -, then 4 bytes per source row and channel, then the source's cell_start table of n_cells + 2 words.
// s_sort.rows == 0 or q_sort.rows == 0: more than 0xFFFFFF00 slots (refused).
struct NeighboursFromScratch { ExportSortScratch s_sort, q_sort; uint64_t q_sort_off, snap_off, snap_bytes, src_off, src_bytes, cells_off, cells_bytes, total; };
HNB_SORT_KEY_FN NeighboursFromScratch neighbours_from_scratch_layout(uint32_t q_capacity, uint32_t s_capacity, uint32_t n_channels, uint32_t n_cells) {
    NeighboursFromScratch l = {};
    const uint64_t align = 255u;
    l.s_sort = export_sort_scratch_layout(1u, s_capacity, HNB_SORT_SCOPE_INSTANCE);
    l.q_sort = export_sort_scratch_layout(1u, q_capacity, HNB_SORT_SCOPE_INSTANCE);
    l.q_sort_off = (l.s_sort.total + align) & ~align;
    l.snap_off = (l.q_sort_off + l.q_sort.total + align) & ~align;
    l.snap_bytes = (uint64_t)l.s_sort.pitch * 16u;
    l.src_off = (l.snap_off + l.snap_bytes + align) & ~align;
    l.src_bytes = (uint64_t)l.s_sort.pitch * 4u * n_channels;
    l.cells_off = (l.src_off + l.src_bytes + align) & ~align;
    l.cells_bytes = (uint64_t)export_bin_entries(n_cells) * 4u;
    l.total = (l.cells_off + l.cells_bytes + align) & ~align;
    return l;
}

// ---- the launches of a call -----------------------------------------------------------------------------------------------------------------------
// The kernel of hnb_neighbours_from.hip: the index of its handle in the context. Numbered apart from every other unit's.
enum NeighboursFromKernel : uint32_t { kNbFromKGather, kNeighboursFromKernelCount };
struct NeighboursFromKernelName { uint32_t kernel; const char* name; };
constexpr NeighboursFromKernelName kNeighboursFromKernelNames[kNeighboursFromKernelCount] = {{kNbFromKGather, "k_neighbours_from_gather"}};

struct NeighboursFromPlan {
    ExportPlan source_sort;         // the binned export's launches but its gather: (one workgroup | memset + keys + the sort's passes) + the table
    ExportPlan query_sort;          //   ... and but the table as well: the queries' order alone, into the second sort section (zero_off is within it)
    uint32_t pack_grid;             // k_neighbours_pack bound to the source: a lane per row of the source's capacity
    uint32_t gather_grid;           // k_neighbours_from_gather: a lane per row of fx's capacity
    uint64_t clear_stats_bytes;     // what the call zeroes in front when out_stats is given
};
// Both capacities must fit a sort (neighbours_from_check_desc). Decides; hanabi_amd.hip run_neighbours_from executes: the sorts through
// run_export_plan, each with the base of its own section.
HNB_SORT_KEY_FN NeighboursFromPlan neighbours_from_launch_plan(uint32_t q_capacity, uint32_t s_capacity, uint32_t n_cells) {
    NeighboursFromPlan pl = {};
    pl.source_sort = export_bin_launch_plan(s_capacity, 16u, n_cells);
    pl.source_sort.n -= 1u;         // (the last launch is the binned export's gather of records: there are none here)
    pl.query_sort = export_bin_launch_plan(q_capacity, 16u, n_cells);
    pl.query_sort.n -= 2u;          // (... and the one in front of it the table: the queries are looked up in the source's)
    const auto groups = [](uint32_t capacity) {
        const uint32_t g = (uint32_t)(((uint64_t)capacity + kNeighboursFromBlock - 1u) / kNeighboursFromBlock);
        return g ? g : 1u;
    };
    pl.pack_grid = groups(s_capacity);
    pl.gather_grid = groups(q_capacity);
    pl.clear_stats_bytes = kNeighboursFromStatsWords * 4u;
    return pl;
}

}  // namespace hnb
