// The neighbour sums (hnb_effect_neighbours; include/hanabi_amd_neighbours.h), shared by the kernels' translation unit (hnb_neighbours.hip: a code
// object of its own) and the runtime that loads and launches them (hanabi_amd.hip): the pair rule - the squared distance, the weight, a
// contribution on top of the deposit's quantisation -, the store, the row ranges and the candidate count of a cell from a cell_start table, the
// kernels' argument block, the kernels by name (NeighbourKernel), the check of a description (neighbour_check_desc), the scratch layout and the
// launches of a call (neighbour_launch_plan). Plain C++: a host compiler takes it, so the tests state the rule with the kernels' own text and check
// the refusals, the layout and the plan without a GPU. Every f32 operation is a statement of its own, in the order the header writes it; nothing
// may be contracted into a fused multiply-add (the pragma for clang / hipcc; a host compiler builds this with -ffp-contract=off).
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd_neighbours.h"
#include "../../include/hanabi_amd_sample.h"
#include "hnb_bin_cell.h"
#include "hnb_deposit.h"
#include "hnb_export_bin.h"
#include "hnb_sort_key.h"

namespace hnb {

constexpr uint32_t kNeighbourBlock = 256;           // lanes per workgroup: one sorted row per lane
constexpr uint32_t kNeighbourStatsWords = 8;
constexpr uint32_t kNeighbourOneBits = 0x3F800000u; // the stored value of a source of HNB_SPLAT_ATTR_ONE: the bits of 1.0f

HNB_SORT_KEY_FN float neighbour_f32(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }
HNB_SORT_KEY_FN uint32_t neighbour_bits(float f) { uint32_t b; __builtin_memcpy(&b, &f, 4); return b; }

// ---- the pair rule --------------------------------------------------------------------------------------------------------------------------------
HNB_SORT_KEY_FN float neighbour_d2(float xi, float yi, float zi, float xj, float yj, float zj) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float dx = xj - xi;
    const float dy = yj - yi;
    const float dz = zj - zi;
    const float xx = dx * dx;
    const float yy = dy * dy;
    const float zz = dz * dz;
    const float s = xx + yy;
    const float d2 = s + zz;
    return d2;
}

// W of a pair at d2 for a weight other than HNB_NEIGHBOUR_W_ONE (for which neither q nor u is formed: 1.0f)
HNB_SORT_KEY_FN float neighbour_weight(uint32_t weight, float d2, float inv_r2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (weight == HNB_NEIGHBOUR_W_ONE) return 1.0f;
    const float q = d2 * inv_r2;
    const float u = 1.0f - q;
    const float u2 = u * u;
    const float u3 = u2 * u;
    return weight == HNB_NEIGHBOUR_W_U1 ? u : weight == HNB_NEIGHBOUR_W_U2 ? u2 : u3;
}

// The contribution of a neighbour whose stored source is vj to a query whose own is vi: v = vj or (diff) vj - vi; cv = v * W, or v itself under
// HNB_NEIGHBOUR_W_ONE; then the deposit's quantisation
HNB_SORT_KEY_FN DepositQuant neighbour_contribution(uint32_t vj_bits, uint32_t vi_bits, bool diff, uint32_t weight, float W, uint32_t frac_bits) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float vj = neighbour_f32(vj_bits), vi = neighbour_f32(vi_bits);
    const float d = vj - vi;
    const float v = diff ? d : vj;
    const float p = v * W;
    const float cv = weight == HNB_NEIGHBOUR_W_ONE ? v : p;
    return deposit_quantise(neighbour_bits(cv), frac_bits);
}

// v' of the stored value v and the sum S in units of 2^-frac_bits: r = (float)S; r = r * 2^-frac_bits; r = r * scale; SET: r; ADD: v + r
HNB_SORT_KEY_FN float neighbour_store(uint32_t op, float v, int64_t S, uint32_t frac_bits, float scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float unit = neighbour_f32((127u - frac_bits) << 23);      // 2^-frac_bits, frac_bits <= 32: a normal number
    const float r0 = (float)S;                                      // to nearest, ties to even
    const float r1 = r0 * unit;
    const float r = r1 * scale;
    const float sum = v + r;
    return op == HNB_SAMPLE_ADD ? sum : r;
}

// ---- the walk -------------------------------------------------------------------------------------------------------------------------------------
// The cell (cx, cy, cz) of an inside particle from its index
struct NeighbourCell { uint32_t x, y, z; };
HNB_SORT_KEY_FN NeighbourCell neighbour_cell_xyz(const uint32_t* dims, uint32_t cell) {
    NeighbourCell c;
    c.x = cell % dims[0];
    const uint32_t t = cell / dims[0];
    c.y = t % dims[1];
    c.z = t / dims[1];
    return c;
}

// Range i (0..8: dy = i % 3 - 1, dz = i / 3 - 1) of the walk around cell c: along x the up to three adjacent cells of one (y, z) are one contiguous
// range of the rows in cell order, [cell_start[first], cell_start[last + 1]), the grid's edges clamped. A (y, z) beyond the grid's edge does not
// exist: lo == hi == 0. cell_start: the binned export's table of n_cells + 2 entries; the largest index read is n_cells.
struct NeighbourRange { uint32_t lo, hi; };
HNB_SORT_KEY_FN NeighbourRange neighbour_range(const uint32_t* cell_start, const uint32_t* dims, const NeighbourCell& c, uint32_t i) {
    NeighbourRange r = {0u, 0u};
    const uint32_t dy = i % 3u, dz = i / 3u;                        // 0..2 for -1..1
    const uint32_t y = c.y + dy, z = c.z + dz;                      // the row's (y, z) plus 1
    if (y < 1u || y > dims[1] || z < 1u || z > dims[2]) return r;
    const uint32_t x0 = c.x > 0u ? c.x - 1u : 0u, x1 = c.x + 1u < dims[0] ? c.x + 1u : dims[0] - 1u;
    const uint32_t row = ((z - 1u) * dims[1] + (y - 1u)) * dims[0];
    r.lo = cell_start[row + x0];
    r.hi = cell_start[row + x1 + 1u];
    return r;
}

// candidates(i): the inside particles of the up to 27 cells around c, the query itself included. The ranges are disjoint: at most the inside rows.
HNB_SORT_KEY_FN uint32_t neighbour_candidates(const uint32_t* cell_start, const uint32_t* dims, const NeighbourCell& c) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < 9u; ++i) {
        const NeighbourRange r = neighbour_range(cell_start, dims, c, i);
        n += r.hi - r.lo;
    }
    return n;
}

// ---- the kernels' argument block ------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kNeighbourSrcOne = 1u << 16, kNeighbourSrcDiff = 1u << 17;
struct NeighbourChannelArg {
    uint64_t src_plane_off;         // bytes from the slab base: the source's plane, ncomp * 4 bytes per slot (not read for HNB_SPLAT_ATTR_ONE)
    uint64_t dst_plane_off;         //   ... and the destination's
    uint32_t src_packed;            // ncomp | comp << 8 | kNeighbourSrcOne | kNeighbourSrcDiff | frac_bits << 24
    uint32_t dst_packed;            // ncomp | comp << 8 | op << 16 (sample_pack_channel's)
};
HNB_SORT_KEY_FN uint32_t neighbour_pack_src(uint32_t ncomp, uint32_t comp, bool one, bool diff, uint32_t frac_bits) {
    return ncomp | (comp << 8) | (one ? kNeighbourSrcOne : 0u) | (diff ? kNeighbourSrcDiff : 0u) | (frac_bits << 24);
}
HNB_SORT_KEY_FN uint32_t neighbour_pack_dst(uint32_t ncomp, uint32_t comp, uint32_t op) { return ncomp | (comp << 8) | (op << 16); }
struct NeighbourArgs {
    const uint64_t* slab;           // [1] the instance's slab base address
    const HnbDeviceMeta* meta;      // [1] its row after the frames enqueued so far
    const uint32_t* keys;           // the sort's [2][pitch] cells and
    const uint32_t* vals;           //   slots, ping-pong: the state words say which half holds the order
    const ExportSortState* state;
    uint32_t* snap;                 // [pitch][4]: (x, y, z, slot) of sorted row r
    uint32_t* srcv;                 // [n_channels][pitch]: channel k's stored source of sorted row r
    const uint32_t* cell_start;     // [n_cells + 2]
    uint32_t* stats;                // [8] or NULL
    uint64_t pos_off;               // bytes from the slab base: POSITION, 12 bytes per slot
    BinGrid grid;
    uint32_t capacity, pitch, n_channels, weight, candidate_limit;
    float r2, inv_r2, scale;
    NeighbourChannelArg ch[HNB_NEIGHBOUR_MAX_CHANNELS];
};
static_assert(sizeof(HnbNeighbourChannel) == 32 && sizeof(HnbNeighbourDesc) == 200, "HnbNeighbourChannel / HnbNeighbourDesc layout");
static_assert(sizeof(NeighbourChannelArg) == 24 && sizeof(NeighbourArgs) == 248, "one NeighbourArgs by value");

// ---- the check of a description -------------------------------------------------------------------------------------------------------------------
enum NeighbourDescError : uint32_t {
    kNeighbourOk, kNeighbourErrStructSize, kNeighbourErrFlags, kNeighbourErrDims, kNeighbourErrOrigin, kNeighbourErrInvCell, kNeighbourErrRadius, kNeighbourErrCoverage,
    kNeighbourErrRadiusSquared, kNeighbourErrWeight, kNeighbourErrCandidateLimit, kNeighbourErrChannelCount, kNeighbourErrSrcAttr, kNeighbourErrSrcComp, kNeighbourErrChannelFlags,
    kNeighbourErrDiffOne, kNeighbourErrFracBits, kNeighbourErrDstAttr, kNeighbourErrDstComp, kNeighbourErrOp, kNeighbourErrChannelReserved, kNeighbourErrDuplicate,
    kNeighbourErrUnusedChannel, kNeighbourErrScale, kNeighbourErrStats, kNeighbourErrNoPosition, kNeighbourErrCapacity, kNeighbourDescErrorCount
};
HNB_SORT_KEY_FN const char* neighbour_error_text(uint32_t e) {
    switch (e) {
        case kNeighbourOk: return "ok";
        case kNeighbourErrStructSize: return "struct_size is not this library's sizeof(HnbNeighbourDesc)";
        case kNeighbourErrFlags: return "flags: 0";
        case kNeighbourErrDims: return "dims: every dims[c] >= 1 and their product at most HNB_BIN_MAX_CELLS";
        case kNeighbourErrOrigin: return "origin is not finite";
        case kNeighbourErrInvCell: return "inv_cell is not finite and above 0";
        case kNeighbourErrRadius: return "radius is not finite and above 0";
        case kNeighbourErrCoverage: return "radius * inv_cell is above 1 on an axis: the ball reaches past the 26 cells around a cell";
        case kNeighbourErrRadiusSquared: return "radius * radius or its reciprocal is not finite in f32, or radius * radius is not a normal number";
        case kNeighbourErrWeight: return "weight: HNB_NEIGHBOUR_W_ONE, _W_U1, _W_U2 or _W_U3";
        case kNeighbourErrCandidateLimit: return "candidate_limit is not 1..HNB_NEIGHBOUR_MAX_CANDIDATES";
        case kNeighbourErrChannelCount: return "n_channels is not 1..HNB_NEIGHBOUR_MAX_CHANNELS";
        case kNeighbourErrSrcAttr: return "the channel's src_attr is not HNB_SPLAT_ATTR_ONE or an f32 attribute of 1..4 components of the particle layout";
        case kNeighbourErrSrcComp: return "the channel's src_comp is at or past the source's component count (HNB_SPLAT_ATTR_ONE: not 0)";
        case kNeighbourErrChannelFlags: return "the channel's flags: 0 or HNB_NEIGHBOUR_DIFF";
        case kNeighbourErrDiffOne: return "the channel's flags: HNB_NEIGHBOUR_DIFF of HNB_SPLAT_ATTR_ONE";
        case kNeighbourErrFracBits: return "the channel's frac_bits is above 32";
        case kNeighbourErrDstAttr: return "the channel's dst_attr is not an f32 attribute of 1..4 components of the particle layout other than AGE";
        case kNeighbourErrDstComp: return "the channel's dst_comp is at or past the attribute's component count";
        case kNeighbourErrOp: return "the channel's op: HNB_SAMPLE_SET or HNB_SAMPLE_ADD";
        case kNeighbourErrChannelReserved: return "the channel's reserved is not 0";
        case kNeighbourErrDuplicate: return "the channel's (dst_attr, dst_comp) is an earlier channel's";
        case kNeighbourErrUnusedChannel: return "a channel entry at or past n_channels is not all 0";
        case kNeighbourErrScale: return "scale is not finite";
        case kNeighbourErrStats: return "out_stats: NULL or a 16-byte aligned device pointer";
        case kNeighbourErrNoPosition: return "the particle layout has no POSITION of 3 f32 components";
        case kNeighbourErrCapacity: return "the effect has more than 0xFFFFFF00 slots";
        default: return "?";
    }
}
constexpr uint32_t kNeighbourLayoutOne = 0xFFFFFFFFu;   // NeighbourCheck::src_index of a channel of HNB_SPLAT_ATTR_ONE: no entry of the layout
struct NeighbourLayoutAttr { uint32_t attr, ncomp, is_f32; };    // what the check is told of the program's layout
struct NeighbourCheck {
    uint32_t error, channel;        // a NeighbourDescError and, for a channel's or an axis's, its index
    uint32_t n_cells;
    uint32_t position_index;        // the layout's entry of POSITION
    uint32_t src_index[HNB_NEIGHBOUR_MAX_CHANNELS], dst_index[HNB_NEIGHBOUR_MAX_CHANNELS];
    float r2, inv_r2;               // radius * radius and 1.0f / r2, in f32
    bool has_age;                   // a channel reads AGE: stale ages are materialised first
};
HNB_SORT_KEY_FN bool neighbour_is_finite(float f) { return f - f == 0.0f; }     // (a NaN or an infinity minus itself is a NaN)
HNB_SORT_KEY_FN bool neighbour_storable_attr(uint32_t attr) { return attr != HNB_ATTR_ID && attr != HNB_ATTR_PARTICLE_COUNTER && attr < HNB_ATTR_COUNT; }
// The refusals of include/hanabi_amd_neighbours.h "Errors" but the NULL arguments, in the order listed there
HNB_SORT_KEY_FN NeighbourCheck neighbour_check_desc(const HnbNeighbourDesc& d, const NeighbourLayoutAttr* layout, uint32_t n_layout, uint32_t capacity) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    NeighbourCheck c = {};
    const auto fail = [&c](uint32_t e, uint32_t k) { c.error = e; c.channel = k; return c; };
    if (d.struct_size != sizeof(HnbNeighbourDesc)) return fail(kNeighbourErrStructSize, 0);
    if (d.flags != 0u) return fail(kNeighbourErrFlags, 0);
    c.n_cells = bin_cell_count(d.dims);
    if (c.n_cells == 0u) return fail(kNeighbourErrDims, 0);
    for (uint32_t a = 0; a < 3u; ++a) {
        if (!neighbour_is_finite(d.origin[a])) return fail(kNeighbourErrOrigin, a);
        if (!neighbour_is_finite(d.inv_cell[a]) || !(d.inv_cell[a] > 0.0f)) return fail(kNeighbourErrInvCell, a);
    }
    if (!neighbour_is_finite(d.radius) || !(d.radius > 0.0f)) return fail(kNeighbourErrRadius, 0);
    for (uint32_t a = 0; a < 3u; ++a)
        if (!((double)d.radius * (double)d.inv_cell[a] <= 1.0)) return fail(kNeighbourErrCoverage, a);
    c.r2 = d.radius * d.radius;
    c.inv_r2 = 1.0f / c.r2;
    if (!neighbour_is_finite(c.r2) || !neighbour_is_finite(c.inv_r2) || !(c.r2 >= 1.17549435e-38f)) return fail(kNeighbourErrRadiusSquared, 0);
    if (d.weight > HNB_NEIGHBOUR_W_U3) return fail(kNeighbourErrWeight, 0);
    if (d.candidate_limit == 0u || d.candidate_limit > HNB_NEIGHBOUR_MAX_CANDIDATES) return fail(kNeighbourErrCandidateLimit, 0);
    if (d.n_channels == 0u || d.n_channels > HNB_NEIGHBOUR_MAX_CHANNELS) return fail(kNeighbourErrChannelCount, 0);
    for (uint32_t k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
        const HnbNeighbourChannel& ch = d.channels[k];
        if (k >= d.n_channels) {
            if (ch.src_attr != 0u || ch.src_comp != 0u || ch.flags != 0u || ch.frac_bits != 0u || ch.dst_attr != 0u || ch.dst_comp != 0u || ch.op != 0u || ch.reserved != 0u)
                return fail(kNeighbourErrUnusedChannel, k);
            continue;
        }
        if (ch.src_attr == HNB_SPLAT_ATTR_ONE) {
            if (ch.src_comp != 0u) return fail(kNeighbourErrSrcComp, k);
            c.src_index[k] = kNeighbourLayoutOne;
        } else {
            uint32_t i = 0;
            while (i < n_layout && layout[i].attr != ch.src_attr) ++i;
            if (!neighbour_storable_attr(ch.src_attr) || i == n_layout || !layout[i].is_f32 || layout[i].ncomp < 1u || layout[i].ncomp > 4u) return fail(kNeighbourErrSrcAttr, k);
            if (ch.src_comp >= layout[i].ncomp) return fail(kNeighbourErrSrcComp, k);
            c.src_index[k] = i;
        }
        if ((ch.flags & ~HNB_NEIGHBOUR_DIFF) != 0u) return fail(kNeighbourErrChannelFlags, k);
        if (ch.flags != 0u && ch.src_attr == HNB_SPLAT_ATTR_ONE) return fail(kNeighbourErrDiffOne, k);
        if (ch.frac_bits > kDepositMaxFracBits) return fail(kNeighbourErrFracBits, k);
        uint32_t i = 0;
        while (i < n_layout && layout[i].attr != ch.dst_attr) ++i;
        if (ch.dst_attr == HNB_ATTR_AGE || !neighbour_storable_attr(ch.dst_attr) || i == n_layout || !layout[i].is_f32 || layout[i].ncomp < 1u || layout[i].ncomp > 4u)
            return fail(kNeighbourErrDstAttr, k);
        if (ch.dst_comp >= layout[i].ncomp) return fail(kNeighbourErrDstComp, k);
        if (ch.op != HNB_SAMPLE_SET && ch.op != HNB_SAMPLE_ADD) return fail(kNeighbourErrOp, k);
        if (ch.reserved != 0u) return fail(kNeighbourErrChannelReserved, k);
        for (uint32_t e = 0; e < k; ++e)
            if (d.channels[e].dst_attr == ch.dst_attr && d.channels[e].dst_comp == ch.dst_comp) return fail(kNeighbourErrDuplicate, k);
        c.dst_index[k] = i;
        if (ch.src_attr == HNB_ATTR_AGE) c.has_age = true;
    }
    if (!neighbour_is_finite(d.scale)) return fail(kNeighbourErrScale, 0);
    if (((uintptr_t)d.out_stats & 15u) != 0u) return fail(kNeighbourErrStats, 0);
    uint32_t p = 0;
    while (p < n_layout && layout[p].attr != HNB_ATTR_POSITION) ++p;
    if (p == n_layout || !layout[p].is_f32 || layout[p].ncomp != 3u) return fail(kNeighbourErrNoPosition, 0);
    c.position_index = p;
    if (export_sort_scratch_layout(1u, capacity, HNB_SORT_SCOPE_INSTANCE).rows == 0u) return fail(kNeighbourErrCapacity, 0);
    return c;
}

// ---- the scratch ----------------------------------------------------------------------------------------------------------------------------------
// One allocation per effect; every section starts on a 256-byte boundary: the sorted export's layout of one instance (the cells as keys, the slots
// as values, the digit tables), then the snapshot - 16 bytes per row of the sort's pitch - then 4 bytes per row and channel for the sources, then
// the cell_start table of n_cells + 2 words. sort.rows == 0: more than 0xFFFFFF00 slots (refused).
struct NeighbourScratch { ExportSortScratch sort; uint64_t snap_off, snap_bytes, src_off, src_bytes, cells_off, cells_bytes, total; };
HNB_SORT_KEY_FN NeighbourScratch neighbour_scratch_layout(uint32_t capacity, uint32_t n_channels, uint32_t n_cells) {
    NeighbourScratch l = {};
    const uint64_t align = 255u;
    l.sort = export_sort_scratch_layout(1u, capacity, HNB_SORT_SCOPE_INSTANCE);
    l.snap_off = (l.sort.total + align) & ~align;
    l.snap_bytes = (uint64_t)l.sort.pitch * 16u;
    l.src_off = (l.snap_off + l.snap_bytes + align) & ~align;
    l.src_bytes = (uint64_t)l.sort.pitch * 4u * n_channels;
    l.cells_off = (l.src_off + l.src_bytes + align) & ~align;
    l.cells_bytes = (uint64_t)export_bin_entries(n_cells) * 4u;
    l.total = (l.cells_off + l.cells_bytes + align) & ~align;
    return l;
}

// ---- the launches of a call -----------------------------------------------------------------------------------------------------------------------
// The kernels of hnb_neighbours.hip: the index of a kernel's handle in the context. Numbered apart from every other unit's.
enum NeighbourKernel : uint32_t { kNeighbourKPack, kNeighbourKGather, kNeighbourKernelCount };
struct NeighbourKernelName { uint32_t kernel; const char* name; };
constexpr NeighbourKernelName kNeighbourKernelNames[kNeighbourKernelCount] = {{kNeighbourKPack, "k_neighbours_pack"}, {kNeighbourKGather, "k_neighbours_gather"}};

struct NeighbourPlan {
    ExportPlan sort;                // the binned export's launches but its gather: (one workgroup | memset + keys + the sort's passes) + the table
    uint32_t pack_grid, gather_grid;    // workgroups of kNeighbourBlock lanes behind them: a lane per row of the capacity
    uint64_t clear_stats_bytes;     // what the call zeroes in front when out_stats is given
};
// A capacity must fit a sort (neighbour_check_desc). Decides; hanabi_amd.hip run_neighbours executes: the sort's part through run_export_plan.
HNB_SORT_KEY_FN NeighbourPlan neighbour_launch_plan(uint32_t capacity, uint32_t n_cells) {
    NeighbourPlan pl = {};
    pl.sort = export_bin_launch_plan(capacity, 16u, n_cells);
    pl.sort.n -= 1u;                // (the last launch is the binned export's gather of records: there are none here)
    uint32_t groups = (uint32_t)(((uint64_t)capacity + kNeighbourBlock - 1u) / kNeighbourBlock);
    if (groups == 0u) groups = 1u;
    pl.pack_grid = groups;
    pl.gather_grid = groups;
    pl.clear_stats_bytes = kNeighbourStatsWords * 4u;
    return pl;
}

}  // namespace hnb
