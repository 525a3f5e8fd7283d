// The splat (hnb_effect_splat, hnb_program_splat; include/hanabi_amd_splat.h), shared by the kernels' translation unit (hnb_splat.hip: a code object
// of its own) and the runtime that loads and launches them (hanabi_amd.hip): the rule itself - the weights and corners of an axis, the eight
// (row, weight) pairs of an inside particle, the contribution of a value to a corner - as the functions the kernels call, the kernels' argument
// block, the kernels by name (SplatKernel), the check of a description (splat_check_desc) and the launch of a call (splat_launch_plan). The cell is
// the deposit's (hnb_bin_cell.h bin_cell_of), the quantisation the deposit's (hnb_deposit.h deposit_quantise), the stencil the sample's
// (hnb_sample.h sample_axis_t, sample_axis, sample_corner_rows): none is restated here. Plain C++: a host compiler takes it, so the tests state the
// rule with the kernels' own text and check the refusals and the plan without a GPU. Every f32 operation is a statement of its own, in the order the
// header writes it; nothing may be contracted into a fused multiply-add (the pragma for clang / hipcc; a host compiler builds this with
// -ffp-contract=off).
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd_splat.h"
#include "hnb_bin_cell.h"
#include "hnb_deposit.h"
#include "hnb_sample.h"
#include "hnb_sort_key.h"

namespace hnb {

constexpr uint32_t kSplatBlock = 256;               // lanes per workgroup
constexpr uint32_t kSplatTile = 4096;               // slots per tile: four quads of consecutive slots per lane (the deposit's walk)
constexpr uint32_t kSplatMaxInstances = kDepositMaxInstances;
constexpr uint32_t kSplatOneBits = 0x3F800000u;     // the stored value of a channel of HNB_SPLAT_ATTR_ONE: the bits of 1.0f
static_assert(kSplatTile == kDepositTile && kSplatBlock == kDepositBlock, "the splat walks the deposit's tiles");

// ---- the rule -------------------------------------------------------------------------------------------------------------------------------------
HNB_SORT_KEY_FN uint32_t splat_bits_of(float f) { uint32_t b; __builtin_memcpy(&b, &f, 4); return b; }
HNB_SORT_KEY_FN float splat_float_of(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }

// The two cell centres around t along an axis of `dim` cells (sample_axis) and the weights of both: w1 of the upper one, w0 = 1 - w1 of the lower.
// For an inside particle alone: both corners lie in 0 .. dim - 1, and w1 = u - floorf(u) is in [0, 1] (1.0 when a tiny negative u rounds up), so
// w0 is in [0, 1] too.
struct SplatAxis { uint32_t lo, hi; float w0, w1; };
HNB_SORT_KEY_FN SplatAxis splat_axis(float t, uint32_t dim) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const SampleAxis s = sample_axis(t, dim);
    SplatAxis a;
    a.lo = s.lo;
    a.hi = s.hi;
    a.w1 = s.w;
    a.w0 = 1.0f - s.w;
    return a;
}

// The eight corners of an inside particle in sample_corner_rows' order - corner i = a + 2 b + 4 c takes lo (0) or hi (1) along x (a), y (b), z (c) -
// with W = (w_a[x] * w_b[y]) * w_c[z]: two rounded products, in that order. Every row is below n_cells; clamped corners name the same row twice
// or more, and every one of them is added.
struct SplatCorners { uint32_t row[8]; float w[8]; };
HNB_SORT_KEY_FN SplatCorners splat_corners(const uint32_t* dims, const SplatAxis& x, const SplatAxis& y, const SplatAxis& z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    SplatCorners c;
    const SampleAxis sx = {x.lo, x.hi, x.w1}, sy = {y.lo, y.hi, y.w1}, sz = {z.lo, z.hi, z.w1};
    sample_corner_rows(dims, sx, sy, sz, c.row);
    const float xy[4] = {x.w0 * y.w0, x.w1 * y.w0, x.w0 * y.w1, x.w1 * y.w1};
    for (uint32_t i = 0; i < 4u; ++i) {
        c.w[i] = xy[i] * z.w0;
        c.w[4u + i] = xy[i] * z.w1;
    }
    return c;
}

// What the stored value v adds to a corner of weight W: cv = v * W, one rounded product, quantised as the deposit quantises a stored value. W is in
// [0, 1], so |cv| <= |v|: a value the deposit's rule accepts has eight accepted corners, and the acceptance is tested once, on v itself
// (deposit_quantise(bits_v, frac_bits).ok). |cv| < 2^-33 gives 0 at every frac_bits up to 32, so a product in the denormal range (below 2^-126)
// gives 0 whether the hardware keeps or flushes it.
HNB_SORT_KEY_FN int64_t splat_contribution(uint32_t bits_v, float W, uint32_t frac_bits) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float cv = splat_float_of(bits_v) * W;
    return deposit_quantise(splat_bits_of(cv), frac_bits).q;
}

// ---- the kernels' argument block ------------------------------------------------------------------------------------------------------------------
// The deposit's, unchanged: the same grid, destinations and walk. A channel of HNB_SPLAT_ATTR_ONE has no plane: its `packed` carries a component
// count of 0 (an attribute of the layout has 1..4), which is the marker the kernels test; plane_off is 0 and never added to anything.
typedef DepositArgs SplatArgs;
typedef DepositChannelArg SplatChannelArg;
HNB_SORT_KEY_FN uint32_t splat_pack_channel(bool one, uint32_t ncomp, uint32_t comp, uint32_t frac_bits) { return deposit_pack_channel(one ? 0u : ncomp, one ? 0u : comp, frac_bits); }
HNB_SORT_KEY_FN bool splat_channel_is_one(uint32_t packed) { return deposit_channel_ncomp(packed) == 0u; }
static_assert(sizeof(SplatArgs) == 184, "one SplatArgs by value");

// ---- the check of a description -------------------------------------------------------------------------------------------------------------------
// The deposit's errors by their numbers, and behind them the one the splat adds
constexpr uint32_t kSplatErrOneComp = kDepositDescErrorCount;
constexpr uint32_t kSplatDescErrorCount = kDepositDescErrorCount + 1u;
constexpr uint32_t kSplatLayoutOne = 0xFFFFFFFFu;   // SplatCheck::layout_index of a channel of HNB_SPLAT_ATTR_ONE: no entry of the layout
HNB_SORT_KEY_FN const char* splat_error_text(uint32_t e) {
    switch (e) {
        case kDepositErrAttr: return "the channel's attr is not HNB_SPLAT_ATTR_ONE or an f32 attribute of 1..4 components of the particle layout";
        case kSplatErrOneComp: return "the channel's attr is HNB_SPLAT_ATTR_ONE and its comp is not 0";
        default: return deposit_error_text(e);
    }
}
typedef DepositCheck SplatCheck;                    // (layout_index[k] == kSplatLayoutOne: channel k is HNB_SPLAT_ATTR_ONE)
// The refusals of include/hanabi_amd_splat.h "Errors" but the NULL arguments and the program's instance count: the deposit's, in its order, with a
// channel of HNB_SPLAT_ATTR_ONE admitted - its comp must be 0, its frac_bits and reserved follow the rule of every channel
HNB_SORT_KEY_FN SplatCheck splat_check_desc(const HnbDepositDesc& d, const DepositLayoutAttr* layout, uint32_t n_layout) {
    SplatCheck c = {};
    const auto fail = [&c](uint32_t e, uint32_t k) { c.error = e; c.channel = k; return c; };
    if (d.struct_size != sizeof(HnbDepositDesc)) return fail(kDepositErrStructSize, 0);
    if ((d.flags & ~HNB_DEPOSIT_ACCUMULATE) != 0u) return fail(kDepositErrFlags, 0);
    c.n_cells = bin_cell_count(d.dims);
    if (c.n_cells == 0u) return fail(kDepositErrDims, 0);
    for (uint32_t a = 0; a < 3u; ++a) {
        if (!deposit_is_finite(d.origin[a])) return fail(kDepositErrOrigin, a);
        if (!deposit_is_finite(d.inv_cell[a]) || !(d.inv_cell[a] > 0.0f)) return fail(kDepositErrInvCell, a);
    }
    if (d.n_channels > HNB_DEPOSIT_MAX_CHANNELS) return fail(kDepositErrChannelCount, 0);
    for (uint32_t k = 0; k < HNB_DEPOSIT_MAX_CHANNELS; ++k) {
        const HnbDepositChannel& ch = d.channels[k];
        if (k >= d.n_channels) {
            if (ch.attr != 0u || ch.comp != 0u || ch.frac_bits != 0u || ch.reserved != 0u) return fail(kDepositErrUnusedChannel, k);
            continue;
        }
        if (ch.attr == HNB_SPLAT_ATTR_ONE) {
            if (ch.comp != 0u) return fail(kSplatErrOneComp, k);
            c.layout_index[k] = kSplatLayoutOne;
        } else {
            uint32_t i = 0;
            while (i < n_layout && layout[i].attr != ch.attr) ++i;
            if (ch.attr == HNB_ATTR_ID || ch.attr == HNB_ATTR_PARTICLE_COUNTER || ch.attr >= HNB_ATTR_COUNT || i == n_layout || !layout[i].is_f32 || layout[i].ncomp < 1u ||
                layout[i].ncomp > 4u)
                return fail(kDepositErrAttr, k);
            if (ch.comp >= layout[i].ncomp) return fail(kDepositErrComp, k);
            c.layout_index[k] = i;
        }
        if (ch.frac_bits > kDepositMaxFracBits) return fail(kDepositErrFracBits, k);
        if (ch.reserved != 0u) return fail(kDepositErrChannelReserved, k);
        if (ch.attr == HNB_ATTR_AGE) c.has_age = true;
    }
    if (!d.count || ((uintptr_t)d.count & 15u) != 0u) return fail(kDepositErrCount, 0);
    if ((d.n_channels != 0u) != (d.sums != nullptr) || ((uintptr_t)d.sums & 15u) != 0u) return fail(kDepositErrSums, 0);
    if (((uintptr_t)d.out_stats & 15u) != 0u) return fail(kDepositErrStats, 0);
    uint32_t p = 0;
    while (p < n_layout && layout[p].attr != HNB_ATTR_POSITION) ++p;
    if (p == n_layout || !layout[p].is_f32 || layout[p].ncomp != 3u) return fail(kDepositErrNoPosition, 0);
    c.position_index = p;
    return c;
}

// ---- the launch of a call -------------------------------------------------------------------------------------------------------------------------
// The kernels of hnb_splat.hip: the index of a kernel's handle in the context. Numbered apart from the deposit's.
enum SplatKernel : uint32_t { kSplatKLds, kSplatKGlobal, kSplatKernelCount };
struct SplatKernelName { uint32_t kernel; const char* name; };
constexpr SplatKernelName kSplatKernelNames[kSplatKernelCount] = {{kSplatKLds, "k_splat_lds"}, {kSplatKGlobal, "k_splat_global"}};

struct SplatPlan {
    uint32_t kernel;                // a SplatKernel
    uint32_t grid_x, grid_y;        // workgroups of kSplatBlock lanes: groups per instance x instances
    uint32_t span;                  // tiles per workgroup
    uint32_t lds_bytes;             // k_splat_lds: the workgroup's table (dynamic LDS); 0 for k_splat_global
    uint64_t clear_count_bytes, clear_sums_bytes, clear_stats_bytes;   // what a call without HNB_DEPOSIT_ACCUMULATE zeroes in front (stats: when given)
};
// The deposit's decision on the deposit's table, named apart: a table within kDepositLdsBudget goes to k_splat_lds, a workgroup per span of
// ceil(table / kDepositSpanBytes) tiles; a larger one to k_splat_global, a workgroup per tile. Decides; hanabi_amd.hip run_splat executes.
HNB_SORT_KEY_FN SplatPlan splat_launch_plan(bool program, uint32_t n_inst, uint32_t capacity, uint32_t n_cells, uint32_t n_channels) {
    SplatPlan pl = {};
    const uint64_t table = deposit_table_bytes(n_cells, n_channels);
    uint32_t tiles = (uint32_t)(((uint64_t)capacity + kSplatTile - 1u) / kSplatTile);
    if (tiles == 0u) tiles = 1u;
    pl.grid_y = program ? n_inst : 1u;
    if (table <= kDepositLdsBudget) {
        pl.kernel = kSplatKLds;
        pl.span = (uint32_t)((table + kDepositSpanBytes - 1u) / kDepositSpanBytes);      // 1..24
        pl.grid_x = (tiles + pl.span - 1u) / pl.span;
        pl.lds_bytes = (uint32_t)table;
    } else {
        pl.kernel = kSplatKGlobal;
        pl.span = 1u;
        pl.grid_x = tiles;
    }
    pl.clear_count_bytes = ((uint64_t)n_cells + 1u) * 4u;
    pl.clear_sums_bytes = ((uint64_t)n_cells + 1u) * 8u * n_channels;
    pl.clear_stats_bytes = 16u;
    return pl;
}

}  // namespace hnb
