// The sample (hnb_effect_sample; include/hanabi_amd_sample.h), shared by the kernels' translation unit (hnb_sample.hip: a code object of its own) and
// the runtime that loads and launches them (hanabi_amd.hip): the sampling rule itself - the weights and corners of an axis, the blend, the store -
// as the functions the kernels call, the kernels' argument block, the kernels by name (SampleKernel), the check of a description
// (sample_check_desc) and the launch of a call (sample_launch_plan). Plain C++: a host compiler takes it, so the tests state the rule with the
// kernels' own text and check the refusals and the plan without a GPU. Every f32 operation is a statement of its own, in the order the header
// writes it; nothing may be contracted into a fused multiply-add (the pragma for clang / hipcc; a host compiler builds this with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/hanabi_amd_sample.h"
#include "hnb_bin_cell.h"
#include "hnb_sort_key.h"

namespace hnb {

constexpr uint32_t kSampleBlock = 256;              // lanes per workgroup
constexpr uint32_t kSampleTile = 4096;              // slots per tile: four quads of consecutive slots per lane (the deposit's walk)

// ---- the rule -------------------------------------------------------------------------------------------------------------------------------------
// t of an axis, bin_cell_of's two statements: the same operands in the same order give the same bits
HNB_SORT_KEY_FN float sample_axis_t(float p, float origin, float inv_cell) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float d = p - origin;
    const float t = d * inv_cell;
    return t;
}

// The two cell centres around t along an axis of `dim` cells and the weight of the upper one. For an inside particle alone: t in [0, dim), so
// u is in [-0.5, dim - 0.5], fl in -1 .. dim - 1 and both corners in 0 .. dim - 1.
struct SampleAxis { uint32_t lo, hi; float w; };
HNB_SORT_KEY_FN SampleAxis sample_axis(float t, uint32_t dim) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float u = t - 0.5f;
    const float fl = floorf(u);
    SampleAxis a;
    a.w = u - fl;
    const int32_t j = (int32_t)fl;
    const int32_t up = j + 1, last = (int32_t)dim - 1;
    a.lo = (uint32_t)(j > 0 ? j : 0);
    a.hi = (uint32_t)(up < last ? up : last);
    return a;
}

HNB_SORT_KEY_FN float sample_lerp(float lo, float hi, float w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float d = hi - lo;
    const float m = w * d;
    return lo + m;
}

// c[x + 2 y + 4 z]: the corner at (x ? hi0 : lo0, y ? hi1 : lo1, z ? hi2 : lo2). Along x four times, along y twice, along z once.
HNB_SORT_KEY_FN float sample_blend(const float* c, float w0, float w1, float w2) {
    const float a00 = sample_lerp(c[0], c[1], w0), a10 = sample_lerp(c[2], c[3], w0), a01 = sample_lerp(c[4], c[5], w0), a11 = sample_lerp(c[6], c[7], w0);
    const float b0 = sample_lerp(a00, a10, w1), b1 = sample_lerp(a01, a11, w1);
    return sample_lerp(b0, b1, w2);
}

// The rows of the eight corners, in sample_blend's order: row = (z * dims[1] + y) * dims[0] + x, below n_cells
HNB_SORT_KEY_FN void sample_corner_rows(const uint32_t* dims, const SampleAxis& x, const SampleAxis& y, const SampleAxis& z, uint32_t* rows) {
    const uint32_t zy[4] = {(z.lo * dims[1] + y.lo) * dims[0], (z.lo * dims[1] + y.hi) * dims[0], (z.hi * dims[1] + y.lo) * dims[0], (z.hi * dims[1] + y.hi) * dims[0]};
    for (uint32_t i = 0; i < 4u; ++i) {
        rows[2u * i] = zy[i] + x.lo;
        rows[2u * i + 1u] = zy[i] + x.hi;
    }
}

// v' of the stored value v and the sample s: r = s * scale; SET: r; ADD: v + r
HNB_SORT_KEY_FN float sample_store(uint32_t op, float v, float s, float scale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float r = s * scale;
    const float sum = v + r;
    return op == HNB_SAMPLE_ADD ? sum : r;
}

// ---- the kernels' argument block ------------------------------------------------------------------------------------------------------------------
struct SampleChannelArg {
    uint64_t plane_off;             // bytes from the slab base: the attribute's plane, ncomp * 4 bytes per slot
    uint32_t packed;                // ncomp | comp << 8 | op << 16 (sample_pack_channel): one scalar register
    uint32_t pad;
};
HNB_SORT_KEY_FN uint32_t sample_pack_channel(uint32_t ncomp, uint32_t comp, uint32_t op) { return ncomp | (comp << 8) | (op << 16); }
HNB_SORT_KEY_FN uint32_t sample_channel_ncomp(uint32_t packed) { return packed & 0xFFu; }
HNB_SORT_KEY_FN uint32_t sample_channel_comp(uint32_t packed) { return (packed >> 8) & 0xFFu; }
HNB_SORT_KEY_FN uint32_t sample_channel_op(uint32_t packed) { return packed >> 16; }
struct SampleArgs {
    const uint64_t* slab;           // the instance's slab base address (its row of the program's table)
    const HnbDeviceMeta* meta;      // its row after the frames enqueued so far
    const float* field;             // [n_cells * n_channels]
    uint32_t* stats;                // [4] or NULL
    uint64_t pos_off;               // bytes from the slab base: POSITION, 12 bytes per slot
    uint64_t flag_off;              //   ... and the alive bytes, one per slot
    BinGrid grid;
    uint32_t capacity, tiles;       // tiles of kSampleTile slots
    uint32_t n_channels;
    float scale;
    SampleChannelArg ch[HNB_SAMPLE_MAX_CHANNELS];
};
static_assert(sizeof(HnbSampleChannel) == 16 && sizeof(HnbSampleDesc) == 136, "HnbSampleChannel / HnbSampleDesc layout");
static_assert(sizeof(SampleArgs) == 168, "one SampleArgs by value");

// ---- the check of a description -------------------------------------------------------------------------------------------------------------------
enum SampleDescError : uint32_t {
    kSampleOk, kSampleErrStructSize, kSampleErrFlags, kSampleErrMode, kSampleErrDims, kSampleErrOrigin, kSampleErrInvCell, kSampleErrChannelCount, kSampleErrAttr, kSampleErrComp,
    kSampleErrOp, kSampleErrChannelReserved, kSampleErrDuplicate, kSampleErrUnusedChannel, kSampleErrScale, kSampleErrField, kSampleErrStats, kSampleErrNoPosition, kSampleDescErrorCount
};
HNB_SORT_KEY_FN const char* sample_error_text(uint32_t e) {
    switch (e) {
        case kSampleOk: return "ok";
        case kSampleErrStructSize: return "struct_size is not this library's sizeof(HnbSampleDesc)";
        case kSampleErrFlags: return "flags: 0";
        case kSampleErrMode: return "mode: HNB_SAMPLE_NEAREST or HNB_SAMPLE_TRILINEAR";
        case kSampleErrDims: return "dims: every dims[c] >= 1 and their product at most HNB_BIN_MAX_CELLS";
        case kSampleErrOrigin: return "origin is not finite";
        case kSampleErrInvCell: return "inv_cell is not finite and above 0";
        case kSampleErrChannelCount: return "n_channels is not 1..HNB_SAMPLE_MAX_CHANNELS";
        case kSampleErrAttr: return "the channel's attr is not an f32 attribute of 1..4 components of the particle layout other than AGE";
        case kSampleErrComp: return "the channel's comp is at or past the attribute's component count";
        case kSampleErrOp: return "the channel's op: HNB_SAMPLE_SET or HNB_SAMPLE_ADD";
        case kSampleErrChannelReserved: return "the channel's reserved is not 0";
        case kSampleErrDuplicate: return "the channel's (attr, comp) is an earlier channel's";
        case kSampleErrUnusedChannel: return "a channel entry at or past n_channels is not all 0";
        case kSampleErrScale: return "scale is not finite";
        case kSampleErrField: return "field: a 16-byte aligned device pointer";
        case kSampleErrStats: return "out_stats: NULL or a 16-byte aligned device pointer";
        case kSampleErrNoPosition: return "the particle layout has no POSITION of 3 f32 components";
        default: return "?";
    }
}
struct SampleLayoutAttr { uint32_t attr, ncomp, is_f32; };       // what the check is told of the program's layout
struct SampleCheck {
    uint32_t error, channel;        // a SampleDescError and, for a channel's or an axis's, its index
    uint32_t n_cells;
    uint32_t position_index;        // the layout's entry of POSITION
    uint32_t layout_index[HNB_SAMPLE_MAX_CHANNELS];
};
HNB_SORT_KEY_FN bool sample_is_finite(float f) { return f - f == 0.0f; }        // (a NaN or an infinity minus itself is a NaN)
// The refusals of include/hanabi_amd_sample.h "Errors" but the NULL arguments, in the order listed there
HNB_SORT_KEY_FN SampleCheck sample_check_desc(const HnbSampleDesc& d, const SampleLayoutAttr* layout, uint32_t n_layout) {
    SampleCheck c = {};
    const auto fail = [&c](uint32_t e, uint32_t k) { c.error = e; c.channel = k; return c; };
    if (d.struct_size != sizeof(HnbSampleDesc)) return fail(kSampleErrStructSize, 0);
    if (d.flags != 0u) return fail(kSampleErrFlags, 0);
    if (d.mode != HNB_SAMPLE_NEAREST && d.mode != HNB_SAMPLE_TRILINEAR) return fail(kSampleErrMode, 0);
    c.n_cells = bin_cell_count(d.dims);
    if (c.n_cells == 0u) return fail(kSampleErrDims, 0);
    for (uint32_t a = 0; a < 3u; ++a) {
        if (!sample_is_finite(d.origin[a])) return fail(kSampleErrOrigin, a);
        if (!sample_is_finite(d.inv_cell[a]) || !(d.inv_cell[a] > 0.0f)) return fail(kSampleErrInvCell, a);
    }
    if (d.n_channels == 0u || d.n_channels > HNB_SAMPLE_MAX_CHANNELS) return fail(kSampleErrChannelCount, 0);
    for (uint32_t k = 0; k < HNB_SAMPLE_MAX_CHANNELS; ++k) {
        const HnbSampleChannel& ch = d.channels[k];
        if (k >= d.n_channels) {
            if (ch.attr != 0u || ch.comp != 0u || ch.op != 0u || ch.reserved != 0u) return fail(kSampleErrUnusedChannel, k);
            continue;
        }
        uint32_t i = 0;
        while (i < n_layout && layout[i].attr != ch.attr) ++i;
        if (ch.attr == HNB_ATTR_AGE || ch.attr == HNB_ATTR_ID || ch.attr == HNB_ATTR_PARTICLE_COUNTER || ch.attr >= HNB_ATTR_COUNT || i == n_layout || !layout[i].is_f32 ||
            layout[i].ncomp < 1u || layout[i].ncomp > 4u)
            return fail(kSampleErrAttr, k);
        if (ch.comp >= layout[i].ncomp) return fail(kSampleErrComp, k);
        if (ch.op != HNB_SAMPLE_SET && ch.op != HNB_SAMPLE_ADD) return fail(kSampleErrOp, k);
        if (ch.reserved != 0u) return fail(kSampleErrChannelReserved, k);
        for (uint32_t e = 0; e < k; ++e)
            if (d.channels[e].attr == ch.attr && d.channels[e].comp == ch.comp) return fail(kSampleErrDuplicate, k);
        c.layout_index[k] = i;
    }
    if (!sample_is_finite(d.scale)) return fail(kSampleErrScale, 0);
    if (!d.field || ((uintptr_t)d.field & 15u) != 0u) return fail(kSampleErrField, 0);
    if (((uintptr_t)d.out_stats & 15u) != 0u) return fail(kSampleErrStats, 0);
    uint32_t p = 0;
    while (p < n_layout && layout[p].attr != HNB_ATTR_POSITION) ++p;
    if (p == n_layout || !layout[p].is_f32 || layout[p].ncomp != 3u) return fail(kSampleErrNoPosition, 0);
    c.position_index = p;
    return c;
}

// ---- the launch of a call -------------------------------------------------------------------------------------------------------------------------
// The kernels of hnb_sample.hip: the index of a kernel's handle in the context, which is the mode's value
enum SampleKernel : uint32_t { kSampleKNearest, kSampleKTrilinear, kSampleKernelCount };
static_assert(kSampleKNearest == HNB_SAMPLE_NEAREST && kSampleKTrilinear == HNB_SAMPLE_TRILINEAR, "a mode is its kernel's index");
struct SampleKernelName { uint32_t kernel; const char* name; };
constexpr SampleKernelName kSampleKernelNames[kSampleKernelCount] = {{kSampleKNearest, "k_sample_nearest"}, {kSampleKTrilinear, "k_sample_trilinear"}};

struct SamplePlan {
    uint32_t kernel;                // a SampleKernel
    uint32_t grid_x, grid_y;        // workgroups of kSampleBlock lanes: a workgroup per tile
    uint32_t tiles;
    uint64_t clear_stats_bytes;     // what the call zeroes in front when out_stats is given
};
// Decides; hanabi_amd.hip run_sample executes.
HNB_SORT_KEY_FN SamplePlan sample_launch_plan(uint32_t mode, uint32_t capacity) {
    SamplePlan pl = {};
    uint32_t tiles = (uint32_t)(((uint64_t)capacity + kSampleTile - 1u) / kSampleTile);
    if (tiles == 0u) tiles = 1u;
    pl.kernel = mode == HNB_SAMPLE_TRILINEAR ? kSampleKTrilinear : kSampleKNearest;
    pl.grid_x = tiles;
    pl.grid_y = 1u;
    pl.tiles = tiles;
    pl.clear_stats_bytes = 16u;
    return pl;
}

}  // namespace hnb
