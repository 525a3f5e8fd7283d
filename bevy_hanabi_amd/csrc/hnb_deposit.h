// The deposit (hnb_effect_deposit, hnb_program_deposit; include/hanabi_amd_deposit.h), shared by the kernels' translation unit (hnb_deposit.hip: a
// code object of its own) and the runtime that loads and launches them (hanabi_amd.hip): the quantisation of a stored f32 into a fixed-point
// contribution, the kernels' argument block, the kernels by name (DepositKernel), the check of a description (deposit_check_desc) and the launch of a
// call (deposit_launch_plan). Plain C++: a host compiler takes it, so the tests check the quantisation, the refusals and the plan without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd_deposit.h"
#include "hnb_bin_cell.h"
#include "hnb_sort_key.h"

namespace hnb {

constexpr uint32_t kDepositBlock = 256;             // lanes per workgroup
constexpr uint32_t kDepositTile = 4096;             // slots per tile: four quads of consecutive slots per lane (the bounds' walk)
constexpr uint32_t kDepositMaxInstances = 65535;
constexpr uint32_t kDepositMaxFracBits = 32;
// The LDS a workgroup of k_deposit_lds may hold its private table in: 48 KiB, so that two workgroups (three) fit the 160 KiB of a CU. Grids of up to
// 12,287 cells without a channel, 4,095 with one and 1,364 with four have their table there: 8^3 with four channels takes 18,468 bytes.
constexpr uint32_t kDepositLdsBudget = 48u * 1024u;
// Bytes of table per tile of span (deposit_launch_plan; DESIGN.md "Deposit", the span rule)
constexpr uint32_t kDepositSpanBytes = 2048;

// ---- the quantisation -----------------------------------------------------------------------------------------------------------------------------
// q = v * 2^frac_bits rounded to the nearest integer, ties to even, as a function of the 32 stored bits in integer arithmetic alone. With E the
// exponent field and F the fraction: v = (-1)^sign * m * 2^e with m = F, e = -149 (E = 0: zeros and denormals) or m = 2^23 + F, e = E - 150; so
// v * 2^frac_bits = m * 2^sh with sh = e + frac_bits in [-149, 136]. sh >= 0: the value is the integer m << sh, rejected when it is at or above
// 2^62 (m < 2^24: never for sh <= 38, always for sh >= 62 unless m = 0). sh < 0: the quotient m >> s, s = -sh, and the remainder against the half
// 2^(s-1); s > 25 leaves less than a half: 0. E = 255 (an infinity or a NaN) is rejected.
struct DepositQuant { bool ok; int64_t q; };
HNB_SORT_KEY_FN DepositQuant deposit_quantise(uint32_t bits, uint32_t frac_bits) {
    // straight-line: every shift count is clamped into its type's width, so that no path is undefined and a GPU lane takes no branch
    const uint32_t E = (bits >> 23) & 0xFFu, F = bits & 0x7FFFFFu;
    const uint32_t m = E == 0u ? F : (F | 0x800000u);
    const int32_t sh = (E == 0u ? -149 : (int32_t)E - 150) + (int32_t)frac_bits;
    // sh >= 0: m << sh, at or above 2^62 iff sh >= 62 or m has a bit at or above 62 - sh (m < 2^24: none for sh < 31, where the count is held at 31)
    const uint32_t up = sh < 0 ? 0u : sh > 61 ? 61u : (uint32_t)sh;
    const uint32_t top = sh < 31 ? 31u : sh > 61 ? 1u : (uint32_t)(62 - sh);
    const bool too_big = sh >= 0 && m != 0u && (sh >= 62 || (m >> top) != 0u);
    const uint64_t shifted = (uint64_t)m << up;
    // sh < 0: m >> s with s = -sh, held at 26 (m < 2^24 is below a quarter of 2^26: quotient 0, remainder below the half), ties to even
    const uint32_t s = sh >= 0 ? 1u : sh < -26 ? 26u : (uint32_t)(-sh);
    const uint32_t quo = m >> s, rem = m & ((1u << s) - 1u), half = 1u << (s - 1u);
    const uint64_t rounded = (uint64_t)quo + ((rem > half || (rem == half && (quo & 1u) != 0u)) ? 1u : 0u);
    const uint64_t mag = sh >= 0 ? shifted : rounded;         // below 2^62 where the contribution is accepted
    DepositQuant r;
    r.ok = E != 255u && !too_big;
    r.q = r.ok ? ((bits >> 31) ? (int64_t)(0u - mag) : (int64_t)mag) : 0;
    return r;
}

// ---- the kernels' argument block ------------------------------------------------------------------------------------------------------------------
struct DepositChannelArg {
    uint64_t plane_off;             // bytes from the slab base: the attribute's plane, ncomp * 4 bytes per slot
    uint32_t packed;                // ncomp | comp << 8 | frac_bits << 16 (deposit_pack_channel): one scalar register
    uint32_t pad;
};
HNB_SORT_KEY_FN uint32_t deposit_pack_channel(uint32_t ncomp, uint32_t comp, uint32_t frac_bits) { return ncomp | (comp << 8) | (frac_bits << 16); }
HNB_SORT_KEY_FN uint32_t deposit_channel_ncomp(uint32_t packed) { return packed & 0xFFu; }
HNB_SORT_KEY_FN uint32_t deposit_channel_comp(uint32_t packed) { return (packed >> 8) & 0xFFu; }
HNB_SORT_KEY_FN uint32_t deposit_channel_frac_bits(uint32_t packed) { return packed >> 16; }
struct DepositArgs {
    const uint64_t* slabs;          // [n_inst] slab base addresses (the effect form: the one row of the program's table)
    const HnbDeviceMeta* meta;      // [n_inst] rows after the frames enqueued so far
    uint32_t* count;                // [n_cells + 1]
    uint64_t* sums;                 // [(n_cells + 1) * n_channels]: two's-complement sums, added as unsigned
    uint32_t* stats;                // [4] or NULL
    uint64_t pos_off;               // bytes from the slab base: POSITION, 12 bytes per slot
    uint64_t flag_off;              //   ... and the alive bytes, one per slot
    BinGrid grid;
    uint32_t capacity, tiles;       // tiles of kDepositTile slots per instance
    uint32_t span, groups;          // k_deposit_lds: tiles per workgroup and workgroups per instance (k_deposit_global: 1, tiles)
    uint32_t n_inst, n_channels;
    DepositChannelArg ch[HNB_DEPOSIT_MAX_CHANNELS];
};
static_assert(sizeof(HnbDepositChannel) == 16 && sizeof(HnbDepositDesc) == 136, "HnbDepositChannel / HnbDepositDesc layout");
static_assert(sizeof(DepositArgs) == 184, "one DepositArgs by value");

// ---- the check of a description -------------------------------------------------------------------------------------------------------------------
enum DepositDescError : uint32_t {
    kDepositOk, kDepositErrStructSize, kDepositErrFlags, kDepositErrDims, kDepositErrOrigin, kDepositErrInvCell, kDepositErrChannelCount, kDepositErrAttr, kDepositErrComp,
    kDepositErrFracBits, kDepositErrChannelReserved, kDepositErrUnusedChannel, kDepositErrCount, kDepositErrSums, kDepositErrStats, kDepositErrNoPosition, kDepositDescErrorCount
};
HNB_SORT_KEY_FN const char* deposit_error_text(uint32_t e) {
    switch (e) {
        case kDepositOk: return "ok";
        case kDepositErrStructSize: return "struct_size is not this library's sizeof(HnbDepositDesc)";
        case kDepositErrFlags: return "flags: 0 or HNB_DEPOSIT_ACCUMULATE";
        case kDepositErrDims: return "dims: every dims[c] >= 1 and their product at most HNB_BIN_MAX_CELLS";
        case kDepositErrOrigin: return "origin is not finite";
        case kDepositErrInvCell: return "inv_cell is not finite and above 0";
        case kDepositErrChannelCount: return "n_channels is above HNB_DEPOSIT_MAX_CHANNELS";
        case kDepositErrAttr: return "the channel's attr is not an f32 attribute of 1..4 components of the particle layout";
        case kDepositErrComp: return "the channel's comp is at or past the attribute's component count";
        case kDepositErrFracBits: return "the channel's frac_bits is above 32";
        case kDepositErrChannelReserved: return "the channel's reserved is not 0";
        case kDepositErrUnusedChannel: return "a channel entry at or past n_channels is not all 0";
        case kDepositErrCount: return "count: a 16-byte aligned device pointer";
        case kDepositErrSums: return "sums: a 16-byte aligned device pointer with channels, NULL without";
        case kDepositErrStats: return "out_stats: NULL or a 16-byte aligned device pointer";
        case kDepositErrNoPosition: return "the particle layout has no POSITION of 3 f32 components";
        default: return "?";
    }
}
struct DepositLayoutAttr { uint32_t attr, ncomp, is_f32; };      // what the check is told of the program's layout
struct DepositCheck {
    uint32_t error, channel;        // a DepositDescError and, for a channel's, its index
    uint32_t n_cells;
    uint32_t position_index;        // the layout's entry of POSITION
    uint32_t layout_index[HNB_DEPOSIT_MAX_CHANNELS];
    bool has_age;                   // a channel reads AGE: stale ages are materialised first
};
HNB_SORT_KEY_FN bool deposit_is_finite(float f) { return f - f == 0.0f; }       // (a NaN or an infinity minus itself is a NaN)
// The refusals of include/hanabi_amd_deposit.h "Errors" but the NULL arguments and the program's instance count, in the order listed there
HNB_SORT_KEY_FN DepositCheck deposit_check_desc(const HnbDepositDesc& d, const DepositLayoutAttr* layout, uint32_t n_layout) {
    DepositCheck c = {};
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
        uint32_t i = 0;
        while (i < n_layout && layout[i].attr != ch.attr) ++i;
        if (ch.attr == HNB_ATTR_ID || ch.attr == HNB_ATTR_PARTICLE_COUNTER || ch.attr >= HNB_ATTR_COUNT || i == n_layout || !layout[i].is_f32 || layout[i].ncomp < 1u ||
            layout[i].ncomp > 4u)
            return fail(kDepositErrAttr, k);
        if (ch.comp >= layout[i].ncomp) return fail(kDepositErrComp, k);
        if (ch.frac_bits > kDepositMaxFracBits) return fail(kDepositErrFracBits, k);
        if (ch.reserved != 0u) return fail(kDepositErrChannelReserved, k);
        c.layout_index[k] = i;
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
// The kernels of hnb_deposit.hip: the index of a kernel's handle in the context. Numbered apart from the exports' and the bounds'.
enum DepositKernel : uint32_t { kDepositKLds, kDepositKGlobal, kDepositKernelCount };
struct DepositKernelName { uint32_t kernel; const char* name; };
constexpr DepositKernelName kDepositKernelNames[kDepositKernelCount] = {{kDepositKLds, "k_deposit_lds"}, {kDepositKGlobal, "k_deposit_global"}};

HNB_SORT_KEY_FN uint64_t deposit_table_bytes(uint32_t n_cells, uint32_t n_channels) { return ((uint64_t)n_cells + 1u) * (4u + 8u * n_channels); }   // (below 2^30)

struct DepositPlan {
    uint32_t kernel;                // a DepositKernel
    uint32_t grid_x, grid_y;        // workgroups of kDepositBlock lanes: groups per instance x instances
    uint32_t span;                  // tiles per workgroup
    uint32_t lds_bytes;             // k_deposit_lds: the workgroup's table (dynamic LDS); 0 for k_deposit_global
    uint64_t clear_count_bytes, clear_sums_bytes, clear_stats_bytes;   // what a call without HNB_DEPOSIT_ACCUMULATE zeroes in front (stats: when given)
};
// `program`: all n_inst instances, else one effect (n_inst is not read). A table within kDepositLdsBudget: k_deposit_lds, a workgroup per span of
// ceil(table / kDepositSpanBytes) tiles, so that the flush's atomics stay a small fraction of the span's own plane traffic; else k_deposit_global, a
// workgroup per tile. Decides; hanabi_amd.hip run_deposit executes.
HNB_SORT_KEY_FN DepositPlan deposit_launch_plan(bool program, uint32_t n_inst, uint32_t capacity, uint32_t n_cells, uint32_t n_channels) {
    DepositPlan pl = {};
    const uint64_t table = deposit_table_bytes(n_cells, n_channels);
    uint32_t tiles = (uint32_t)(((uint64_t)capacity + kDepositTile - 1u) / kDepositTile);
    if (tiles == 0u) tiles = 1u;
    pl.grid_y = program ? n_inst : 1u;
    if (table <= kDepositLdsBudget) {
        pl.kernel = kDepositKLds;
        pl.span = (uint32_t)((table + kDepositSpanBytes - 1u) / kDepositSpanBytes);      // 1..24
        pl.grid_x = (tiles + pl.span - 1u) / pl.span;
        pl.lds_bytes = (uint32_t)table;
    } else {
        pl.kernel = kDepositKGlobal;
        pl.span = 1u;
        pl.grid_x = tiles;
    }
    pl.clear_count_bytes = ((uint64_t)n_cells + 1u) * 4u;
    pl.clear_sums_bytes = ((uint64_t)n_cells + 1u) * 8u * n_channels;
    pl.clear_stats_bytes = 16u;
    return pl;
}

}  // namespace hnb
