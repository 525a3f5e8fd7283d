// Particle bounds (hnb_effect_bounds, hnb_program_bounds; include/hanabi_amd.h "Bounds"), shared by the kernels' translation unit (hnb_bounds.hip: a
// code object of its own) and the runtime that loads and launches them (hanabi_amd.hip): the fold rule, the partial a tile leaves and the record a
// call writes, the kernels' argument block, the scratch layout, the kernels by name (BoundsKernel) and the launches of a call (bounds_launch_plan).
// Plain C++: a host compiler takes it, so the tests check the fold, the layout and the plan without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd.h"
#include "hnb_sort_key.h"

namespace hnb {

constexpr uint32_t kBoundsBlock = 256;         // lanes per workgroup
constexpr uint32_t kBoundsTile = 4096;         // slots per workgroup of k_bounds_tile: four quads of consecutive slots per lane
constexpr uint32_t kBoundsMaxInstances = 65535;

// ---- the fold rule --------------------------------------------------------------------------------------------------------------------------------
// Everything is folded in KEY space (sort_key_f32: an unsigned order with -inf < ... < -0 < +0 < ... < +inf and the NaNs outside on both sides) with
// integer min / max, which are associative and commutative: any grouping of the particles into lanes, waves, tiles and instances gives the same bits.
// The identities are the keys of +inf (for lo) and -inf (for hi): a NaN or a dead slot contributes them, and a component nobody contributed to comes
// out as (+inf, -inf).
constexpr uint32_t kBoundsEmptyLoKey = 0xFF800000u;    // sort_key_f32(+inf): no key of a value that is not a NaN lies above it
constexpr uint32_t kBoundsEmptyHiKey = 0x007FFFFFu;    // sort_key_f32(-inf): ... nor below it

HNB_SORT_KEY_FN bool bounds_is_nan(uint32_t bits) { return (bits & 0x7FFFFFFFu) > 0x7F800000u; }
// the value a key came from
HNB_SORT_KEY_FN uint32_t bounds_value_of_key(uint32_t k) { return (k >> 31) ? k ^ 0x80000000u : ~k; }
HNB_SORT_KEY_FN uint32_t bounds_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
HNB_SORT_KEY_FN uint32_t bounds_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

struct BoundsPartial {              // what a lane, a wave, a tile or an instance has seen: 64 bytes, one per (instance, tile) in the scratch
    uint32_t lo[4], hi[4];          // keys; components at and past ncomp stay empty
    uint32_t alive, nan;
    uint32_t pad[6];                // written as 0
};
static_assert(sizeof(BoundsPartial) == 64, "a partial is 64 bytes");
static_assert(sizeof(HnbBounds) == 48 && sizeof(HnbBoundsDesc) == 32, "HnbBounds / HnbBoundsDesc layout");

HNB_SORT_KEY_FN BoundsPartial bounds_empty() {
    BoundsPartial p = {};
    for (int c = 0; c < 4; ++c) { p.lo[c] = kBoundsEmptyLoKey; p.hi[c] = kBoundsEmptyHiKey; }
    return p;
}
// One slot: `bits` are its ncomp stored components, `alive` its alive byte != 0. A NaN component is skipped for that component only; the particle is
// counted once in `nan` whatever the number of its NaN components.
HNB_SORT_KEY_FN void bounds_fold_slot(BoundsPartial& p, const uint32_t* bits, uint32_t ncomp, bool alive) {
    bool any_nan = false;
    for (uint32_t c = 0; c < ncomp; ++c) {
        const bool is_nan = bounds_is_nan(bits[c]), use = alive && !is_nan;
        const uint32_t k = sort_key_f32(bits[c]);
        p.lo[c] = bounds_min(p.lo[c], use ? k : kBoundsEmptyLoKey);
        p.hi[c] = bounds_max(p.hi[c], use ? k : kBoundsEmptyHiKey);
        any_nan = any_nan || is_nan;
    }
    p.alive += alive ? 1u : 0u;
    p.nan += alive && any_nan ? 1u : 0u;
}
// Two partials into one (lanes into a wave, waves into a tile, tiles into an instance)
HNB_SORT_KEY_FN void bounds_merge(BoundsPartial& p, const BoundsPartial& q) {
    for (int c = 0; c < 4; ++c) { p.lo[c] = bounds_min(p.lo[c], q.lo[c]); p.hi[c] = bounds_max(p.hi[c], q.hi[c]); }
    p.alive += q.alive;
    p.nan += q.nan;
}
// Word w (0..11) of the HnbBounds record of a partial: keys back into values for the components the attribute has, bits 0 for the others
HNB_SORT_KEY_FN uint32_t bounds_record_word(uint32_t w, uint32_t folded, uint32_t ncomp) {
    if (w < 8u) return (w & 3u) < ncomp ? bounds_value_of_key(folded) : 0u;
    return w < 10u ? folded : 0u;
}
HNB_SORT_KEY_FN HnbBounds bounds_record(const BoundsPartial& p, uint32_t ncomp) {
    HnbBounds r;
    uint32_t w[12];
    for (uint32_t i = 0; i < 12u; ++i) w[i] = bounds_record_word(i, i < 4u ? p.lo[i] : i < 8u ? p.hi[i - 4u] : i == 8u ? p.alive : i == 9u ? p.nan : 0u, ncomp);
    uint32_t* out = reinterpret_cast<uint32_t*>(&r);
    for (uint32_t i = 0; i < 12u; ++i) out[i] = w[i];
    return r;
}
// A record into a partial: the union of a program's instances folds their records by the same rule (a record's lo / hi are never NaNs, and an
// instance nobody contributed to holds the identities' values); alive and nan are summed modulo 2^32
HNB_SORT_KEY_FN void bounds_fold_record(BoundsPartial& p, const uint32_t* rec /* [12] */, uint32_t ncomp) {
    for (uint32_t c = 0; c < ncomp; ++c) {
        p.lo[c] = bounds_min(p.lo[c], sort_key_f32(rec[c]));
        p.hi[c] = bounds_max(p.hi[c], sort_key_f32(rec[4u + c]));
    }
    p.alive += rec[8];
    p.nan += rec[9];
}


// ---- the kernels' argument block ------------------------------------------------------------------------------------------------------------------
struct BoundsArgs {
    const uint64_t* slabs;          // [n_inst] slab base addresses (the effect form: the one row of the program's table)
    const HnbDeviceMeta* meta;      // [n_inst] rows after the frames enqueued so far
    BoundsPartial* partials;        // the scratch: instance k's tiles at k * pitch_bytes; NULL for instances of one tile (k_bounds_small)
    uint32_t* dst;                  // HnbBounds records, 16-byte aligned: [n_inst] and, program form, the union behind them
    uint64_t plane_off;             // bytes from the slab base: the attribute's plane, ncomp * 4 bytes per slot
    uint64_t flag_off;              //   ... and the alive bytes, one per slot
    uint64_t pitch_bytes;           // bytes between two instances' sections of the scratch
    uint32_t capacity, tiles, ncomp, n_inst;
};


// ---- the scratch ----------------------------------------------------------------------------------------------------------------------------------
// One allocation per effect and per program: 64 bytes per tile of 4096 slots and instance, every instance's section on a 256-byte boundary, offsets
// in 64 bits (65,535 instances of 2^32 - 1 slots are 2^42 bytes). Instances of one tile need none: total == 0.
struct BoundsScratch { uint32_t n_inst, tiles; uint64_t pitch_bytes, total; };
HNB_SORT_KEY_FN BoundsScratch bounds_scratch_layout(uint32_t n_inst, uint32_t capacity) {
    BoundsScratch l;
    l.n_inst = n_inst;
    l.tiles = (uint32_t)(((uint64_t)capacity + kBoundsTile - 1u) / kBoundsTile);
    l.pitch_bytes = l.tiles <= 1u ? 0u : ((uint64_t)l.tiles * sizeof(BoundsPartial) + 255u) & ~(uint64_t)255u;
    l.total = (uint64_t)n_inst * l.pitch_bytes;
    return l;
}
HNB_SORT_KEY_FN uint64_t bounds_partial_offset(const BoundsScratch& l, uint32_t instance, uint32_t tile) {
    return (uint64_t)instance * l.pitch_bytes + (uint64_t)tile * sizeof(BoundsPartial);
}


// ---- the launches of a call -----------------------------------------------------------------------------------------------------------------------
// The kernels of hnb_bounds.hip: the index of a kernel's handle in the context. Numbered apart from the exports' (hnb_export.h ExportKernel).
enum BoundsKernel : uint32_t { kBoundsKTile, kBoundsKFinish, kBoundsKUnion, kBoundsKSmall, kBoundsKernelCount };
struct BoundsLaunch { uint32_t kernel, grid_x, grid_y; };   // (workgroups of kBoundsBlock lanes; every kernel takes one BoundsArgs by value)
constexpr uint32_t kBoundsPlanMax = 3;
struct BoundsPlan { uint32_t n; BoundsLaunch launch[kBoundsPlanMax]; };

// `program`: all n_inst instances and the union record behind them, else one effect (n_inst is not read). Up to 4096 slots one workgroup per instance
// and no scratch: one launch, two with the union; above, tiles and a fold of the tiles: two and three. Decides; hanabi_amd.hip run_bounds executes.
HNB_SORT_KEY_FN BoundsPlan bounds_launch_plan(bool program, uint32_t n_inst, uint32_t capacity) {
    BoundsPlan pl = {};
    const uint32_t n = program ? n_inst : 1u;
    const uint32_t tiles = (uint32_t)(((uint64_t)capacity + kBoundsTile - 1u) / kBoundsTile);
    if (tiles <= 1u) pl.launch[pl.n++] = BoundsLaunch{kBoundsKSmall, 1u, n};
    else {
        pl.launch[pl.n++] = BoundsLaunch{kBoundsKTile, tiles, n};
        pl.launch[pl.n++] = BoundsLaunch{kBoundsKFinish, 1u, n};
    }
    if (program) pl.launch[pl.n++] = BoundsLaunch{kBoundsKUnion, 1u, 1u};
    return pl;
}

}  // namespace hnb
