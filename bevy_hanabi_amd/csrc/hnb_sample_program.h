// The program form of the sample (hnb_program_sample; include/hanabi_amd_sample_program.h), shared by the kernels' translation unit
// (hnb_sample_prog.hip: a code object of its own) and the runtime that loads and launches them (hanabi_amd.hip run_program_sample): the check of the
// outer description (sample_program_check_desc), the kernels' argument block (SampleProgArgs), the field of an instance, the byte ranges the reset
// kernel clears, the kernels by name (SampleProgKernel) and the launches of a call (sample_program_launch_plan). The rule, the inner description's
// check and the tile are the effect form's (hnb_sample.h): none is restated here. Plain C++: a host compiler takes it, so the tests check the
// refusals, the plan and the 64-bit field offset without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd_sample_program.h"
#include "hnb_sample.h"
#include "hnb_sort_key.h"

namespace hnb {

constexpr uint32_t kSampleProgMaxInstances = HNB_PROGRAM_SAMPLE_MAX_INSTANCES;      // a launch's grid along y
constexpr uint32_t kSampleProgResetBlock = 256;     // lanes per workgroup of the reset kernel, a 4-byte word each
constexpr uint32_t kSampleProgLdsWords = 12;        // the stats of a workgroup's four waves, three numbers each: 48 bytes of LDS
static_assert(sizeof(HnbProgramSampleDesc) == 168, "HnbProgramSampleDesc layout");

// ---- the check of a description -------------------------------------------------------------------------------------------------------------------
enum SampleProgDescError : uint32_t {
    kSampleProgOk, kSampleProgErrStructSize, kSampleProgErrFlags, kSampleProgErrReserved, kSampleProgErrInner, kSampleProgErrStride, kSampleProgErrInstanceStats,
    kSampleProgErrInstances, kSampleProgDescErrorCount
};
HNB_SORT_KEY_FN const char* sample_program_error_text(uint32_t e) {
    switch (e) {
        case kSampleProgOk: return "ok";
        case kSampleProgErrStructSize: return "struct_size is not this library's sizeof(HnbProgramSampleDesc)";
        case kSampleProgErrFlags: return "flags: 0";
        case kSampleProgErrReserved: return "reserved is not 0";
        case kSampleProgErrInner: return "sample: refused as hnb_effect_sample refuses it";
        case kSampleProgErrStride: return "field_instance_stride: 0, or a multiple of 4 that is at least n_cells * n_channels";
        case kSampleProgErrInstanceStats: return "out_instance_stats: NULL or a 16-byte aligned device pointer";
        case kSampleProgErrInstances: return "the program's instance count is not 1..HNB_PROGRAM_SAMPLE_MAX_INSTANCES";
        default: return "?";
    }
}
struct SampleProgCheck {
    uint32_t error;                 // a SampleProgDescError; kSampleProgErrInner: inner.error says which
    SampleCheck inner;              // sample_check_desc of desc.sample (filled from kSampleProgErrInner on)
};
// The refusals of include/hanabi_amd_sample_program.h "Errors" but the NULL arguments, in the order listed there
HNB_SORT_KEY_FN SampleProgCheck sample_program_check_desc(const HnbProgramSampleDesc& d, const SampleLayoutAttr* layout, uint32_t n_layout, uint32_t n_inst) {
    SampleProgCheck c = {};
    const auto fail = [&c](uint32_t e) { c.error = e; return c; };
    if (d.struct_size != sizeof(HnbProgramSampleDesc)) return fail(kSampleProgErrStructSize);
    if (d.flags != 0u) return fail(kSampleProgErrFlags);
    if (d.reserved != 0u) return fail(kSampleProgErrReserved);
    c.inner = sample_check_desc(d.sample, layout, n_layout);
    if (c.inner.error != kSampleOk) return fail(kSampleProgErrInner);
    const uint64_t row_words = (uint64_t)c.inner.n_cells * d.sample.n_channels;      // (at most 2^24 * 4)
    if (d.field_instance_stride != 0u && ((d.field_instance_stride & 3u) != 0u || d.field_instance_stride < row_words)) return fail(kSampleProgErrStride);
    if (((uintptr_t)d.out_instance_stats & 15u) != 0u) return fail(kSampleProgErrInstanceStats);
    if (n_inst == 0u || n_inst > kSampleProgMaxInstances) return fail(kSampleProgErrInstances);
    return c;
}

// ---- the kernels' argument block ------------------------------------------------------------------------------------------------------------------
// The members sample_tile reads (hnb_sample.hip.h) are named as SampleArgs names them.
struct SampleProgArgs {
    const uint64_t* slabs;          // the program's table of slab base addresses, a row per instance
    const HnbDeviceMeta* meta;      // the instances' rows after the frames enqueued so far
    const float* field;             // instance 0's: [n_cells * n_channels]
    uint64_t field_stride;          // f32 elements from an instance's field to the next one's; 0: one field for all
    uint32_t* stats;                // [4]: the totals, or NULL
    uint32_t* inst_stats;           // [n_inst][4], or NULL
    uint64_t pos_off;               // bytes from the slab base: POSITION, 12 bytes per slot
    uint64_t flag_off;              //   ... and the alive bytes, one per slot
    uint64_t lmin_off, horizon_off; // k_sample_prog_reset: the sections it clears from, bytes from the slab base, 4-byte aligned
    uint32_t lmin_words, horizon_words;     //   ... and how much of each, in 4-byte words (sample_program_reset_ranges); horizon_words 0: none
    BinGrid grid;
    uint32_t capacity, tiles;       // tiles of kSampleTile slots
    uint32_t n_channels;
    float scale;
    uint32_t n_inst, pad;
    SampleChannelArg ch[HNB_SAMPLE_MAX_CHANNELS];
};
static_assert(sizeof(SampleProgArgs) == 216, "one SampleProgArgs by value");

// Instance i's field, in f32 elements from instance 0's: the product in 64 bits (65,534 * 2^26 is past 2^32)
HNB_SORT_KEY_FN uint64_t sample_program_field_offset(uint32_t i, uint64_t stride) { return (uint64_t)i * stride; }

// What reset_plane_proofs(fx, false) clears of an instance's slab (hanabi_amd.hip), in bytes: the chunks' lifetime bounds - chunks_per_inst words
// at lmin_off; the "completely alive" flags behind them stay - and, for a program whose death horizons are kept, the horizon section: 256 bytes
// and 24 per chunk at horizon_off.
struct SampleProgResetRanges { uint64_t lmin_bytes, horizon_bytes; };
HNB_SORT_KEY_FN SampleProgResetRanges sample_program_reset_ranges(uint32_t chunks_per_inst, bool horizon_eligible) {
    SampleProgResetRanges r;
    r.lmin_bytes = (uint64_t)chunks_per_inst * 4u;
    r.horizon_bytes = horizon_eligible ? 256u + (uint64_t)chunks_per_inst * 24u : 0u;
    return r;
}

// ---- the launches of a call -----------------------------------------------------------------------------------------------------------------------
// The kernels of hnb_sample_prog.hip: the index of a kernel's handle in the context. Numbered apart from SampleKernel.
enum SampleProgKernel : uint32_t { kSampleProgKNearest, kSampleProgKTrilinear, kSampleProgKReset, kSampleProgKernelCount };
struct SampleProgKernelName { uint32_t kernel; const char* name; };
constexpr SampleProgKernelName kSampleProgKernelNames[kSampleProgKernelCount] = {
    {kSampleProgKNearest, "k_sample_prog_nearest"}, {kSampleProgKTrilinear, "k_sample_prog_trilinear"}, {kSampleProgKReset, "k_sample_prog_reset"}};

struct SampleProgPlan {
    uint32_t kernel;                // kSampleProgKNearest or kSampleProgKTrilinear
    uint32_t grid_x, grid_y;        // workgroups of kSampleBlock lanes: (tiles, instances)
    uint32_t tiles;
    uint32_t reset_grid_x, reset_grid_y;    // k_sample_prog_reset: workgroups of kSampleProgResetBlock lanes, (ceil(words / 256), instances)
    uint32_t lmin_words, horizon_words;     // the words of an instance it clears
    uint64_t clear_stats_bytes, clear_instance_stats_bytes;    // what the call zeroes in front when the buffer is given
};
// Decides; hanabi_amd.hip run_program_sample executes. n_inst is 1..kSampleProgMaxInstances (sample_program_check_desc). The reset ranges are
// sample_program_reset_ranges': multiples of 4, and their words fit 32 bits (at most 28 bytes per chunk of a capacity below 2^32).
HNB_SORT_KEY_FN SampleProgPlan sample_program_launch_plan(uint32_t mode, uint32_t n_inst, uint32_t capacity, uint64_t lmin_bytes, uint64_t horizon_bytes) {
    SampleProgPlan pl = {};
    const SamplePlan one = sample_launch_plan(mode, capacity);           // the effect form's tiles
    pl.kernel = mode == HNB_SAMPLE_TRILINEAR ? kSampleProgKTrilinear : kSampleProgKNearest;
    pl.tiles = one.tiles;
    pl.grid_x = one.tiles;
    pl.grid_y = n_inst;
    pl.lmin_words = (uint32_t)(lmin_bytes / 4u);
    pl.horizon_words = (uint32_t)(horizon_bytes / 4u);
    const uint64_t words = (uint64_t)pl.lmin_words + pl.horizon_words;
    pl.reset_grid_x = (uint32_t)((words + kSampleProgResetBlock - 1u) / kSampleProgResetBlock);
    if (pl.reset_grid_x == 0u) pl.reset_grid_x = 1u;
    pl.reset_grid_y = n_inst;
    pl.clear_stats_bytes = one.clear_stats_bytes;
    pl.clear_instance_stats_bytes = (uint64_t)n_inst * 16u;
    return pl;
}

}  // namespace hnb
