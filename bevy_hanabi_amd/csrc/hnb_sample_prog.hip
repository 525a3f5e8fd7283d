// The program form of the sample (hnb_program_sample, include/hanabi_amd_sample_program.h; DESIGN.md "Sample, program form"): hnb_effect_sample
// for every instance of a program in one launch, and the resets behind it in a second. A code object of its own, as hnb_export_filter_prog.hip is
// to hnb_export_filter.hip: the effect form's unit keeps its two kernels, its kernarg and its registers. The tile, the samples and the stores are
// the effect form's text (hnb_sample.hip.h).
//   k_sample_prog_nearest    workgroup (j, i): tile j of instance i; per sampled particle one row of instance i's field
//   k_sample_prog_trilinear  workgroup (j, i): tile j of instance i; per sampled particle the eight corner rows
//   k_sample_prog_reset      workgroup (g, i): words [256 g, 256 g + 256) of what reset_plane_proofs(fx, false) clears of instance i's slab
// A sample workgroup reads its instance's slab base and meta row with scalar loads and leaves when nothing is alive. Its stats: a lane's three
// counters are summed over the wave, the four waves' sums go through 12 words of LDS and one barrier, and lane 0 adds each non-zero number once -
// to the totals and to the instance's row, whichever are given. Every exit in front of the barrier (j >= tiles, i >= n_inst, nothing alive, no
// stats wanted) depends on the arguments, the workgroup's index or the instance's meta row alone: it is taken by the whole workgroup or by none.
// No workgroup waits for another; every loop is bounded by 4, 8 or 12; the reset kernel has none: a lane clears one word.
// Bounds: a slot stored to is below the capacity and a field word read below n_cells * n_channels of the instance's field (hnb_sample.hip.h); a
// stats row is 4 i .. 4 i + 2 with i < n_inst; a reset word lies below lmin_words or horizon_words of its section.
#include <hip/hip_runtime.h>

#include "hnb_sample.hip.h"
#include "hnb_sample_program.h"

#pragma clang fp contract(off)   // (the rule is f32 arithmetic stated operation by operation: hnb_sample.h, hnb_bin_cell.h)

using namespace hnb;

namespace {

// The workgroup's three numbers onto the totals and the instance's row: one add per workgroup, destination and non-zero number. Reached by every
// lane of the workgroup or by none.
__device__ __forceinline__ void add_stats_workgroup(const SampleProgArgs& a, const LaneStats& st, uint32_t inst, uint32_t tid) {
    if (!a.stats && !a.inst_stats) return;                               // (the arguments: the same in every lane)
    __shared__ uint32_t s_part[kSampleProgLdsWords];
    const uint32_t v = wave_sum(st.visited), s = wave_sum(st.sampled), o = wave_sum(st.outside);
    if ((tid & 63u) == 0u) {
        const uint32_t w = tid >> 6;                                     // 0..3: the block is kSampleBlock lanes
        s_part[3u * w] = v; s_part[3u * w + 1u] = s; s_part[3u * w + 2u] = o;
    }
    __syncthreads();
    if (tid != 0u) return;
    uint32_t sum[3] = {0u, 0u, 0u};
#pragma unroll
    for (uint32_t w = 0; w < kSampleBlock / 64u; ++w) {
        sum[0] += s_part[3u * w]; sum[1] += s_part[3u * w + 1u]; sum[2] += s_part[3u * w + 2u];
    }
    uint32_t* row = a.inst_stats ? a.inst_stats + (size_t)inst * 4u : nullptr;
#pragma unroll
    for (uint32_t n = 0; n < 3u; ++n) {
        if (sum[n] == 0u) continue;
        if (a.stats) add_u32(a.stats + n, sum[n]);
        if (row) add_u32(row + n, sum[n]);
    }
}

template <uint32_t MODE>
__device__ __forceinline__ void sample_prog_body(const SampleProgArgs& a) {
    const uint32_t j = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
    if (j >= a.tiles || i >= a.n_inst) return;
    if (a.meta[i].alive_count == 0u) return;                             // nothing alive: no slot is read, nothing is written, nothing is added
    char* base = reinterpret_cast<char*>(a.slabs[i]);
    const float* field = a.field + sample_program_field_offset(i, a.field_stride);
    LaneStats st = {0u, 0u, 0u};
    sample_tile_by_channels<MODE>(a, base, field, j * kSampleTile, tid, st);
    add_stats_workgroup(a, st, i, tid);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_sample_prog_nearest(const SampleProgArgs a) { sample_prog_body<HNB_SAMPLE_NEAREST>(a); }

extern "C" __global__ void __launch_bounds__(256) k_sample_prog_trilinear(const SampleProgArgs a) { sample_prog_body<HNB_SAMPLE_TRILINEAR>(a); }

// The device side of reset_plane_proofs(fx, false) for every instance, whether anything of it was sampled or not: zero = "no bound published" for
// the chunks' lifetime bounds, zero = "may die now" for the death horizons. Plain 4-byte stores.
extern "C" __global__ void __launch_bounds__(256) k_sample_prog_reset(const SampleProgArgs a) {
    const uint32_t i = blockIdx.y;
    if (i >= a.n_inst) return;
    const uint64_t w = (uint64_t)blockIdx.x * kSampleProgResetBlock + threadIdx.x;
    char* base = reinterpret_cast<char*>(a.slabs[i]);
    if (w < a.lmin_words) {
        reinterpret_cast<uint32_t*>(base + a.lmin_off)[w] = 0u;
    } else if (w - a.lmin_words < a.horizon_words) {
        reinterpret_cast<uint32_t*>(base + a.horizon_off)[w - a.lmin_words] = 0u;
    }
}
