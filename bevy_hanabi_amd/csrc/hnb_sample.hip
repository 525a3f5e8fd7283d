// The sample (hnb_effect_sample, include/hanabi_amd_sample.h; DESIGN.md "Sample"): for every alive particle of one instance whose POSITION lies inside
// the uniform grid, up to four channels of an f32 field - the value of its cell or the trilinear blend of the eight cell centres around it - scaled
// and stored or added into one component of an f32 attribute each. A code object of its own, like the deposit's: nothing here is part of the fat
// binary of libhanabi_amd.so. The walk of a tile, the samples of a particle and the stores of a channel are hnb_sample.hip.h's, shared with the program
// form's unit (hnb_sample_prog.hip): the bounds argued there hold for the slab and the field of the one instance here.
//   k_sample_nearest    workgroup j: tile j; per sampled particle one field row
//   k_sample_trilinear  workgroup j: tile j; per sampled particle the eight corner rows, computed once and shared by the channels
// The grid is ceil(capacity / 4096); no workgroup waits for another; an instance with nothing alive leaves after the scalar loads.
#include <hip/hip_runtime.h>

#include "hnb_sample.h"
#include "hnb_sample.hip.h"

#pragma clang fp contract(off)   // (the rule is f32 arithmetic stated operation by operation: hnb_sample.h, hnb_bin_cell.h)

using namespace hnb;

namespace {

// A wave's three numbers onto out_stats: one add per wave and non-zero number
__device__ __forceinline__ void add_stats(const SampleArgs& a, const LaneStats& st, uint32_t tid) {
    if (!a.stats) return;
    const uint32_t v = wave_sum(st.visited), s = wave_sum(st.sampled), o = wave_sum(st.outside);
    if ((tid & 63u) == 0u) {
        if (v != 0u) add_u32(a.stats, v);
        if (s != 0u) add_u32(a.stats + 1, s);
        if (o != 0u) add_u32(a.stats + 2, o);
    }
}

template <uint32_t MODE>
__device__ __forceinline__ void sample_body(const SampleArgs& a) {
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    if (j >= a.tiles) return;
    if (a.meta->alive_count == 0u) return;                               // nothing alive: no slot is read, nothing is written
    char* base = reinterpret_cast<char*>(a.slab[0]);
    LaneStats st = {0u, 0u, 0u};
    sample_tile_by_channels<MODE>(a, base, a.field, j * kSampleTile, tid, st);
    add_stats(a, st, tid);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_sample_nearest(const SampleArgs a) { sample_body<HNB_SAMPLE_NEAREST>(a); }

extern "C" __global__ void __launch_bounds__(256) k_sample_trilinear(const SampleArgs a) { sample_body<HNB_SAMPLE_TRILINEAR>(a); }
