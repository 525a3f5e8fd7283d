// Binned export (hnb_effect_export_binned, include/hanabi_amd_binned.h; DESIGN.md "Binned export"): the alive particles of ONE effect as
// packed records in the order of the cell of a uniform 3-D grid that holds their POSITION, and a table that says where every cell's records start.
// A code object of its own, like the six before it: nothing here is part of the fat binary of libhanabi_amd.so. Only what is new lives here; the
// rest of a call is k_export_sort_hist, k_export_sort_scatter and the gather k_export_sort_rows_* of hnb_export_sort.hip, unchanged, and the tile
// primitives below are theirs (hnb_export_sort.hip.h).
//   k_export_bin_keys    above 4096 slots: the sorted export's keys kernel with the cell (hnb_bin_cell.h) as the key - (cell, slot) of every list
//                        row into (keys[0], vals[0]), the tile's counts of all four digits into hist and gsum set 0, the OR words. Cells below 2^16
//                        leave the upper two digits equal in every key: those passes return at their first scalar load, the sort's own skip.
//   k_export_bin_tile    at most 4096 slots: ONE workgroup computes the cells, publishes the OR words and runs every active pass.
//   k_export_bin_starts  behind the sort: lane c of a grid over the n_cells + 2 entries finds the first row of the sorted keys whose key is >= c, a
//                        lower bound of at most 32 steps over n = min(alive_count, capacity) rows. Nothing is zeroed, there are no atomics, and every
//                        entry is written exactly once. With no pass run (one key, or no row) the keys lie in buffer 0 as the keys kernel left them:
//                        equal keys are sorted keys.
// The simulation is only read. Every loop is bounded by the capacity or by 32; every grid is sized from the capacity or from n_cells. No workgroup
// waits for another.
#include <hip/hip_runtime.h>

#include "hnb_export_bin.h"
#include "hnb_export_sort.hip.h"

#pragma clang fp contract(off)   // the cell arithmetic is rounded operation by operation (the unit is also built with -ffp-contract=off)

using namespace hnb;

namespace {

__device__ __forceinline__ uint32_t cell_of_slot(const BinGrid& g, const uint32_t* __restrict__ plane, uint32_t slot) {
    const uint32_t* p = plane + (size_t)slot * 3u;
    return bin_cell_of(g, __uint_as_float(p[0]), __uint_as_float(p[1]), __uint_as_float(p[2]));
}

}  // namespace

// sort_keys_rows of hnb_export_sort.hip.h with cell_of_slot in place of key_of_slot
extern "C" __global__ void __launch_bounds__(256) k_export_bin_keys(const ExportBinArgs a) {
    __shared__ uint32_t s_hist[kExportSortPasses][256];
    const uint32_t j = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const SortView v = sort_view<kSortEffect>(a.s);
    const SortSource s = sort_source(a.s);
    if (j >= a.s.tiles || j * kExportSortTile >= s.n) return;
#pragma unroll
    for (uint32_t d = 0; d < kExportSortPasses; ++d) s_hist[d][tid] = 0u;
    __syncthreads();
    uint32_t ork = 0u, ornk = 0u;
    for (uint32_t r = 0; r < kSortRounds; ++r) {
        const uint32_t rbase = j * kExportSortTile + r * kExportBlock;
        if (rbase >= s.n) break;
        const uint32_t i = rbase + tid;
        const bool valid = i < s.n;
        uint32_t key = 0u;
        if (valid) {
            const uint32_t slot = s.slot(i, a.s.capacity);
            key = cell_of_slot(a.g, s.plane, slot);
            v.keys[i] = key;
            v.vals[i] = slot;
            ork |= key; ornk |= ~key;
        }
#pragma unroll
        for (uint32_t d = 0; d < kExportSortPasses; ++d) hist_add(s_hist[d], (key >> (8u * d)) & 0xffu, valid, lane);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t d = 0; d < kExportSortPasses; ++d) {
        const uint32_t c = s_hist[d][tid];
        v.hist[((size_t)d * a.s.tiles + j) * 256u + tid] = c;
        if (c) atomicAdd(v.gsum + ((size_t)d * a.s.groups + j / kExportSortGroup) * 256u + tid, c);
    }
    ork = wave_or(ork); ornk = wave_or(ornk);
    if (lane == 0u) { atomicOr(&v.state->or_keys, ork); atomicOr(&v.state->or_not_keys, ornk); }
}

// Effects of at most kExportSortTile slots: the whole call but the table and the gather by one workgroup in one launch, barriers only.
extern "C" __global__ void __launch_bounds__(256) k_export_bin_tile(const ExportBinArgs a) {
    const SortSource s = sort_source(a.s);
    const uint32_t n = s.n < kExportSortTile ? s.n : kExportSortTile;             // (capacity <= kExportSortTile: the host launches this kernel for nothing else)
    sort_tile_rows<kSortEffect, true>(a.s, n, [&](const SortView& v, uint32_t& ork, uint32_t& ornk) {
        for (uint32_t r = 0; r < kSortRounds; ++r) {
            const uint32_t i = r * kExportBlock + threadIdx.x;
            if (i >= n) break;
            const uint32_t slot = s.slot(i, a.s.capacity);
            const uint32_t key = cell_of_slot(a.g, s.plane, slot);
            v.keys[i] = key;
            v.vals[i] = slot;
            ork |= key; ornk |= ~key;
        }
    });
}

extern "C" __global__ void __launch_bounds__(256) k_export_bin_starts(const ExportBinArgs a) {
    const uint32_t c = blockIdx.x * kExportBlock + threadIdx.x;
    if (c >= export_bin_entries(a.g.n_cells)) return;
    const uint32_t varying = a.s.state->or_keys & a.s.state->or_not_keys;         // uniform: scalar loads
    const uint32_t alive = a.s.meta[0].alive_count;
    const uint32_t n = alive < a.s.capacity ? alive : a.s.capacity;
    const uint32_t* __restrict__ keys = a.s.keys + (size_t)export_sort_pass(varying, kExportSortPasses).src * a.s.pitch;   // where the gather finds the order
    uint32_t lo = 0u, hi = n;                                                     // the answer lies in [lo, hi]; keys[i] is read for i < n only
    for (uint32_t step = 0; step < 32u; ++step) {
        if (lo >= hi) break;
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < c) lo = mid + 1u; else hi = mid;
    }
    a.cell_start[c] = lo;
}
