// Neighbour sums across two effects (hnb_effect_neighbours_from, include/hanabi_amd_neighbours_from.h; DESIGN.md "Neighbours across effects"): for
// every alive particle of fx inside a uniform grid, up to four fixed-point sums over the particles of ANOTHER effect - the source - within a radius,
// stored or added into f32 planes of fx. A code object of its own: nothing here is part of the fat binary of libhanabi_amd.so. Only what is new
// lives here; in front of this kernel a call runs, unchanged and into its own scratch, for the SOURCE the binned export's k_export_bin_keys /
// k_export_bin_tile, the sorted export's k_export_sort_hist / _scatter, k_export_bin_starts and the neighbour sums' k_neighbours_pack - the cells as
// sorted keys, cell_start[], the cell-ordered snapshot and the stored sources - and for FX the same sort alone, in the same grid: its queries in
// cell order.
//   k_neighbours_from_gather  lane r of a grid over fx's capacity takes query row r of fx's sorted order (r < min(alive_count, capacity) of fx): the
//                        slot from the sort's values, the cell from its key (the outside bin has key n_cells: counted, nothing else). It reads
//                        its own position and its DIFF operands from fx's planes, forms the nine ranges in the SOURCE's cell_start, applies the
//                        crowding guard from their lengths before any pair is tested, and walks the source's snapshot (hnb_neighbours_from.h
//                        neighbours_from_row). The lanes of a wave hold consecutive sorted query rows, so they share cells and read the same
//                        16-byte candidate records at the same time, as in k_neighbours_gather (no LDS staging: DESIGN.md says why). Up to four
//                        int64 accumulators per lane; at the end the sample's read-modify-write of the destination components of the lane's own
//                        slot. Stats are summed over the workgroup in LDS before one atomic add per non-zero word; one lane of workgroup 0 adds
//                        the source's two words.
// The source is only read; no lane reads another query's planes, and a lane has read its own position and operands before it stores. Every loop is
// bounded by 9 or candidate_limit; the grid is sized from fx's capacity. No workgroup waits for another. Index bounds: query slots come from fx's
// sort and are below fx's capacity; snapshot rows read are below the source's cell_start[n_cells] <= min(alive_count, capacity) of the source <=
// the source's pitch; table entries read are at most n_cells (a query whose key is n_cells or above walks nothing).
#include <hip/hip_runtime.h>

#include "hnb_neighbours_from.h"

#pragma clang fp contract(off)   // the rule is f32 arithmetic stated operation by operation (the unit is also built with -ffp-contract=off)

using namespace hnb;

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_neighbours_from_gather(const NeighboursFromArgs a) {
    __shared__ uint32_t s_stats[5];
    const uint32_t tid = threadIdx.x, r = blockIdx.x * kNeighboursFromBlock + tid;
    if (tid < 5u) s_stats[tid] = 0u;
    __syncthreads();
    // where fx's sort left the order, and how many rows it has: uniform (scalar loads)
    const uint32_t varying = a.q_state->or_keys & a.q_state->or_not_keys;
    const size_t half = (size_t)export_sort_pass(varying, kExportSortPasses).src * a.q_pitch;
    const uint32_t q_alive = a.q_meta[0].alive_count;
    const uint32_t rows_n = q_alive < a.q_capacity ? q_alive : a.q_capacity;
    uint32_t visited = 0u, gathered = 0u, outside = 0u, crowded = 0u, rejected = 0u;
    if (r < rows_n) {
        visited = 1u;
        const uint32_t cell = a.q_keys[half + r];
        if (cell >= a.grid.n_cells) outside = 1u;                          // the outside bin's key is n_cells
        else {
            const uint32_t slot = a.q_vals[half + r];                      // (from fx's alive list: below fx's capacity)
            char* base = reinterpret_cast<char*>(a.q_slab[0]);
            const uint32_t* p = reinterpret_cast<const uint32_t*>(base + a.q_pos_off) + (size_t)slot * 3u;
            const float xi = __uint_as_float(p[0]), yi = __uint_as_float(p[1]), zi = __uint_as_float(p[2]);
            uint32_t vi[HNB_NEIGHBOUR_MAX_CHANNELS];
#pragma unroll
            for (uint32_t k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
                const uint32_t sp = a.ch[k].src_packed;
                vi[k] = 0u;
                if (k < a.n_channels && (sp & kNeighbourSrcDiff) != 0u)
                    vi[k] = reinterpret_cast<const uint32_t*>(base + a.ch[k].src_plane_off)[(size_t)slot * (sp & 0xFFu) + ((sp >> 8) & 0xFFu)];
            }
            const NeighboursFromRow row = neighbours_from_row(a.snap, a.srcv, a.s_pitch, a.cell_start, a.grid.dims, cell, xi, yi, zi, vi, a.ch, a.n_channels, a.weight,
                                                              a.candidate_limit, a.r2, a.inv_r2);
            if (row.crowded) crowded = 1u;
            else {
                gathered = 1u;
                rejected = row.rejected;
#pragma unroll
                for (uint32_t k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
                    if (k >= a.n_channels) break;
                    const uint32_t dp = a.ch[k].dst_packed, op = dp >> 16;
                    uint32_t* d = reinterpret_cast<uint32_t*>(base + a.ch[k].dst_plane_off) + ((size_t)slot * (dp & 0xFFu) + ((dp >> 8) & 0xFFu));
                    const uint32_t old = op == HNB_SAMPLE_ADD ? *d : 0u;
                    *d = __float_as_uint(neighbour_store(op, __uint_as_float(old), row.S[k], a.ch[k].src_packed >> 24, a.scale));
                }
            }
        }
    }
    if (a.stats == nullptr) return;
    const uint32_t lane = tid & 63u;
    const uint32_t w[5] = {wave_sum(visited), wave_sum(gathered), wave_sum(outside), wave_sum(crowded), wave_sum(rejected)};
    if (lane == 0u) {
#pragma unroll
        for (uint32_t i = 0; i < 5u; ++i)
            if (w[i]) atomicAdd(&s_stats[i], w[i]);
    }
    __syncthreads();
    if (tid < 5u && s_stats[tid]) (void)__hip_atomic_fetch_add(a.stats + tid, s_stats[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (blockIdx.x == 0u && tid == 5u) {                                   // the source's side, once: the words were cleared in front of the call
        const uint32_t s_alive = a.s_meta[0].alive_count;
        (void)__hip_atomic_fetch_add(a.stats + 5, a.cell_start[a.grid.n_cells], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // inside sources: the first outside row
        (void)__hip_atomic_fetch_add(a.stats + 6, s_alive < a.s_capacity ? s_alive : a.s_capacity, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // alive sources visited
    }
}
