// The neighbour list across two effects (hnb_effect_pairs_from, include/hanabi_amd_pairs_from.h; DESIGN.md "Neighbour pairs across effects"): for
// every alive particle of fx inside a uniform grid, the slots of the particles of ANOTHER effect - the source - within a radius and within one cell
// of it, as CSR in the binned export's row order of fx. A code object of its own: nothing here is part of the fat binary of libhanabi_amd.so. Only
// what is new lives here; in front of these kernels a call runs, unchanged and into its own scratch, for the SOURCE the binned export's
// k_export_bin_keys / k_export_bin_tile, the sorted export's k_export_sort_hist / _scatter, k_export_bin_starts and the neighbour sums'
// k_neighbours_pack (with no channels: it writes (x, y, z, slot) only) - the cells as sorted keys, cell_start[] and the cell-ordered snapshot - and
// for FX the same sort alone, in the same grid: its queries in cell order. Between the two kernels runs hnb_pairs.hip's k_pairs_scan, unchanged.
//   k_pairs_from_count  lane r of workgroup t takes query row r = 256 t + lane of fx's sorted order. Rows at and past min(alive_count, capacity) of
//                   fx do not exist; a row whose key is n_cells or above is in the outside bin: run length 0. An inside row takes its slot from
//                   the sort's values and its position from fx's plane (a scattered 12-byte read), forms the nine ranges in the SOURCE's
//                   cell_start, applies the crowding guard from their lengths and walks the source's snapshot (hnb_pairs_from.h
//                   pairs_from_row_count), counting. count[r] goes to scratch; the tile's sum - __shfl_xor over the wave, four words in LDS - to
//                   tile[t] as 64 bits. Stats are summed over the workgroup in LDS before one atomic add per non-zero word; one lane of
//                   workgroup 0 adds the inside sources to word [7].
//   k_pairs_from_fill   q_capacity + 1 lanes: lane r takes the in-tile exclusive prefix of count[] (wave scan, four words in LDS), T[r] = tile[t] +
//                   prefix, writes out_start[r] = min(T[r], pair_capacity) and out_rows[r], tails included - there is no table for the queries:
//                   inside is r < rows_n && key < n_cells, and the outside rows form the tail because the sort is ascending -, and - when its run
//                   is not empty and starts below pair_capacity - reads its position again, walks again (pairs_from_row_fill) and stores source
//                   slots, and d2 when asked, at T[r] + k while that index is below pair_capacity.
// The lanes of a wave hold consecutive sorted query rows, so they share cells and read the same 16-byte candidate records at the same time, as in
// k_neighbours_from_gather. Nothing of either effect is written. Every loop is bounded by 9 or candidate_limit; every grid is sized from fx's
// capacity. No workgroup waits for another. Index bounds: query rows read of the sort are below min(alive_count, capacity) of fx <= q_pitch; query
// slots come from fx's sort and are below fx's capacity; snapshot rows read are below the source's cell_start[n_cells] <= min(alive_count, capacity)
// of the source <= the source's pitch; table entries read are at most n_cells (a query whose key is n_cells or above walks nothing); count[] is
// written and read below fx's capacity (<= q_pitch); tile[] is written at t < tiles by the count (its grid is tiles), read at t <= tiles by the fill
// (its grid is at most tiles + 1), and holds tiles + 1 entries; out_rows is stored below fx's capacity, out_start at and below it, out_pairs /
// out_d2 below pair_capacity by the test in front of every store; a slot stored comes from the source's alive list.
#include <hip/hip_runtime.h>

#include "hnb_pairs_from.h"

#pragma clang fp contract(off)   // the rule is f32 arithmetic stated operation by operation (the unit is also built with -ffp-contract=off)

using namespace hnb;

namespace {

// Which half of fx's sort holds the order: uniform (scalar loads)
__device__ __forceinline__ size_t sorted_half(const PairsFromArgs& a) {
    const uint32_t varying = a.q_state->or_keys & a.q_state->or_not_keys;
    return (size_t)export_sort_pass(varying, kExportSortPasses).src * a.q_pitch;
}

// The position of fx's slot `slot`, from its plane
struct QueryPos { float x, y, z; };
__device__ __forceinline__ QueryPos query_pos(const PairsFromArgs& a, uint32_t slot) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.q_slab[0]) + a.q_pos_off) + (size_t)slot * 3u;
    return {__uint_as_float(p[0]), __uint_as_float(p[1]), __uint_as_float(p[2])};
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// The inclusive prefix sum over the lanes of a wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_pairs_from_count(const PairsFromArgs a) {
    __shared__ uint32_t s_stats[4];
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, r = blockIdx.x * kPairsFromBlock + tid;
    if (tid < 4u) s_stats[tid] = 0u;
    __syncthreads();
    const size_t half = sorted_half(a);
    const uint32_t alive = a.q_meta[0].alive_count;
    const uint32_t rows_n = alive < a.q_capacity ? alive : a.q_capacity;
    uint32_t visited = 0u, inside = 0u, outside = 0u, crowded = 0u, count = 0u;
    if (r < rows_n) {
        visited = 1u;
        const uint32_t cell = a.q_keys[half + r];
        if (cell >= a.grid.n_cells) outside = 1u;                          // the outside bin's key is n_cells
        else {
            inside = 1u;
            const QueryPos q = query_pos(a, a.q_vals[half + r]);           // (the slot is from fx's alive list: below fx's capacity)
            const PairsFromRowCount rc = pairs_from_row_count(a.snap, a.cell_start, a.grid.dims, cell, q.x, q.y, q.z, a.candidate_limit, a.r2);
            count = rc.count;
            crowded = rc.crowded;
        }
    }
    if (r < a.q_capacity) a.count[r] = count;
    const uint32_t wsum = wave_sum(count);
    if (lane == 0u) s_wave[tid >> 6] = wsum;
    const uint32_t w[4] = {wave_sum(visited), wave_sum(inside), wave_sum(outside), wave_sum(crowded)};
    if (a.stats != nullptr && lane == 0u) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i)
            if (w[i]) atomicAdd(&s_stats[i], w[i]);
    }
    __syncthreads();
    if (tid == 0u) a.tile[blockIdx.x] = (uint64_t)s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (a.stats != nullptr && tid < 4u && s_stats[tid]) (void)__hip_atomic_fetch_add(a.stats + tid, s_stats[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.stats != nullptr && blockIdx.x == 0u && tid == 4u)               // the source's side, once: the words were cleared in front of the call
        (void)__hip_atomic_fetch_add(a.stats + 7, a.cell_start[a.grid.n_cells], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // inside sources: the first outside row
}

extern "C" __global__ void __launch_bounds__(256) k_pairs_from_fill(const PairsFromArgs a) {
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = blockIdx.x * kPairsFromBlock + tid;
    const uint32_t c = r < a.q_capacity ? a.count[r] : 0u;                 // (a tile's run lengths sum to at most 256 * 65536: 32 bits hold the prefix)
    const uint32_t inc = wave_scan(c, lane);
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t front = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i)
        if (i < wave) front += s_wave[i];
    if (r > a.q_capacity) return;
    const uint64_t T = a.tile[blockIdx.x] + (uint64_t)(front + inc - c);   // (rows at and past n_inside count 0: T is the total there)
    a.out_start[r] = pairs_clamp(T, a.pair_capacity);
    if (r == a.q_capacity) return;
    const size_t half = sorted_half(a);
    const uint32_t alive = a.q_meta[0].alive_count;
    const uint32_t rows_n = alive < a.q_capacity ? alive : a.q_capacity;
    const uint32_t cell = r < rows_n ? a.q_keys[half + r] : a.grid.n_cells;
    const bool inside = cell < a.grid.n_cells;
    const uint32_t slot = inside ? a.q_vals[half + r] : HNB_PAIRS_NO_ROW;
    a.out_rows[r] = slot;
    // A crowded, an outside and a missing row counted 0, so c != 0 also says that the row is inside and passed the crowding guard: the walk below
    // is bounded by candidate_limit, not only the count. Rows whose run is empty or starts at or past pair_capacity have nothing to store and do
    // not walk again.
    if (c != 0u && inside && T < (uint64_t)a.pair_capacity) {
        const QueryPos q = query_pos(a, slot);
        (void)pairs_from_row_fill(a.snap, a.cell_start, a.grid.dims, cell, q.x, q.y, q.z, a.r2, T, a.pair_capacity, a.out_pairs, a.out_d2);
    }
}
