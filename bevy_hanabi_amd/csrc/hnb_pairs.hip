// The neighbour list (hnb_effect_pairs, include/hanabi_amd_pairs.h; DESIGN.md "Neighbour pairs"): for every alive particle of ONE effect inside a
// uniform grid, the slots of the particles within a radius and within one cell of it, as CSR in the binned export's row order. A code object of its
// own: nothing here is part of the fat binary of libhanabi_amd.so. Only what is new lives here; in front of these three kernels a call runs the
// binned export's k_export_bin_keys / k_export_bin_tile, the sorted export's k_export_sort_hist / _scatter, k_export_bin_starts and the neighbour
// sums' k_neighbours_pack (with no channels: it writes (x, y, z, slot) only), unchanged, into its own scratch: the cells as sorted keys,
// cell_start[], and the cell-ordered snapshot.
//   k_pairs_count   lane r of workgroup t takes sorted row r = 256 t + lane. Rows at and past cell_start[n_cells] are outside or do not exist: run
//                   length 0. An inside row takes the crowding guard first, then the gather's walk over at most nine contiguous row ranges
//                   (hnb_pairs.h pairs_row_count), counting. count[r] goes to scratch; the tile's sum - __shfl_xor over the wave, four words in
//                   LDS - to tile[t] as 64 bits. Stats are summed over the workgroup in LDS before one atomic add per non-zero word.
//   k_pairs_scan    ONE workgroup: the exclusive 64-bit scan of tile[0 .. tiles) in place, in rounds of 256 tiles with a running carry; the
//                   true total to tile[tiles] and to stats[4..5], the written total to stats[6]. No look-back, no workgroup waiting on another.
//   k_pairs_fill    capacity + 1 lanes: lane r takes the in-tile exclusive prefix of count[] (wave scan, four words in LDS), T[r] = tile[t] +
//                   prefix, writes out_start[r] = min(T[r], pair_capacity) and out_rows[r], tails included, and - when its run is not empty and
//                   starts below pair_capacity - walks again (pairs_row_fill) and stores slots, and d2 when asked, at T[r] + k while that index
//                   is below pair_capacity.
// Every loop is bounded by the capacity, 9, candidate_limit or the tile count; every grid is sized from the capacity. No workgroup waits for
// another. Rows read are below cell_start[n_cells] <= min(alive_count, capacity) <= pitch; table entries read are at most n_cells; count[] is
// written below the capacity (<= pitch) and read below cell_start[n_cells]; tile[] is written at t < tiles by the count (its grid is tiles), read
// and written below tiles + 1 by the scan, read at t <= tiles by the fill (its grid is at most tiles + 1), and holds tiles + 1 entries; out_rows
// is stored below the capacity, out_start at and below it, out_pairs / out_d2 below pair_capacity by the test in front of every store; a slot
// stored comes from the alive list and is below the capacity.
#include <hip/hip_runtime.h>

#include "hnb_pairs.h"

#pragma clang fp contract(off)   // the rule is f32 arithmetic stated operation by operation (the unit is also built with -ffp-contract=off)

using namespace hnb;

namespace {

// Which half of the sort's keys holds the order: uniform (scalar loads)
__device__ __forceinline__ const uint32_t* sorted_keys(const PairsArgs& a) {
    const uint32_t varying = a.state->or_keys & a.state->or_not_keys;
    return a.keys + (size_t)export_sort_pass(varying, kExportSortPasses).src * a.pitch;
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
__device__ __forceinline__ uint64_t wave_scan64(uint64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
        if (lane >= d) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_pairs_count(const PairsArgs a) {
    __shared__ uint32_t s_stats[4];
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, r = blockIdx.x * kPairsBlock + tid;
    if (tid < 4u) s_stats[tid] = 0u;
    __syncthreads();
    const uint32_t alive = a.meta[0].alive_count;
    const uint32_t rows_n = alive < a.capacity ? alive : a.capacity;
    const uint32_t inside_n = a.cell_start[a.grid.n_cells];                // the first outside row
    uint32_t visited = 0u, inside = 0u, outside = 0u, crowded = 0u, count = 0u;
    if (r < rows_n) {
        visited = 1u;
        if (r >= inside_n) outside = 1u;
        else {
            inside = 1u;
            const PairsRowCount rc = pairs_row_count(a.snap, a.cell_start, a.grid.dims, r, sorted_keys(a)[r], a.candidate_limit, a.r2, a.half != 0u);
            count = rc.count;                                              // (an inside row's key is its cell, below n_cells)
            crowded = rc.crowded;
        }
    }
    if (r < a.capacity) a.count[r] = count;
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
}

// tile[k] = the run lengths of the tiles in front of k; tile[tiles] = the true total. One workgroup of 256 lanes: a block scan per 256 tiles, a
// running carry between them - tiles / 256 rounds, rounded up.
extern "C" __global__ void __launch_bounds__(256) k_pairs_scan(const PairsArgs a) {
    __shared__ uint64_t s_wave[4];
    __shared__ uint64_t s_carry;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0u) s_carry = 0u;
    __syncthreads();
    for (uint32_t k0 = 0; k0 < a.tiles; k0 += kPairsBlock) {
        const uint32_t k = k0 + tid;
        const uint64_t mine = k < a.tiles ? a.tile[k] : 0u;
        const uint64_t inc = wave_scan64(mine, lane);
        if (lane == 63u) s_wave[wave] = inc;
        __syncthreads();
        uint64_t front = s_carry;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i)
            if (i < wave) front += s_wave[i];
        if (k < a.tiles) a.tile[k] = front + inc - mine;
        __syncthreads();
        if (tid == kPairsBlock - 1u) s_carry = front + inc;
        __syncthreads();
    }
    if (tid == 0u) {
        const uint64_t total = s_carry;
        a.tile[a.tiles] = total;
        if (a.stats != nullptr) {
            a.stats[4] = (uint32_t)total;
            a.stats[5] = (uint32_t)(total >> 32);
            a.stats[6] = pairs_clamp(total, a.pair_capacity);
        }
    }
}

extern "C" __global__ void __launch_bounds__(256) k_pairs_fill(const PairsArgs a) {
    __shared__ uint32_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = blockIdx.x * kPairsBlock + tid;
    const uint32_t inside_n = a.cell_start[a.grid.n_cells];
    const uint32_t c = r < inside_n ? a.count[r] : 0u;                     // (a tile's run lengths sum to at most 256 * 65536: 32 bits hold the prefix)
    const uint32_t inc = wave_scan(c, lane);
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t front = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i)
        if (i < wave) front += s_wave[i];
    if (r > a.capacity) return;
    const uint64_t T = a.tile[blockIdx.x] + (uint64_t)(front + inc - c);   // (rows at and past n_inside count 0: T is the total there)
    a.out_start[r] = pairs_clamp(T, a.pair_capacity);
    if (r == a.capacity) return;
    a.out_rows[r] = r < inside_n ? a.snap[r].slot : HNB_PAIRS_NO_ROW;
    // A crowded row counted 0, so c != 0 also says that the row passed the crowding guard: the walk below is bounded by candidate_limit, not only
    // the count. Rows whose run is empty or starts at or past pair_capacity have nothing to store and do not walk again.
    if (c != 0u && T < (uint64_t)a.pair_capacity)
        (void)pairs_row_fill(a.snap, a.cell_start, a.grid.dims, r, sorted_keys(a)[r], a.r2, a.half != 0u, T, a.pair_capacity, a.out_pairs, a.out_d2);
}
