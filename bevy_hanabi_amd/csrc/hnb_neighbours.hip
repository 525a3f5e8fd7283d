// Neighbour sums (hnb_effect_neighbours, include/hanabi_amd_neighbours.h; DESIGN.md "Neighbours"): for every alive particle of ONE effect inside a
// uniform grid, up to four fixed-point sums over the particles within a radius, stored or added into f32 planes. A code object of its own: nothing
// here is part of the fat binary of libhanabi_amd.so. Only what is new lives here; in front of these two kernels a call runs the binned export's
// k_export_bin_keys / k_export_bin_tile, the sorted export's k_export_sort_hist / _scatter and k_export_bin_starts, unchanged, into its own scratch:
// the cells as sorted keys, the slots as values, and cell_start[].
//   k_neighbours_pack    lane r of a grid over the capacity takes sorted row r (r < min(alive_count, capacity)): (x, y, z, slot) as one 16-byte
//                        record into snap[r] and the row's stored source of every channel into srcv[k][r]. The snapshot is cell-contiguous, so the
//                        gather's reads are coalesced runs; every later read of positions and sources comes from it, never from the planes.
//   k_neighbours_gather  lane r takes sorted row r. Rows at and past cell_start[n_cells] count themselves as outside. The walk around the row's
//                        cell is at most nine contiguous row ranges (hnb_neighbours.h neighbour_range); their lengths give candidates(i) before any
//                        pair is tested: the crowding guard, which bounds every loop below by candidate_limit. The lanes of a wave hold
//                        consecutive sorted rows, so they share cells and read the same 16-byte candidate records at the same time: the loads of
//                        a wave collapse to a few cache lines served by the L1 (no LDS staging: DESIGN.md says why). Four int64 accumulators per
//                        lane (8 VGPRs); at the end the sample's read-modify-write of the destination components of the lane's own slot. Stats
//                        are summed over the workgroup in LDS before one atomic add per non-zero word.
// Every loop is bounded by the capacity, 9 or candidate_limit; every grid is sized from the capacity. No workgroup waits for another. Rows read are
// below cell_start[n_cells] <= min(alive_count, capacity) <= pitch; table entries read are at most n_cells; a slot stored to comes from the alive
// list and is below the capacity.
#include <hip/hip_runtime.h>

#include "hnb_neighbours.h"

#pragma clang fp contract(off)   // the rule is f32 arithmetic stated operation by operation (the unit is also built with -ffp-contract=off)

using namespace hnb;

namespace {

struct NeighbourRows { const uint32_t* keys; const uint32_t* vals; uint32_t n; };

// Where the sort left the order, and how many rows it has: uniform (scalar loads)
__device__ __forceinline__ NeighbourRows sorted_rows(const NeighbourArgs& a) {
    const uint32_t varying = a.state->or_keys & a.state->or_not_keys;
    const size_t half = (size_t)export_sort_pass(varying, kExportSortPasses).src * a.pitch;
    const uint32_t alive = a.meta[0].alive_count;
    NeighbourRows r;
    r.keys = a.keys + half;
    r.vals = a.vals + half;
    r.n = alive < a.capacity ? alive : a.capacity;
    return r;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_neighbours_pack(const NeighbourArgs a) {
    const uint32_t r = blockIdx.x * kNeighbourBlock + threadIdx.x;
    const NeighbourRows rows = sorted_rows(a);
    if (r >= rows.n) return;
    const char* base = reinterpret_cast<const char*>(a.slab[0]);
    const uint32_t slot = rows.vals[r];
    const uint32_t* p = reinterpret_cast<const uint32_t*>(base + a.pos_off) + (size_t)slot * 3u;
    reinterpret_cast<uint4*>(a.snap)[r] = make_uint4(p[0], p[1], p[2], slot);
#pragma unroll
    for (uint32_t k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
        if (k >= a.n_channels) break;
        const uint32_t sp = a.ch[k].src_packed;
        uint32_t v = kNeighbourOneBits;
        if ((sp & kNeighbourSrcOne) == 0u) v = reinterpret_cast<const uint32_t*>(base + a.ch[k].src_plane_off)[(size_t)slot * (sp & 0xFFu) + ((sp >> 8) & 0xFFu)];
        a.srcv[(size_t)k * a.pitch + r] = v;
    }
}

extern "C" __global__ void __launch_bounds__(256) k_neighbours_gather(const NeighbourArgs a) {
    __shared__ uint32_t s_stats[5];
    const uint32_t tid = threadIdx.x, r = blockIdx.x * kNeighbourBlock + tid;
    if (tid < 5u) s_stats[tid] = 0u;
    __syncthreads();
    const NeighbourRows rows = sorted_rows(a);
    const uint32_t inside_n = a.cell_start[a.grid.n_cells];            // the first outside row
    uint32_t visited = 0u, gathered = 0u, outside = 0u, crowded = 0u, rejected = 0u;
    if (r < rows.n) {
        visited = 1u;
        if (r >= inside_n) outside = 1u;
        else {
            const NeighbourCell c = neighbour_cell_xyz(a.grid.dims, rows.keys[r]);   // (an inside row's key is its cell, below n_cells)
            if (neighbour_candidates(a.cell_start, a.grid.dims, c) > a.candidate_limit) crowded = 1u;
            else {
                gathered = 1u;
                const uint4* snap = reinterpret_cast<const uint4*>(a.snap);
                const uint4 own = snap[r];
                const float xi = __uint_as_float(own.x), yi = __uint_as_float(own.y), zi = __uint_as_float(own.z);
                uint32_t vi[HNB_NEIGHBOUR_MAX_CHANNELS];
                int64_t S[HNB_NEIGHBOUR_MAX_CHANNELS];
#pragma unroll
                for (uint32_t k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
                    S[k] = 0;
                    vi[k] = k < a.n_channels ? a.srcv[(size_t)k * a.pitch + r] : 0u;
                }
                for (uint32_t i = 0; i < 9u; ++i) {
                    const NeighbourRange rg = neighbour_range(a.cell_start, a.grid.dims, c, i);
                    for (uint32_t j = rg.lo; j < rg.hi; ++j) {             // (all nine together: at most candidate_limit rounds)
                        if (j == r) continue;                             // the particle itself; a coincident one is another row
                        const uint4 o = snap[j];
                        const float d2 = neighbour_d2(xi, yi, zi, __uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z));
                        if (!(d2 < a.r2)) continue;
                        const float W = neighbour_weight(a.weight, d2, a.inv_r2);
#pragma unroll
                        for (uint32_t k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
                            if (k >= a.n_channels) break;
                            const uint32_t sp = a.ch[k].src_packed;
                            const uint32_t vj = (sp & kNeighbourSrcOne) ? kNeighbourOneBits : a.srcv[(size_t)k * a.pitch + j];
                            const DepositQuant q = neighbour_contribution(vj, vi[k], (sp & kNeighbourSrcDiff) != 0u, a.weight, W, sp >> 24);
                            S[k] += q.q;                                  // (0 when rejected)
                            rejected += q.ok ? 0u : 1u;
                        }
                    }
                }
                char* base = reinterpret_cast<char*>(a.slab[0]);
#pragma unroll
                for (uint32_t k = 0; k < HNB_NEIGHBOUR_MAX_CHANNELS; ++k) {
                    if (k >= a.n_channels) break;
                    const uint32_t dp = a.ch[k].dst_packed, op = dp >> 16;
                    uint32_t* p = reinterpret_cast<uint32_t*>(base + a.ch[k].dst_plane_off) + ((size_t)own.w * (dp & 0xFFu) + ((dp >> 8) & 0xFFu));
                    const uint32_t old = op == HNB_SAMPLE_ADD ? *p : 0u;
                    *p = __float_as_uint(neighbour_store(op, __uint_as_float(old), S[k], a.ch[k].src_packed >> 24, a.scale));
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
}
