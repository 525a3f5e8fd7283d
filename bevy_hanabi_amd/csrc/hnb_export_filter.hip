// Filtered export (hnb_effect_export_filtered, include/hanabi_amd.h "Packed output"; DESIGN.md "Filtered export"): the alive particles of ONE effect
// that a predicate keeps - inside up to six half-spaces, inside a sphere, or with a scalar attribute in a range - as packed records in list order.
// A code object of its own, like hnb_export.hip and hnb_export_sort.hip: nothing here is part of the fat binary of libhanabi_amd.so.
//
// The simulation is only read: the alive list, the planes and the metadata row stay as they are, the kept rows' slots live in scratch the library owns
// per effect (export_filter_scratch_layout). A stable compaction over tiles of 4096 rows with 256 lanes:
//   k_export_filter_mark     row r: slot = list[ring(head, r)], the predicate on plane[slot] (hnb_filter_pred.h); every wave's ballot is one 64-bit word
//                            of the tile's mask (LDS, then 512 bytes to global memory), the tile's kept count -> tile_count[tile].
//   k_export_filter_scan     ONE workgroup: the exclusive scan of the counts of the tiles that hold rows -> tile_offset[], the total -> state[0].
//   k_export_filter_compact  a tile reads its 64 mask words and ranks its kept rows by the popcounts of the earlier words and of the lower lanes; the
//                            list row is read again only for kept rows; order[tile_offset + rank] = slot, contiguous per tile.
//   k_export_filter_tile     an effect of at most 4096 slots: mark, the count and compact by ONE workgroup in one launch, the mask never leaves LDS.
//   k_export_filter_rows_*   the gather of hnb_export_rows.hip.h with n = state[0] and slot = order[r].
// Every loop is bounded by the capacity; every grid is sized from it, and workgroups past alive_count leave after the scalar loads. No workgroup
// waits for another.
#include <hip/hip_runtime.h>

#include "hnb_export_filter.hip.h"   // the rows a filter kernel reads, the predicate of a slot, a tile's mask, its prefix and its compaction

#pragma clang fp contract(off)   // the predicates are rounded operation by operation (the unit is also built with -ffp-contract=off)

using namespace hnb;

namespace {

constexpr uint32_t kWords = kFilterWords;

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_export_filter_mark(const ExportFilterArgs a) {
    __shared__ uint64_t s_word[kWords];
    __shared__ uint32_t s_pref[kWords];
    __shared__ uint32_t s_total;
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const FilterSource s = filter_source(a);
    if (j >= a.tiles || j * kExportFilterTile >= s.n) return;
    mark_tile(a, s, j, s_word, tid);
    if (tid < kWords) a.mask[(size_t)j * kWords + tid] = s_word[tid];
    const uint32_t kept = tile_prefix(s_word, s_pref, &s_total, tid);
    if (tid == 0u) a.tile_count[j] = kept;
}

// tile_offset[j] = kept rows of the tiles in front of j, for the tiles that hold rows (the others were not counted and are not compacted); state[0] =
// the total. One workgroup of 256 lanes: a block scan per 256 tiles, a running carry between them - at most tiles-of-capacity / 256 rounds.
extern "C" __global__ void __launch_bounds__(256) k_export_filter_scan(const ExportFilterArgs a) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t carry;
    const uint32_t tid = threadIdx.x;
    const FilterSource s = filter_source(a);
    uint32_t used = s.n / kExportFilterTile + (s.n % kExportFilterTile ? 1u : 0u);   // tiles that hold rows; <= a.tiles
    if (used > a.tiles) used = a.tiles;
    if (tid == 0u) carry = 0u;
    __syncthreads();
    for (uint32_t k0 = 0; k0 < used; k0 += 256u) {
        const uint32_t k = k0 + tid;
        const uint32_t mine = k < used ? a.tile_count[k] : 0u;
        part[tid] = mine;
        __syncthreads();
        for (uint32_t d = 1u; d < 256u; d <<= 1) {                                // Hillis-Steele inclusive scan
            const uint32_t add = tid >= d ? part[tid - d] : 0u;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        const uint32_t c = carry;
        if (k < used) a.tile_offset[k] = c + part[tid] - mine;
        __syncthreads();
        if (tid == 255u) carry = c + part[255];
        __syncthreads();
    }
    if (tid == 0u) a.state[0] = carry;
}

extern "C" __global__ void __launch_bounds__(256) k_export_filter_compact(const ExportFilterArgs a) {
    __shared__ uint64_t s_word[kWords];
    __shared__ uint32_t s_pref[kWords];
    __shared__ uint32_t s_total;
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const FilterSource s = filter_source(a);
    if (j >= a.tiles || j * kExportFilterTile >= s.n) return;
    if (tid < kWords) s_word[tid] = a.mask[(size_t)j * kWords + tid];
    __syncthreads();
    tile_prefix(s_word, s_pref, &s_total, tid);
    compact_tile(a, s, j, s_word, s_pref, a.tile_offset[j], tid);
}

// Effects of at most kExportFilterTile slots: the whole compaction by one workgroup in one launch, barriers only.
extern "C" __global__ void __launch_bounds__(256) k_export_filter_tile(const ExportFilterArgs a) {
    __shared__ uint64_t s_word[kWords];
    __shared__ uint32_t s_pref[kWords];
    __shared__ uint32_t s_total;
    const uint32_t tid = threadIdx.x;
    FilterSource s = filter_source(a);
    if (s.n > kExportFilterTile) s.n = kExportFilterTile;                         // (capacity <= kExportFilterTile: the host launches this kernel for nothing else)
    mark_tile(a, s, 0u, s_word, tid);
    const uint32_t kept = tile_prefix(s_word, s_pref, &s_total, tid);
    if (tid == 0u) a.state[0] = kept;
    compact_tile(a, s, 0u, s_word, s_pref, 0u, tid);
}

extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_filter_rows_32(const ExportArgs a) { export_rows<256u * 32u / 4u, kRowsFiltered>(a); }
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_filter_rows_64(const ExportArgs a) { export_rows<256u * 64u / 4u, kRowsFiltered>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_filter_rows_128(const ExportArgs a) { export_rows<256u * 128u / 4u, kRowsFiltered>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_filter_rows_256(const ExportArgs a) { export_rows<128u * 256u / 4u, kRowsFiltered>(a); }
