// Filtered export, program form (hnb_program_export_filtered, include/hanabi_amd.h "Packed output"; DESIGN.md "Filtered export, program form"): the
// alive particles of ALL instances of a program that a predicate keeps - one filter for all of them or one per instance - as packed records,
// instances back to back in instance order, every segment in list order. A code object of its own, like the four before it: nothing here is part
// of the fat binary of libhanabi_amd.so. The bodies are the filtered export's (hnb_export_filter.hip.h) and the shared gather's
// (hnb_export_rows.hip.h); what this unit adds is the instance, blockIdx.y, and where instance k's tables, scratch sections and filter lie
// (filter_instance_args).
//   k_export_filter_mark_inst     workgroup (j, k): tile j of instance k's list -> its 64 mask words and tile_count[k][j].
//   k_export_filter_scan_inst     ONE workgroup per instance: the exclusive scan of its tile counts -> tile_offset[k][], the kept count -> word 0 of
//                                 kept[k], a 32-byte row with HnbDeviceMeta's layout whose other words stay zero.
//   (k_export_offsets of hnb_export.hip, bound to kept[]: the exclusive scan of the kept counts -> offsets[], out_count.)
//   k_export_filter_compact_inst  workgroup (j, k): order[k][tile_offset + rank] = slot.
//   k_export_filter_tile_inst     instances of at most 4096 slots: mark, count and compact of instance k by ONE workgroup, barriers only.
//   k_export_filter_rows_inst_*   the gather with meta = kept: n = kept[k].alive_count, slot = order[k][r], the record position from offsets[k].
// The simulation is only read. Every loop is bounded by the capacity; every grid is sized from it and from the instance count, and workgroups past
// an instance's alive_count leave after the scalar loads. No workgroup waits for another.
#include <hip/hip_runtime.h>

#include "hnb_export_filter.hip.h"

#pragma clang fp contract(off)   // the predicates are rounded operation by operation (the unit is also built with -ffp-contract=off)

using namespace hnb;

namespace {

// The body of k_export_filter_scan (hnb_export_filter.hip) over one instance's view: tile_offset[j] = kept rows of the tiles in front of j, for the
// tiles that hold rows (the others were not counted and are not compacted); state[0] = the total. One workgroup of 256 lanes: a block scan per 256 tiles, a running carry between them - at most tiles-of-capacity / 256 rounds.
__device__ __forceinline__ void scan_tile_counts(const ExportFilterArgs& a, const FilterSource& s) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t carry;
    const uint32_t tid = threadIdx.x;
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

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_export_filter_mark_inst(const ExportFilterProgArgs p) {
    __shared__ uint64_t s_word[kFilterWords];
    __shared__ uint32_t s_pref[kFilterWords];
    __shared__ uint32_t s_total;
    const uint32_t j = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    if (k >= p.n_inst) return;
    const ExportFilterArgs a = filter_instance_args(p, k);
    const FilterSource s = filter_source(p.f, k);
    if (j >= a.tiles || j * kExportFilterTile >= s.n) return;
    mark_tile_by(s, a.capacity, j, s_word, tid, [&](uint32_t slot) { return keeps_slot_of_view(a, s.plane, slot); });
    if (tid < kFilterWords) a.mask[(size_t)j * kFilterWords + tid] = s_word[tid];
    const uint32_t kept = tile_prefix(s_word, s_pref, &s_total, tid);
    if (tid == 0u) a.tile_count[j] = kept;
}

extern "C" __global__ void __launch_bounds__(256) k_export_filter_scan_inst(const ExportFilterProgArgs p) {
    const uint32_t k = blockIdx.y;
    if (k >= p.n_inst) return;
    scan_tile_counts(filter_instance_args(p, k), filter_source(p.f, k));
}

extern "C" __global__ void __launch_bounds__(256) k_export_filter_compact_inst(const ExportFilterProgArgs p) {
    __shared__ uint64_t s_word[kFilterWords];
    __shared__ uint32_t s_pref[kFilterWords];
    __shared__ uint32_t s_total;
    const uint32_t j = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    if (k >= p.n_inst) return;
    const ExportFilterArgs a = filter_instance_args(p, k);
    const FilterSource s = filter_source(p.f, k);
    if (j >= a.tiles || j * kExportFilterTile >= s.n) return;
    if (tid < kFilterWords) s_word[tid] = a.mask[(size_t)j * kFilterWords + tid];
    __syncthreads();
    tile_prefix(s_word, s_pref, &s_total, tid);
    compact_tile(a, s, j, s_word, s_pref, a.tile_offset[j], tid);
}

// Instances of at most kExportFilterTile slots: an instance's whole compaction by one workgroup, barriers only.
extern "C" __global__ void __launch_bounds__(256) k_export_filter_tile_inst(const ExportFilterProgArgs p) {
    __shared__ uint64_t s_word[kFilterWords];
    __shared__ uint32_t s_pref[kFilterWords];
    __shared__ uint32_t s_total;
    const uint32_t k = blockIdx.y, tid = threadIdx.x;
    if (k >= p.n_inst) return;
    const ExportFilterArgs a = filter_instance_args(p, k);
    FilterSource s = filter_source(p.f, k);
    if (s.n > kExportFilterTile) s.n = kExportFilterTile;                         // (capacity <= kExportFilterTile: the host launches this kernel for nothing else)
    mark_tile_by(s, a.capacity, 0u, s_word, tid, [&](uint32_t slot) { return keeps_slot_of_view(a, s.plane, slot); });
    const uint32_t kept = tile_prefix(s_word, s_pref, &s_total, tid);
    if (tid == 0u) a.state[0] = kept;
    compact_tile(a, s, 0u, s_word, s_pref, 0u, tid);
}

extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_filter_rows_inst_32(const ExportArgs a) { export_rows<256u * 32u / 4u, kRowsFilteredInstance>(a); }
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_filter_rows_inst_64(const ExportArgs a) { export_rows<256u * 64u / 4u, kRowsFilteredInstance>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_filter_rows_inst_128(const ExportArgs a) { export_rows<256u * 128u / 4u, kRowsFilteredInstance>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_filter_rows_inst_256(const ExportArgs a) { export_rows<128u * 256u / 4u, kRowsFilteredInstance>(a); }
