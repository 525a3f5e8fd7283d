// The gather of the packed export (hnb_export.hip: k_export_rows_*, slots from the alive list; hnb_export_sort.hip: k_export_sort_rows_*, slots
// from the order a sorted export produced; k_export_sort_rows_inst_* / _all_*: the two scopes of the sorted program export; hnb_export_filter.hip:
// k_export_filter_rows_*, the slots a filtered export kept; hnb_export_filter_prog.hip: k_export_filter_rows_inst_*, the same per instance). One body; the instantiations by where a row's slot comes from.
#pragma once
#include <hip/hip_runtime.h>

#include "hnb_export.h"

namespace hnb {

__device__ __forceinline__ uint32_t ring_index(uint32_t head, uint32_t r, uint32_t capacity) {   // head < capacity, r < capacity
    const uint32_t i = head + r;
    return (i >= capacity || i < head) ? i - capacity : i;
}

__device__ __forceinline__ uint4 load_field(const char* __restrict__ base, const ExportFieldArg f, uint32_t slot, uint32_t id) {
    const uint32_t nc = f.ncomp_flags & 7u;
    uint4 v = make_uint4(id, 0u, 0u, 0u);
    if (f.ncomp_flags & kExportIdField) return v;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(base + f.plane_off) + (size_t)slot * nc;
    if (nc == 4u) v = *reinterpret_cast<const uint4*>(p);                       // planes are 256-byte aligned: a vec4 slot is 16-byte aligned, a vec2 slot 8
    else if (nc == 3u) { v.x = p[0]; v.y = p[1]; v.z = p[2]; }
    else if (nc == 2u) { const uint2 q = *reinterpret_cast<const uint2*>(p); v.x = q.x; v.y = q.y; }
    else v.x = p[0];
    return v;
}

__device__ __forceinline__ void store_field(uint32_t* rec, const ExportFieldArg f, const uint4 v) {
    const uint32_t nc = f.ncomp_flags & 7u;
    uint32_t* d = rec + f.dst_dw;
    d[0] = v.x;
    if (nc > 1u) d[1] = v.y;
    if (nc > 2u) d[2] = v.z;
    if (nc > 3u) d[3] = v.w;
}

// ORDER: where row r's slot comes from.
//   kRowsList (false)      the alive list's row r
//   kRowsOrdered (true)    order[r], a sorted export's result (export_order_of)
//   kRowsOrderedInstance   instance blockIdx.y's section of the sorted program export's value buffers (export_order_of_instance)
//   kRowsOrderedProgram    one order over all instances: order[r] names (instance, slot); the rows are those of the concatenated space, the
//                          instance's slab and slot base are taken per lane
//   kRowsFiltered          order[r], the slots a filtered export kept (one buffer); the rows are order_state[0], the kept total, not alive_count
//   kRowsFilteredInstance  instance blockIdx.y's section of the filtered program export's order[] (order_pitch slots each); meta[] are the kept rows:
//                          alive_count is the instance's kept count, their other words are zero (the list they would name is never read)
constexpr uint32_t kRowsList = 0, kRowsOrdered = 1, kRowsOrderedInstance = 2, kRowsOrderedProgram = 3, kRowsFiltered = 4, kRowsFilteredInstance = 5;
template <uint32_t LDS_DWORDS, uint32_t ORDER>
__device__ __forceinline__ void export_rows(const ExportArgs& a) {
    __shared__ __attribute__((aligned(16))) uint32_t image[LDS_DWORDS];
    const uint32_t k = ORDER == kRowsOrderedProgram ? 0u : blockIdx.y, tid = threadIdx.x;
    const HnbDeviceMeta m = a.meta[k];                                           // uniform: scalar loads
    uint32_t n = m.alive_count;
    if constexpr (ORDER == kRowsOrderedProgram) {                                 // every instance's rows; the sort bounded them the same way
        const uint32_t all = a.offsets[a.n_inst];
        n = all < a.total_cap ? all : a.total_cap;
    }
    if constexpr (ORDER == kRowsFiltered) {                                       // the rows the filter kept; the compaction bounded them the same way
        const uint32_t kept = a.order_state[0];
        n = kept < a.capacity ? kept : a.capacity;
    }
    if constexpr (ORDER == kRowsFilteredInstance) n = n < a.capacity ? n : a.capacity;   // (a kept count; the compaction bounded it the same way)
    const uint32_t row0 = blockIdx.x * a.tile_rows;
    if (a.out_count && blockIdx.x == 0u && tid == 0u) {                           // (effect form only)
        a.out_count[0] = (uint64_t)n < a.dst_capacity ? n : (uint32_t)a.dst_capacity;
        a.out_count[1] = n;
    }
    if (row0 >= n) return;                                                        // the grid is sized from capacity: workgroups past the count leave here
    const uint64_t first = (ORDER != kRowsOrderedProgram && a.offsets ? (uint64_t)a.offsets[k] : 0ull) + row0;   // record of the tile's first row
    if (first >= a.dst_capacity) return;
    uint32_t rows = n - row0 < a.tile_rows ? n - row0 : a.tile_rows;
    if ((uint64_t)rows > a.dst_capacity - first) rows = (uint32_t)(a.dst_capacity - first);
    const char* base0 = reinterpret_cast<const char*>(a.slabs[k]);
    const uint32_t* list = reinterpret_cast<const uint32_t*>(base0 + a.alive_off[m.list_column & 1u]);
    const uint32_t head = m.list_column >> 1, sdw = a.stride_dw;

    // ---- phase 1: gather into the LDS image ----
    if (tid < rows) {
        uint32_t slot, ki = k;
        const char* base = base0;
        if constexpr (ORDER == kRowsOrdered) slot = export_order_of(a)[row0 + tid];
        else if constexpr (ORDER == kRowsOrderedInstance) slot = export_order_of_instance(a, k)[row0 + tid];
        else if constexpr (ORDER == kRowsOrderedProgram) {
            const uint32_t v = export_order_of(a)[row0 + tid];
            ki = export_sort_unpack_instance(v, a.slot_bits);
            slot = export_sort_unpack_slot(v, a.slot_bits);
            if (ki >= a.n_inst) ki = a.n_inst - 1u;                               // (the sort packed only pairs inside the program; nothing is read outside it whatever the buffer holds)
            if (slot >= a.capacity) slot = a.capacity - 1u;
            base = reinterpret_cast<const char*>(a.slabs[ki]);
        } else if constexpr (ORDER == kRowsFiltered) {
            slot = a.order[row0 + tid];
            if (slot >= a.capacity) slot = a.capacity - 1u;                       // (the compaction wrote list entries; nothing is read outside the planes whatever the buffer holds)
        } else if constexpr (ORDER == kRowsFilteredInstance) {
            slot = a.order[(size_t)k * a.order_pitch + row0 + tid];
            if (slot >= a.capacity) slot = a.capacity - 1u;                       // (as above)
        } else slot = list[ring_index(head, row0 + tid, a.capacity)];
        const uint32_t id = (a.slot_bases ? a.slot_bases[ki] : a.slot_base) + slot;
        uint32_t* rec = image + tid * sdw;
        for (uint32_t f0 = 0; f0 < a.n_fields; f0 += 4u) {                        // four fields' loads in flight together, then their LDS writes
            uint4 v[4];
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q)
                if (f0 + q < a.n_fields) v[q] = load_field(base, a.fields[f0 + q], slot, id);
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q)
                if (f0 + q < a.n_fields) store_field(rec, a.fields[f0 + q], v[q]);
        }
        for (uint64_t pm = a.pad_mask; pm; pm &= pm - 1ull) rec[__builtin_ctzll(pm)] = 0u;
    }
    __syncthreads();

    // ---- phase 2: stream the image out ----
    const uint32_t total = rows * sdw;                                            // dwords
    const uint64_t g0 = first * sdw;                                              // dword index of the tile in dst
    uint32_t* out = a.dst + g0;
    uint32_t lead = (4u - (uint32_t)(g0 & 3ull)) & 3u;                            // dwords in front of the first 16-byte boundary (0 in the effect form)
    if (lead > total) lead = total;
    const uint32_t nvec = (total - lead) >> 2;
    if (lead == 0u) {
        const uint4* src = reinterpret_cast<const uint4*>(image);
        uint4* o = reinterpret_cast<uint4*>(out);
        for (uint32_t i = tid; i < nvec; i += kExportBlock) o[i] = src[i];
    } else {
        if (tid < lead) out[tid] = image[tid];
        uint4* o = reinterpret_cast<uint4*>(out + lead);
        for (uint32_t i = tid; i < nvec; i += kExportBlock) {
            const uint32_t* s = image + lead + 4u * i;
            o[i] = make_uint4(s[0], s[1], s[2], s[3]);
        }
    }
    const uint32_t done = lead + 4u * nvec;                                       // a partial tile's last record may end between two boundaries
    if (tid < total - done) out[done + tid] = image[done + tid];
}

}  // namespace hnb
