// Packed output (include/hanabi_amd.h "Packed output"): the alive particles of an effect, in list order, as records of a layout the caller
// describes - "row r of the list = record r of your buffer". A code object of its own (hipcc --genco, loaded with hipModuleLoadData on first use):
// nothing here is part of the fat binary of libhanabi_amd.so.
//
// k_export_rows: a workgroup of 256 lanes owns a tile of consecutive list rows.
//   Phase 1  lane l loads the slot of row row0 + l (coalesced; the ring wrap per row), then every field's plane[slot] (packed planes: dword loads
//            for vec3) and writes it into an LDS image of the tile's records; dwords no field covers are written as zero.
//   Phase 2  after a barrier the workgroup streams the image to dst: 16-byte stores, consecutive lanes on consecutive addresses - full lines, not
//            4..16-byte pieces at the record pitch. A tile starts at row0 * stride bytes, 16-byte aligned because tiles hold a multiple of 4 rows; in
//            the program form an instance's first record is wherever the instances before it end, so up to 3 leading dwords go out singly.
//            The last, partial tile stores whole records only.
// k_export_offsets: the program form's exclusive scan of the instances' alive counts (one workgroup), in front of the gather.
#include <hip/hip_runtime.h>

#include "hnb_export.h"

using namespace hnb;

namespace {

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

template <uint32_t LDS_DWORDS>
__device__ __forceinline__ void export_rows(const ExportArgs& a) {
    __shared__ __attribute__((aligned(16))) uint32_t image[LDS_DWORDS];
    const uint32_t k = blockIdx.y, tid = threadIdx.x;
    const HnbDeviceMeta m = a.meta[k];                                           // uniform: scalar loads
    const uint32_t n = m.alive_count;
    const uint32_t row0 = blockIdx.x * a.tile_rows;
    if (a.out_count && blockIdx.x == 0u && tid == 0u) {                           // (effect form only)
        a.out_count[0] = (uint64_t)n < a.dst_capacity ? n : (uint32_t)a.dst_capacity;
        a.out_count[1] = n;
    }
    if (row0 >= n) return;                                                        // the grid is sized from capacity: workgroups past the count leave here
    const uint64_t first = (a.offsets ? (uint64_t)a.offsets[k] : 0ull) + row0;   // record of the tile's first row
    if (first >= a.dst_capacity) return;
    uint32_t rows = n - row0 < a.tile_rows ? n - row0 : a.tile_rows;
    if ((uint64_t)rows > a.dst_capacity - first) rows = (uint32_t)(a.dst_capacity - first);
    const char* base = reinterpret_cast<const char*>(a.slabs[k]);
    const uint32_t* list = reinterpret_cast<const uint32_t*>(base + a.alive_off[m.list_column & 1u]);
    const uint32_t head = m.list_column >> 1, sdw = a.stride_dw;

    // ---- phase 1: gather into the LDS image ----
    if (tid < rows) {
        const uint32_t slot = list[ring_index(head, row0 + tid, a.capacity)];
        const uint32_t id = (a.slot_bases ? a.slot_bases[k] : a.slot_base) + slot;
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

}  // namespace

extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_rows_32(const ExportArgs a) { export_rows<256u * 32u / 4u>(a); }
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_rows_64(const ExportArgs a) { export_rows<256u * 64u / 4u>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_rows_128(const ExportArgs a) { export_rows<256u * 128u / 4u>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_rows_256(const ExportArgs a) { export_rows<128u * 256u / 4u>(a); }

// offsets[k] = alive rows of the instances in front of k, offsets[n_inst] = their total; out_count (may be NULL): [0] = records the gather writes
// (the clamp against dst_capacity is global), [1] = the total. One workgroup of 256 lanes: a block scan per 256 instances, a running carry between them.
extern "C" __global__ void __launch_bounds__(256)
k_export_offsets(const HnbDeviceMeta* __restrict__ meta, uint32_t n_inst, uint32_t* __restrict__ offsets, uint32_t* __restrict__ out_count, uint64_t dst_capacity) {
    __shared__ uint32_t part[256];
    __shared__ uint32_t carry;
    const uint32_t tid = threadIdx.x;
    if (tid == 0u) carry = 0u;
    __syncthreads();
    for (uint32_t k0 = 0; k0 < n_inst; k0 += 256u) {
        const uint32_t k = k0 + tid;
        const uint32_t mine = k < n_inst ? meta[k].alive_count : 0u;
        part[tid] = mine;
        __syncthreads();
        for (uint32_t d = 1u; d < 256u; d <<= 1) {                                // Hillis-Steele inclusive scan
            const uint32_t add = tid >= d ? part[tid - d] : 0u;
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        const uint32_t c = carry;
        if (k < n_inst) offsets[k] = c + part[tid] - mine;
        __syncthreads();
        if (tid == 255u) carry = c + part[255];
        __syncthreads();
    }
    if (tid == 0u) {
        const uint32_t total = carry;
        offsets[n_inst] = total;
        if (out_count) { out_count[0] = (uint64_t)total < dst_capacity ? total : (uint32_t)dst_capacity; out_count[1] = total; }
    }
}
