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
// The body of the gather is export_rows in hnb_export_rows.hip.h, shared with the sorted export's code object (hnb_export_sort.hip).
#include <hip/hip_runtime.h>

#include "hnb_export_rows.hip.h"

using namespace hnb;

extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_rows_32(const ExportArgs a) { export_rows<256u * 32u / 4u, false>(a); }
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_rows_64(const ExportArgs a) { export_rows<256u * 64u / 4u, false>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_rows_128(const ExportArgs a) { export_rows<256u * 128u / 4u, false>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_rows_256(const ExportArgs a) { export_rows<128u * 256u / 4u, false>(a); }

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
