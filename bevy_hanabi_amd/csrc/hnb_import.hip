// Packed input (hnb_effect_import, include/hanabi_amd_import.h; DESIGN.md "Packed input"): records of a layout the caller describes, resident on the
// device, written into the attribute planes of the particles they belong to - the mirror image of k_export_rows (hnb_export_rows.hip.h). A code
// object of its own, like the exports': nothing here is part of the fat binary of libhanabi_amd.so.
//
// k_import_rows_* / k_import_ids_*: a workgroup of 256 lanes owns a tile of consecutive records (256 of up to 128 bytes, 128 of up to 256).
//   Phase 1  the workgroup streams the tile's rows x stride bytes from src into an LDS image: 16-byte loads, consecutive lanes on consecutive
//            addresses - full lines whatever the stride. A tile starts at row0 * stride bytes, 16-byte aligned because tiles hold a multiple of 4
//            records; the last, partial tile may end between two boundaries: its last dwords come in singly, and nothing at or past record n is read.
//   Phase 2  behind one barrier lane l owns record row0 + l. ROWS: its slot is the alive list's row (the ring wrap per row), clamped below the
//            capacity. IDS: the record's ID field minus the slot base, tested against the capacity in uint32_t, then the slot's alive byte; a record
//            that fails either writes nothing. Every field goes from the image into plane[slot]: one 16-byte store for 4 components, 8 bytes
//            for 2, dword stores for 3 and 1 - the inverse of load_field.
//   Counts   ROWS: lane 0 of workgroup 0 writes out_count = {n, 0}. IDS: the host zeroes out_count in front; every workgroup adds its applied and
//            its skipped records, counted by ballots, with one integer atomicAdd each (the wave sums meet in the image, which is free by then).
// The lists, the alive bytes and the counters are only read. The grid is sized by the host from the capacity (ROWS) or from src_capacity_records
// (IDS); workgroups past the count leave after their scalar loads. No workgroup waits for another.
#include <hip/hip_runtime.h>

#include "hnb_export_rows.hip.h"
#include "hnb_import.h"

using namespace hnb;

namespace {

// rec: the record in the LDS image (dword aligned only); the plane's slot is 16-byte aligned for 4 components, 8 for 2 (planes are 256-byte aligned)
__device__ __forceinline__ void scatter_field(char* __restrict__ base, const ExportFieldArg f, uint32_t slot, const uint32_t* rec) {
    const uint32_t nc = f.ncomp_flags & 7u;
    const uint32_t* s = rec + f.dst_dw;
    uint32_t* p = reinterpret_cast<uint32_t*>(base + f.plane_off) + (size_t)slot * nc;
    if (nc == 4u) *reinterpret_cast<uint4*>(p) = make_uint4(s[0], s[1], s[2], s[3]);
    else if (nc == 3u) { p[0] = s[0]; p[1] = s[1]; p[2] = s[2]; }
    else if (nc == 2u) *reinterpret_cast<uint2*>(p) = make_uint2(s[0], s[1]);
    else p[0] = s[0];
}

template <uint32_t LDS_DWORDS, uint32_t MODE>
__device__ __forceinline__ void import_rows(const ImportArgs& a) {
    __shared__ __attribute__((aligned(16))) uint32_t image[LDS_DWORDS];
    const uint32_t tid = threadIdx.x;
    uint64_t n64 = a.src_capacity;                                                // uniform: scalar loads
    if (a.src_count) { const uint32_t c = a.src_count[0]; n64 = c < n64 ? c : n64; }
    uint32_t head = 0u;
    const uint32_t* list = nullptr;
    char* base = reinterpret_cast<char*>(a.slab[0]);
    if constexpr (MODE == HNB_IMPORT_ROWS) {
        const HnbDeviceMeta m = a.meta[0];
        uint32_t alive = m.alive_count < a.capacity ? m.alive_count : a.capacity;
        n64 = alive < n64 ? alive : n64;
        head = m.list_column >> 1;
        list = reinterpret_cast<const uint32_t*>(base + a.alive_off[m.list_column & 1u]);
    } else if (n64 > 0xFFFFFFFFull) n64 = 0xFFFFFFFFull;                          // (the host refused it; the grid covers no more)
    const uint32_t n = (uint32_t)n64;
    const uint32_t row0 = blockIdx.x * a.tile_rows;
    if constexpr (MODE == HNB_IMPORT_ROWS)
        if (a.out_count && blockIdx.x == 0u && tid == 0u) { a.out_count[0] = n; a.out_count[1] = 0u; }
    if (row0 >= n) return;                                                        // workgroups past the count leave here
    const uint32_t rows = n - row0 < a.tile_rows ? n - row0 : a.tile_rows, sdw = a.stride_dw;

    // ---- phase 1: stream the tile's records into the LDS image ----
    const uint32_t total = rows * sdw;                                            // dwords: at most LDS_DWORDS
    const uint32_t* in = a.src + (uint64_t)row0 * sdw;                            // 16-byte aligned: row0 is a multiple of 128
    const uint32_t nvec = total >> 2;
    {
        const uint4* in4 = reinterpret_cast<const uint4*>(in);
        uint4* img4 = reinterpret_cast<uint4*>(image);
        for (uint32_t i = tid; i < nvec; i += kExportBlock) img4[i] = in4[i];
        const uint32_t done = 4u * nvec;                                          // a partial tile's last record may end between two boundaries
        if (tid < total - done) image[done + tid] = in[done + tid];
    }
    __syncthreads();

    // ---- phase 2: one lane per record ----
    const bool valid = tid < rows;
    bool ok = valid;
    uint32_t slot = 0u;
    if (valid) {
        const uint32_t* rec = image + tid * sdw;
        if constexpr (MODE == HNB_IMPORT_ROWS) {
            slot = list[ring_index(head, row0 + tid, a.capacity)];
            if (slot >= a.capacity) slot = a.capacity - 1u;                       // (the list holds slots; nothing is written outside the planes whatever the buffer holds)
        } else {
            ok = import_slot_of_id(rec[a.id_dw], a.slot_base, a.capacity, &slot);
            if (ok) ok = reinterpret_cast<const uint8_t*>(base + a.alive_flag_off)[slot] != 0u;
        }
        if (ok)
            for (uint32_t f = 0; f < a.n_fields; ++f) scatter_field(base, a.fields[f], slot, rec);
    }

    // ---- counts (IDS): ballots per wave, the four waves' sums through the image, one atomicAdd per count ----
    if constexpr (MODE == HNB_IMPORT_IDS) {
        if (!a.out_count) return;                                                 // uniform
        const uint32_t applied = (uint32_t)__popcll(__ballot(ok)), skipped = (uint32_t)__popcll(__ballot(valid && !ok));
        __syncthreads();                                                          // every lane is done with its record
        if ((tid & 63u) == 0u) { image[2u * (tid >> 6)] = applied; image[2u * (tid >> 6) + 1u] = skipped; }
        __syncthreads();
        if (tid == 0u) {
            uint32_t ap = 0u, sk = 0u;
#pragma unroll
            for (uint32_t w = 0; w < kExportBlock / 64u; ++w) { ap += image[2u * w]; sk += image[2u * w + 1u]; }
            if (ap) atomicAdd(a.out_count, ap);
            if (sk) atomicAdd(a.out_count + 1, sk);
        }
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_import_rows_32(const ImportArgs a) { import_rows<256u * 32u / 4u, HNB_IMPORT_ROWS>(a); }
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_import_rows_64(const ImportArgs a) { import_rows<256u * 64u / 4u, HNB_IMPORT_ROWS>(a); }
extern "C" __global__ void __launch_bounds__(256) k_import_rows_128(const ImportArgs a) { import_rows<256u * 128u / 4u, HNB_IMPORT_ROWS>(a); }
extern "C" __global__ void __launch_bounds__(256) k_import_rows_256(const ImportArgs a) { import_rows<128u * 256u / 4u, HNB_IMPORT_ROWS>(a); }
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_import_ids_32(const ImportArgs a) { import_rows<256u * 32u / 4u, HNB_IMPORT_IDS>(a); }
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_import_ids_64(const ImportArgs a) { import_rows<256u * 64u / 4u, HNB_IMPORT_IDS>(a); }
extern "C" __global__ void __launch_bounds__(256) k_import_ids_128(const ImportArgs a) { import_rows<256u * 128u / 4u, HNB_IMPORT_IDS>(a); }
extern "C" __global__ void __launch_bounds__(256) k_import_ids_256(const ImportArgs a) { import_rows<128u * 256u / 4u, HNB_IMPORT_IDS>(a); }
