// Kernel arguments of the packed export (hnb_effect_export / hnb_program_export, include/hanabi_amd.h "Packed output"): shared by the
// kernels' translation unit (hnb_export.hip, a code object of its own) and the runtime that loads and launches them (hanabi_amd.hip).
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd.h"

namespace hnb {

constexpr uint32_t kExportBlock = 256;         // lanes per workgroup: one list row per lane and pass
constexpr uint32_t kExportMaxStride = 256;     // bytes per record
constexpr uint32_t kExportIdField = 0x100u;    // ExportFieldArg::ncomp_flags: the field is HNB_ATTR_ID (slot_base + slot, no plane)

struct ExportFieldArg {
    uint64_t plane_off;      // bytes from an instance's slab base
    uint32_t dst_dw;         // dwords from the record's start
    uint32_t ncomp_flags;    // bits 0..2: components of 4 bytes; kExportIdField
};

struct ExportArgs {
    const uint64_t* slabs;          // [n_instances] slab base addresses
    const HnbDeviceMeta* meta;      // [n_instances] rows after the frames enqueued so far
    const uint32_t* offsets;        // program form: [n_instances + 1] first record of every instance (k_export_offsets); NULL: one instance, record 0
    const uint32_t* slot_bases;     // program form with an ID field: [n_instances]; NULL: slot_base below
    uint32_t* out_count;            // effect form: [0] = records written, [1] = alive rows found (the program form's are written by k_export_offsets); may be NULL
    uint32_t* dst;                  // 16-byte aligned
    uint64_t dst_capacity;          // records
    uint64_t alive_off[2];          // bytes from the slab base
    uint64_t pad_mask;              // bit d: dword d of a record is covered by no field (written as zero)
    uint32_t capacity, stride_dw, n_fields, tile_rows, slot_base, reserved;
    ExportFieldArg fields[HNB_EXPORT_MAX_FIELDS];
};

// The four instantiations of k_export_rows by the LDS image they declare: records of up to 32 / 64 / 128 bytes in tiles of 256 rows, up to 256 bytes in
// tiles of 128 rows. At most 32 KiB per workgroup.
constexpr uint32_t kExportVariants = 4;
inline uint32_t export_variant(uint32_t stride_bytes) { return stride_bytes <= 32u ? 0u : stride_bytes <= 64u ? 1u : stride_bytes <= 128u ? 2u : 3u; }
inline uint32_t export_tile_rows(uint32_t variant) { return variant == 3u ? 128u : 256u; }

}  // namespace hnb
