// The packed input (hnb_effect_import, include/hanabi_amd_import.h), shared by its kernels' translation unit (hnb_import.hip, a code object of its
// own) and the runtime that loads and launches them (hanabi_amd.hip): the argument block, the kernels by name, the check of a description, the
// range test of an id and the launches of a call. The call is the mirror image of hnb_effect_export: the tile's records stream from `src` into an
// LDS image, then one lane per record resolves its slot (the alive list's row, or the record's ID field) and stores the fields into the planes.
// Numbered and planned apart from the units of hnb_export.h, as the bounds and the binned export are: that header's units, kernels and plans are
// what they were. Plain C++ below the argument block: a host compiler takes it, so the tests check the refusals, the range test and the plan without
// a GPU.
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd_import.h"
#include "hnb_export.h"

namespace hnb {

struct ImportArgs {
    const uint64_t* slab;           // [1] the instance's slab base address
    const HnbDeviceMeta* meta;      // [1] its row after the frames enqueued so far (ROWS: alive_count, list column and head)
    const uint32_t* src;            // 16-byte aligned
    const uint32_t* src_count;      // may be NULL
    uint32_t* out_count;            // may be NULL; IDS: zeroed in front of the launch
    uint64_t src_capacity;          // records (IDS: at most 0xFFFFFFFF)
    uint64_t alive_off[2];          // bytes from the slab base
    uint64_t alive_flag_off;        // the alive bytes, one per slot
    uint32_t capacity, stride_dw, n_fields, tile_rows, slot_base;
    uint32_t id_dw;                 // IDS: the dword of a record that holds slot_base + slot
    ExportFieldArg fields[HNB_EXPORT_MAX_FIELDS];   // the payload fields (the ID field is not among them): dst_dw is the dword in the SOURCE record
};

// The kernels of hnb_import.hip: the index of a kernel's handle in the context's table of this unit. One instantiation per mode and LDS image
// (export_variant: records of up to 32 / 64 / 128 bytes in tiles of 256 rows, up to 256 bytes in tiles of 128 rows).
enum ImportKernel : uint32_t { kImpRows0, kImpRows1, kImpRows2, kImpRows3, kImpIds0, kImpIds1, kImpIds2, kImpIds3, kImportKernelCount };
struct ImportKernelName { uint32_t kernel; const char* name; };
constexpr ImportKernelName kImportKernelNames[kImportKernelCount] = {
    {kImpRows0, "k_import_rows_32"}, {kImpRows1, "k_import_rows_64"}, {kImpRows2, "k_import_rows_128"}, {kImpRows3, "k_import_rows_256"},
    {kImpIds0, "k_import_ids_32"},   {kImpIds1, "k_import_ids_64"},   {kImpIds2, "k_import_ids_128"},   {kImpIds3, "k_import_ids_256"}};
HNB_SORT_KEY_FN uint32_t import_rows_kernel(uint32_t mode, uint32_t variant) { return (mode == HNB_IMPORT_IDS ? kImpIds0 : kImpRows0) + variant; }

// The slot an id names: id - slot_base in uint32_t, inside the effect iff below the capacity. The subtraction wraps, so an id below slot_base
// becomes a large value and fails the one comparison, and a slot_base near 2^32 whose ids wrap through 0 is handled the same way.
HNB_SORT_KEY_FN bool import_slot_of_id(uint32_t id, uint32_t slot_base, uint32_t capacity, uint32_t* slot) {
    const uint32_t s = id - slot_base;
    *slot = s;
    return s < capacity;
}


// ---- the check of a description: a pure function over the description and the layout's (attr, ncomp) ----
struct ImportLayoutAttr { uint32_t attr, ncomp; };
enum ImportDescError : uint32_t {
    kImportOk, kImportErrStructSize, kImportErrFieldCount, kImportErrFlags, kImportErrReserved, kImportErrMode, kImportErrStride, kImportErrSrc, kImportErrCountPtr,
    kImportErrFieldReserved, kImportErrAttr, kImportErrNotInLayout, kImportErrFieldPlace, kImportErrOverlap, kImportErrIdInRows, kImportErrIdCount, kImportErrCapacity,
    kImportDescErrorCount
};
struct ImportPayload { uint32_t layout_index, src_dw, ncomp; };
struct ImportCheck {
    uint32_t error;                 // ImportDescError
    uint32_t field;                 // the field the error names
    uint32_t n_payload;             // the fields with a plane
    uint32_t id_dw;                 // IDS: where the ID lies
    bool has_age;                   // AGE is among the fields
    ImportPayload payload[HNB_EXPORT_MAX_FIELDS];
};
HNB_SORT_KEY_FN const char* import_error_text(uint32_t e) {
    switch (e) {
    case kImportOk: return "ok";
    case kImportErrStructSize: return "HnbImportDesc::struct_size is not this library's";
    case kImportErrFieldCount: return "n_fields: 1..HNB_EXPORT_MAX_FIELDS fields per record";
    case kImportErrFlags: return "flags: no flag is defined";
    case kImportErrReserved: return "HnbImportDesc::reserved is not 0";
    case kImportErrMode: return "mode: HNB_IMPORT_ROWS or HNB_IMPORT_IDS";
    case kImportErrStride: return "record_stride: a multiple of 4 bytes, at most 256";
    case kImportErrSrc: return "src: a 16-byte aligned device pointer";
    case kImportErrCountPtr: return "src_count / out_count is not 4-byte aligned";
    case kImportErrFieldReserved: return "a field's reserved is not 0";
    case kImportErrAttr: return "the attribute cannot be imported (PARTICLE_COUNTER is a property of the effect, not of a particle)";
    case kImportErrNotInLayout: return "the attribute is not part of the particle layout";
    case kImportErrFieldPlace: return "offsets are multiples of 4, fields end inside the stride";
    case kImportErrOverlap: return "the field overlaps an earlier field";
    case kImportErrIdInRows: return "HNB_ATTR_ID is no field of HNB_IMPORT_ROWS: the list row names the particle";
    case kImportErrIdCount: return "HNB_IMPORT_IDS takes exactly one HNB_ATTR_ID field";
    case kImportErrCapacity: return "HNB_IMPORT_IDS without src_count reads src_capacity_records records: at most 0xFFFFFFFF";
    }
    return "?";
}
HNB_SORT_KEY_FN ImportCheck import_check_desc(const HnbImportDesc& d, const ImportLayoutAttr* layout, uint32_t n_layout) {
    ImportCheck c = {};
    const auto fail = [&c](uint32_t e, uint32_t f = 0u) { c.error = e; c.field = f; return c; };
    if (d.struct_size != sizeof(HnbImportDesc)) return fail(kImportErrStructSize);
    if (d.n_fields == 0 || d.n_fields > HNB_EXPORT_MAX_FIELDS) return fail(kImportErrFieldCount);
    if (d.flags != 0) return fail(kImportErrFlags);
    if (d.reserved != 0) return fail(kImportErrReserved);
    if (d.mode != HNB_IMPORT_ROWS && d.mode != HNB_IMPORT_IDS) return fail(kImportErrMode);
    if (d.record_stride == 0 || d.record_stride % 4u != 0 || d.record_stride > kExportMaxStride) return fail(kImportErrStride);
    if (!d.src || ((uintptr_t)d.src & 15u) != 0) return fail(kImportErrSrc);
    if (((uintptr_t)d.src_count & 3u) != 0 || ((uintptr_t)d.out_count & 3u) != 0) return fail(kImportErrCountPtr);
    uint64_t covered = 0;
    uint32_t ids = 0;
    for (uint32_t f = 0; f < d.n_fields; ++f) {
        const HnbExportField& in = d.fields[f];
        if (in.reserved != 0) return fail(kImportErrFieldReserved, f);
        if (in.attr == HNB_ATTR_PARTICLE_COUNTER || in.attr >= HNB_ATTR_COUNT) return fail(kImportErrAttr, f);
        uint32_t nc = 1, li = 0;
        if (in.attr == HNB_ATTR_ID) {
            if (d.mode == HNB_IMPORT_ROWS) return fail(kImportErrIdInRows, f);
        } else {
            while (li < n_layout && layout[li].attr != in.attr) ++li;
            if (li == n_layout) return fail(kImportErrNotInLayout, f);
            nc = layout[li].ncomp;
        }
        if (in.dst_offset % 4u != 0 || (uint64_t)in.dst_offset + nc * 4u > d.record_stride) return fail(kImportErrFieldPlace, f);
        const uint32_t dw = in.dst_offset / 4u;
        const uint64_t bits = ((1ull << nc) - 1ull) << dw;
        if (covered & bits) return fail(kImportErrOverlap, f);
        covered |= bits;
        if (in.attr == HNB_ATTR_ID) { c.id_dw = dw; ++ids; }
        else {
            c.payload[c.n_payload++] = ImportPayload{li, dw, nc};
            if (in.attr == HNB_ATTR_AGE) c.has_age = true;
        }
    }
    if (d.mode == HNB_IMPORT_IDS && ids != 1u) return fail(kImportErrIdCount);
    if (d.mode == HNB_IMPORT_IDS && !d.src_count && d.src_capacity_records > 0xFFFFFFFFull) return fail(kImportErrCapacity);
    return c;
}


// ---- the launches of one import, in stream order ----
// (k_materialise_age of the instance, when AGE is imported while its plane may be stale) + (IDS with an out_count: 8 bytes of it zeroed) + the
// scatter. ROWS: the grid is sized from the capacity; IDS: from src_capacity_records (at most 0xFFFFFFFF: the count is a 32-bit word), and no
// kernel at all when that is 0. Behind them the caller enqueues the resets (hanabi_amd.hip reset_plane_proofs). Decides; hanabi_amd.hip run_import
// executes.
enum ImportStep : uint32_t { kImportStepMaterialise, kImportStepZeroCounts, kImportStepScatter };
struct ImportLaunch { uint32_t step, kernel, grid_x; };   // (kernel, grid_x: kImportStepScatter only; workgroups of kExportBlock lanes)
constexpr uint32_t kImportPlanMax = 3;
struct ImportPlan { uint32_t n; ImportLaunch launch[kImportPlanMax]; };
HNB_SORT_KEY_FN ImportPlan import_launch_plan(uint32_t capacity, uint32_t stride_bytes, uint32_t mode, uint64_t src_capacity_records, bool materialise_age = false,
                                              bool has_out_count = false) {
    ImportPlan pl = {};
    const uint32_t variant = export_variant(stride_bytes), tile_rows = export_tile_rows(variant);
    const uint64_t rows = mode == HNB_IMPORT_IDS ? (src_capacity_records < 0xFFFFFFFFull ? src_capacity_records : 0xFFFFFFFFull) : capacity;
    const uint32_t tiles = (uint32_t)((rows + tile_rows - 1u) / tile_rows);       // (in 64 bits; at most 2^25)
    if (materialise_age) pl.launch[pl.n++] = ImportLaunch{kImportStepMaterialise, 0u, 0u};
    if (mode == HNB_IMPORT_IDS && has_out_count) pl.launch[pl.n++] = ImportLaunch{kImportStepZeroCounts, 0u, 0u};
    if (tiles) pl.launch[pl.n++] = ImportLaunch{kImportStepScatter, import_rows_kernel(mode, variant), tiles};
    return pl;
}

}  // namespace hnb
