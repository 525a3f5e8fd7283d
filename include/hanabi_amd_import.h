/* hanabi_amd_import.h - the packed input of libhanabi_amd.so: one entry point next to the 61 of hanabi_amd.h, in a header of its own. It uses the
 * types and the error codes of hanabi_amd.h and is exported by the same library; a caller that writes nothing back does not need it. */
#ifndef HANABI_AMD_IMPORT_H
#define HANABI_AMD_IMPORT_H

#include "hanabi_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Packed input: the inverse of hnb_effect_export. Records in a caller-described layout, resident on the device, are written into the attribute
 * planes of the particles they belong to - what a consumer on the same GPU (a torch module that predicts forces from an [alive, k] tensor, a
 * collision or constraint pass over the binned export's cell list, a solver on depth-sorted records) hands back to the simulation. One call, no
 * host synchronisation, no readback, and every fact the library caches about the planes is reset as hnb_effect_write_attr resets it.
 * Records
 *   `n_fields` fields of HnbExportField, the type of the exports, so one layout description serves both directions: field f takes the ncomp x 4
 *   bytes at byte `dst_offset` of a record (here: the offset in the SOURCE record) and stores them bit for bit into the slot's place in the plane of
 *   `attr`. Bytes of a record that no field covers are ignored. Attributes not named, and every slot not addressed, keep every bit.
 * Which particle a record belongs to
 *   HNB_IMPORT_ROWS  record r belongs to the particle in row r of the alive list, the export's formula:
 *                    alive_list[list_column & 1][((list_column >> 1) + r) % capacity] - ring lists are read through their head. Column, head and
 *                    alive_count come from the effect's HnbDeviceMeta row on the device. n = min(alive_count, src_capacity_records, *src_count if
 *                    given) records are applied; nothing is skipped, out_count[1] = 0.
 *   HNB_IMPORT_IDS   exactly one field has attr == HNB_ATTR_ID; its value is what HNB_ATTR_ID exports, slot_base + slot. Records may come back in
 *                    any order and as any subset: the output of the sorted, filtered and binned exports. n = min(src_capacity_records, *src_count if
 *                    given) records are read; with src_count == NULL, n = src_capacity_records. A record is SKIPPED - it writes nothing and is counted
 *                    in out_count[1] - when id - slot_base, computed in uint32_t, is >= capacity, or when the slot's alive byte is zero. A
 *                    description whose only field is the ID is legal: it writes nothing and out_count classifies the ids.
 *                    Two records that name one slot: which record's value each component ends up with is unspecified; every stored dword is a
 *                    whole dword of one of the records.
 *   out_count (may be NULL): [0] = records applied, [1] = records skipped.
 * Ordering and state
 *   Asynchronous: enqueued on the context's simulation stream behind everything enqueued so far. No host synchronisation and no readback. `src`,
 *   `src_count` and `out_count` must stay valid until the stream has run the call.
 *   The import never touches the lists, the alive bytes or any counter: a particle whose imported age is at or past its lifetime dies in the next
 *   update like any other.
 *   After the call, later frames compute exactly what they would after hnb_effect_write_attr of planes holding the same values: the call makes the
 *   same resets, on the stream and in the host's plan state (the published no-death bound, the death horizons, the chunks' lifetime bounds, the
 *   ribbon front proofs, and - with AGE among the fields - the age cohorts). One difference follows from writing a subset: when AGE is imported
 *   while its plane may be stale (HnbDeviceView::stale_attr_mask), the plane is materialised first, so the slots the call does not address keep
 *   their true ages.
 *   Frozen instances (hnb_effect_set_simulated(fx, 0)) accept imports.
 * Errors: HNB_ERR_INVALID_ARG (with hnb_last_error text; nothing is enqueued) for a NULL argument, an attribute the layout lacks,
 *   HNB_ATTR_PARTICLE_COUNTER, overlapping fields, a field that is not dword aligned or ends past the stride, a stride that is no multiple of 4 or
 *   above 256, src NULL or not 16-byte aligned, src_count or out_count not 4-byte aligned, n_fields == 0 or above HNB_EXPORT_MAX_FIELDS, flags,
 *   reserved or a field's `reserved` not 0, another struct_size, an unknown mode, HNB_ATTR_ID as a field in ROWS mode, no or more than one ID field in
 *   IDS mode, and in IDS mode without src_count a src_capacity_records above 0xFFFFFFFF.
 * Out of scope: a program form, spawning or killing through the import, any transform of the values, and a defined winner among duplicate ids.
 * The kernels live in a code object of their own that the library carries and loads on first use; HNB_ERR_HIP if it cannot be loaded. There is no
 *   other implementation to fall back to. */
#define HNB_IMPORT_ROWS 0u
#define HNB_IMPORT_IDS  1u
typedef struct HnbImportDesc {
    uint32_t        struct_size;            /* sizeof(HnbImportDesc) of the caller */
    uint32_t        n_fields;               /* 1..HNB_EXPORT_MAX_FIELDS */
    uint32_t        record_stride;          /* bytes per record: a multiple of 4, >= the end of every field, <= 256 */
    uint32_t        mode;                   /* HNB_IMPORT_ROWS or HNB_IMPORT_IDS */
    uint32_t        flags;                  /* 0 */
    uint32_t        reserved;               /* 0 */
    const void*     src;                    /* device pointer, 16-byte aligned */
    uint64_t        src_capacity_records;   /* clamp on the record count */
    const uint32_t* src_count;              /* device pointer, may be NULL: the number of records, read on the device */
    uint32_t*       out_count;              /* device pointer, may be NULL: [0] = records applied, [1] = records skipped */
    HnbExportField  fields[HNB_EXPORT_MAX_FIELDS];
} HnbImportDesc;
int hnb_effect_import(HnbEffect* fx, const HnbImportDesc* desc);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_AMD_IMPORT_H */
