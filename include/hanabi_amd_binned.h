/* hanabi_amd_binned.h - the binned export of libhanabi_amd.so: one entry point next to the 61 of hanabi_amd.h, in a header of its own. It uses the
 * types, the error codes and the contract of hanabi_amd.h "Packed output" and is exported by the same library; a caller that does not bin particles
 * does not need it. */
#ifndef HANABI_AMD_BINNED_H
#define HANABI_AMD_BINNED_H

#include "hanabi_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Binned export: the records of hnb_effect_export, ordered by the cell of a uniform 3-D grid that holds their POSITION, and a table on the device
 * that says where every cell's records start - the cell list that clustered or froxel lighting of particles, density injection into a fog volume, a
 * collision broad-phase, a neighbour search or density-driven level of detail start from. One call, no readback. HnbExportDesc is used unchanged.
 * Cell of a particle
 *   p = POSITION as stored: no transform is applied, as in the filters. Every f32 operation is rounded on its own, in the order written.
 *   Per axis c: t = (p[c] - origin[c]) * inv_cell[c]. The axis is inside iff t >= 0 and t < (float)dims[c]: -0 is inside, a NaN or an infinity is
 *   not. Inside: i[c] = (uint32_t)t - t lies in [0, 2^24), the conversion is exact truncation, and the range is tested BEFORE the conversion.
 *   Inside on all three axes: cell = (i[2] * dims[1] + i[1]) * dims[0] + i[0]. Otherwise cell = n_cells = dims[0] * dims[1] * dims[2], the
 *   OUTSIDE BIN.
 * Order
 *   Record r is the alive particle with the r-th smallest cell; particles of one cell stay in list order (the sort is stable); the outside bin
 *   comes last.
 * The table
 *   cell_start[c] = the number of alive rows whose cell is smaller than c, for c = 0 .. n_cells + 1: cell_start[0] = 0, cell_start[n_cells] is the
 *   first outside record, cell_start[n_cells + 1] the alive count. Cell c's records are [cell_start[c], cell_start[c + 1]). Every entry is written
 *   by every call. The table describes the whole order: it is NOT clamped to dst_capacity_records.
 * Counts and clamp
 *   The sorted export's: the first min(alive, dst_capacity_records) records of the order are written, out_count[0] = the records written,
 *   out_count[1] = the alive rows. Records at and past the written count are not touched; padding dwords of written records are zero.
 * One identity
 *   With dims = {1, 1, 1} and a cell that contains every particle, dst and out_count are byte for byte hnb_effect_export's.
 * Everything else is hnb_effect_export_sorted's: enqueued on the simulation stream behind the frames enqueued so far, no host synchronisation and
 *   no readback on the steady path; the alive count, the list column and the ring head are read from the HnbDeviceMeta row on the device; every
 *   grid is sized from the capacity or from n_cells, both known to the host; no workgroup waits for another. Stale AGE is materialised first when
 *   AGE is a record field. The simulation is only read.
 * Errors: HNB_ERR_INVALID_ARG (with hnb_last_error text; nothing is enqueued) for a NULL argument, for everything hnb_effect_export_sorted rejects
 *   in `desc`, another struct_size, flags or reserved not 0, a dims[c] of 0, a product above HNB_BIN_MAX_CELLS (taken in 64 bits), an origin or
 *   inv_cell that is not finite, an inv_cell that is not > 0, cell_start NULL or not 16-byte aligned, a layout without POSITION, an effect of more
 *   than 0xFFFFFF00 slots.
 * Scratch: owned by the library, per effect, one allocation of its own with the sorted export's layout: 16 bytes per slot of capacity plus, for
 *   capacities above 4096, about 5 bytes per slot of digit tables. Allocated by the effect's FIRST binned export - that one call may synchronise
 *   the device once for the allocation - and freed with the effect. Binned exports of one effect reuse it in stream order. It is apart from the
 *   scratch of every other export: the calls may be interleaved on one effect.
 * Out of scope: a program form, a filter in front of the binning, and any transform of the positions.
 * The kernels: the sorted export's digit passes and gather, unchanged, and three that are new (the cells as keys; for effects of at most 4096
 *   slots cells and sort by one workgroup; the table, one lower bound per entry over the sorted keys), which live in a code object of their own
 *   that the library carries and loads on first use; HNB_ERR_HIP if it cannot be loaded. Cells below 2^16 leave the upper two digits of every
 *   key equal, and the sort skips those passes. */
#define HNB_BIN_MAX_CELLS (1u << 24)
typedef struct HnbExportBins {
    uint32_t  struct_size;   /* sizeof(HnbExportBins) of the caller */
    uint32_t  flags;         /* 0 */
    uint32_t  dims[3];       /* cells along x, y, z: each >= 1, product n_cells <= HNB_BIN_MAX_CELLS */
    uint32_t  reserved;      /* 0 */
    float     origin[3];     /* the grid's lowest corner, finite */
    float     inv_cell[3];   /* 1 / cell edge per axis, finite and > 0 */
    uint32_t* cell_start;    /* device, 16-byte aligned: [n_cells + 2] words */
} HnbExportBins;
int hnb_effect_export_binned(HnbEffect* fx, const HnbExportDesc* desc, const HnbExportBins* bins);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_AMD_BINNED_H */
