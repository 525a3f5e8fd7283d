// The binned export (hnb_effect_export_binned, include/hanabi_amd_binned.h), shared by its kernels' translation unit (hnb_export_bin.hip, a code
// object of its own) and the runtime that loads and launches them (hanabi_amd.hip): the argument block, the kernels by name and the launches of a
// call. The call is the sorted export with the cell of a uniform grid as the key (hnb_bin_cell.h) and, behind the sort, one lower bound per table
// entry over the sorted keys: cell_start[c] = the first row whose key is >= c. Its scratch is export_sort_scratch_layout(1, capacity,
// HNB_SORT_SCOPE_INSTANCE), an allocation of the effect's own. Numbered and planned apart from the units of hnb_export.h, as the bounds are
// (hnb_bounds.h): that header's units, kernels and plans are what they were. Plain C++ below the argument block: a host compiler takes it, so the
// tests check the plan without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd_binned.h"
#include "hnb_bin_cell.h"
#include "hnb_export.h"

namespace hnb {

struct ExportBinArgs {
    ExportSortArgs s;               // as the sorted export binds it; plane_off: the POSITION plane; key, is_f32, descending, v are not read
    BinGrid g;
    uint32_t* cell_start;           // [g.n_cells + 2]
};
HNB_SORT_KEY_FN uint32_t export_bin_entries(uint32_t n_cells) { return n_cells + 2u; }   // (n_cells <= 2^24)

// The kernels of hnb_export_bin.hip: the index of a kernel's handle in the context's table of this unit. In an ExportLaunch they are told from an
// ExportKernel by kExportBinKernelBase, which lies above every ExportKernel; their argument block is numbered behind hnb_export.h's.
enum ExportBinKernel : uint32_t { kBinKTile, kBinKKeys, kBinKStarts, kExportBinKernelCount };
constexpr uint32_t kExportBinKernelBase = 0x100u;
constexpr uint32_t kExportArgsBin = kExportArgsCullProg + 1u;
static_assert(kExportBinKernelBase >= kExpKernelCount, "a launch's kernel names an ExportKernel or, from the base on, an ExportBinKernel");

// The launches of one binned export, in order: (one workgroup | memset + keys + the sort's hist / scatter passes) + the table + the sort's gather.
// At most 11. A capacity must fit a sort (export_sort_scratch_layout(1, capacity, HNB_SORT_SCOPE_INSTANCE).rows != 0). Decides; hanabi_amd.hip
// run_export_plan executes.
HNB_SORT_KEY_FN ExportPlan export_bin_launch_plan(uint32_t capacity, uint32_t stride_bytes, uint32_t n_cells) {
    ExportPlan pl = {};
    pl.memset_before = kExportNoMemset;
    const ExportSortScratch l = export_sort_scratch_layout(1u, capacity, HNB_SORT_SCOPE_INSTANCE);
    const uint32_t variant = export_variant(stride_bytes), tile_rows = export_tile_rows(variant);
    const auto add = [&pl](uint32_t kernel, uint32_t gx, uint32_t args, uint32_t pass = 0u) { pl.launch[pl.n++] = ExportLaunch{kernel, gx, 1u, args, pass}; };
    if (l.tiles <= 1u) add(kExportBinKernelBase + kBinKTile, 1u, kExportArgsBin);                  // cells and every pass by one workgroup
    else {
        pl.memset_before = pl.n; pl.zero_off = l.state_off; pl.zero_bytes = l.zero_bytes;
        add(kExportBinKernelBase + kBinKKeys, l.tiles, kExportArgsBin);                           // the cells, and pass 0's digit counts
        for (uint32_t pass = 0; pass < kExportSortPasses; ++pass) {
            if (pass) add(kExpSortHist, l.tiles, kExportArgsSortPass, pass);
            add(kExpSortScatter, l.tiles, kExportArgsSortPass, pass);
        }
    }
    add(kExportBinKernelBase + kBinKStarts, (export_bin_entries(n_cells) + kExportBlock - 1u) / kExportBlock, kExportArgsBin);   // one lane per entry of cell_start[]
    add(export_rows_kernel(kExportSorted, false, HNB_SORT_SCOPE_INSTANCE, variant), (uint32_t)(((uint64_t)capacity + tile_rows - 1u) / tile_rows), kExportArgsRows);
    return pl;
}

}  // namespace hnb
