// Filtered, then sorted export, program form (hnb_program_export_sorted with an HnbExportSortFiltered; include/hanabi_amd.h "Packed output"; DESIGN.md
// "Filtered, then sorted, program form"), shared by the kernels' translation unit (hnb_export_cull_prog.hip: a seventh code object) and the runtime
// that loads and launches them (hanabi_amd.hip): the kernels' argument block, the scratch layout, the unit's kernels by name (CullProgKernel) and the
// launches of a call (cull_prog_launch_plan). hnb_export.h's tables are closed - five units, their kernels and at most twelve launches - so this
// form has a numbering, a plan and a loader of its own, as hnb_bounds.h has; most of its launches are kernels of the older units (ExportKernel),
// bound to this form's scratch. Plain C++: a host compiler takes it, so the tests check the layout and the plan without a GPU.
#pragma once
#include <stdint.h>

#include "hnb_export.h"

namespace hnb {

static_assert(sizeof(HnbExportSortFiltered) == 48, "HnbExportSortFiltered layout");

struct ExportCullProgArgs {
    ExportFilterProgArgs p;         // as the filtered program export binds it (f.meta: the program's rows), in this form's own scratch
    ExportSortArgs s;               // as the sorted program export binds its instance scope, except meta: the kept rows (p.f.state)
};

// The scratch of a program's filtered-then-sorted exports, one allocation: export_filter_prog_scratch_layout, then (at sort_off, a 256-byte
// boundary) export_sort_scratch_layout of the instance scope. sort.rows == 0: more than 0xFFFFFF00 slots, refused as the sorted export refuses them.
struct ExportCullProgScratch { ExportFilterProgScratch filter; ExportSortScratch sort; uint64_t sort_off, total; };
HNB_SORT_KEY_FN ExportCullProgScratch export_cull_prog_scratch_layout(uint32_t n_inst, uint32_t capacity) {
    ExportCullProgScratch l;
    l.filter = export_filter_prog_scratch_layout(n_inst, capacity);
    l.sort = export_sort_scratch_layout(n_inst, capacity, HNB_SORT_SCOPE_INSTANCE);
    l.sort_off = (l.filter.total + 255u) & ~(uint64_t)255u;
    l.total = l.sort_off + l.sort.total;
    return l;
}

// The kernels of hnb_export_cull_prog.hip: the index of a kernel's handle in the context. Numbered apart from ExportKernel.
enum CullProgKernel : uint32_t { kCullProgTileInst, kCullProgKeysInst, kCullProgKernelCount };
// A launch names a kernel of this unit (own) or of the five older ones (an ExportKernel), and what it is passed: an ExportArgBlock, or this unit's block
constexpr uint32_t kCullProgArgs = 7;   // (behind kExportArgsFilterProg)
struct CullProgLaunch { uint32_t own, kernel, grid_x, grid_y, args, pass; };   // (workgroups of kExportBlock lanes)
constexpr uint32_t kCullProgPlanMax = 13;
struct CullProgPlan {
    uint32_t n;                         // launches, in stream order
    uint32_t memset_before;             // above one tile: bytes [zero_off, zero_off + zero_bytes) of the scratch are zeroed in front of launch
    uint64_t zero_off, zero_bytes;      //   `memset_before` (the sort's state words and group sums); kExportNoMemset: nothing is
    CullProgLaunch launch[kCullProgPlanMax];
};

// The launches of one call over n_inst instances of `capacity` slots (at most 0xFFFFFF00), in order. Up to 4096 slots: one workgroup per instance
// does everything in front of the scan of the kept counts, three launches. Above: the filtered program export's compaction, the kept counts'
// scan, the keys of the kept rows, four radix passes and the gather, thirteen. The scan runs behind the kept counts and in front of nothing
// that needs it but the gather; it stands where the filtered program export has it. Decides; hanabi_amd.hip run_export_cull_prog executes.
HNB_SORT_KEY_FN CullProgPlan cull_prog_launch_plan(uint32_t n_inst, uint32_t capacity, uint32_t stride_bytes) {
    CullProgPlan pl = {};
    pl.memset_before = kExportNoMemset;
    const ExportCullProgScratch l = export_cull_prog_scratch_layout(n_inst, capacity);
    const uint32_t tiles = l.filter.tiles, n = n_inst;
    const uint32_t variant = export_variant(stride_bytes), tile_rows = export_tile_rows(variant);
    const auto add = [&pl](uint32_t own, uint32_t kernel, uint32_t gx, uint32_t gy, uint32_t args, uint32_t pass = 0u) {
        pl.launch[pl.n++] = CullProgLaunch{own, kernel, gx, gy, args, pass};
    };
    if (tiles <= 1u) {
        add(1u, kCullProgTileInst, 1u, n, kCullProgArgs);                          // mark, (key, slot) pairs at their ranks, the kept count, every pass
        add(0u, kExpOffsets, 1u, 1u, kExportArgsOffsets);                          // over the kept counts
    } else {
        add(0u, kExpFilterMarkInst, tiles, n, kExportArgsFilterProg);
        add(0u, kExpFilterScanInst, 1u, n, kExportArgsFilterProg);
        add(0u, kExpOffsets, 1u, 1u, kExportArgsOffsets);
        add(0u, kExpFilterCompactInst, tiles, n, kExportArgsFilterProg);
        pl.memset_before = pl.n; pl.zero_off = l.sort_off + l.sort.state_off; pl.zero_bytes = l.sort.zero_bytes;
        add(1u, kCullProgKeysInst, tiles, n, kCullProgArgs);                       // the kept rows' keys, and pass 0's digit counts
        for (uint32_t pass = 0; pass < kExportSortPasses; ++pass) {
            if (pass) add(0u, kExpSortHistInst, tiles, n, kExportArgsSortPass, pass);
            add(0u, kExpSortScatterInst, tiles, n, kExportArgsSortPass, pass);
        }
    }
    add(0u, kExpSortRowsInst0 + variant, (uint32_t)(((uint64_t)capacity + tile_rows - 1u) / tile_rows), n, kExportArgsRows);
    return pl;
}

}  // namespace hnb
