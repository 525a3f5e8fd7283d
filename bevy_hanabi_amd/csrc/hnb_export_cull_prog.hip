// Filtered, then sorted export, program form (hnb_program_export_sorted with an HnbExportSortFiltered, include/hanabi_amd.h "Packed output";
// DESIGN.md "Filtered, then sorted, program form"): of ALL instances of a program the alive particles a predicate keeps - one filter for all of them
// or one per instance -, every instance's segment in the order of a 32-bit key, segments back to back in instance order. A code object of its own,
// the seventh: nothing here is part of the fat binary of libhanabi_amd.so. It is hnb_export_cull.hip with the instance as blockIdx.y: only what
// joins the filtered program export to the sorted one lives here; the rest of a call is the kernels of hnb_export_filter_prog.hip, hnb_export.hip
// and hnb_export_sort.hip, unchanged, and the bodies below are theirs (hnb_export_filter.hip.h, hnb_export_sort.hip.h).
//   k_export_cull_keys_inst   above 4096 slots, behind k_export_filter_mark_inst / _scan_inst / _compact_inst: workgroup (j, k) is the sorted export's
//                             keys kernel over tile j of the rows instance k's compaction kept - n = word 0 of kept[k], row i = order[k][i] - into
//                             instance k's section of (keys[0], vals[0]), with the tile's counts of all four digits and the OR words.
//                             k_export_sort_scatter_inst / _hist_inst and the gather k_export_sort_rows_inst_* follow; they take the same count from
//                             the rows ExportCullProgArgs::s.meta names, which ARE kept[].
//   k_export_cull_tile_inst   at most 4096 slots: ONE workgroup per instance marks its rows, ranks the kept ones, writes a kept row's (key, slot)
//                             straight to its rank - order[] is not used -, publishes the kept count in kept[k] and the OR words and runs every
//                             active pass.
// The simulation is only read. Every loop is bounded by the capacity; every grid is sized from it and from the instance count. No workgroup waits
// for another.
#include <hip/hip_runtime.h>

#include "hnb_export.h"
#include "hnb_export_filter.hip.h"
#include "hnb_export_sort.hip.h"

#pragma clang fp contract(off)   // predicates and keys are rounded operation by operation (the unit is also built with -ffp-contract=off)

using namespace hnb;

namespace {

// The rows of the keys kernel: what an instance's compaction left. A slot is clamped before it addresses a plane, as the filtered gather clamps it:
// nothing outside the planes is read whatever the scratch holds.
struct KeptSource {
    const uint32_t* order;
    const uint32_t* plane;
    uint32_t n;
    __device__ __forceinline__ uint32_t slot(uint32_t i, uint32_t capacity) const {
        const uint32_t s = order[i];
        return s < capacity ? s : capacity - 1u;
    }
};

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_export_cull_keys_inst(const ExportCullProgArgs a) {
    const uint32_t k = blockIdx.y;
    if (k >= a.p.n_inst) return;
    const uint32_t kept = a.p.f.state[(size_t)k * (sizeof(HnbDeviceMeta) / 4u)];  // uniform: a scalar load
    KeptSource s;
    s.order = a.p.f.order + (size_t)k * a.p.order_pitch;
    s.plane = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.s.slab[k]) + a.s.plane_off);
    s.n = kept < a.s.capacity ? kept : a.s.capacity;
    sort_keys_rows<kSortBatch>(a.s, s);
}

// Instances of at most kExportSortTile slots: the whole call but the counts' scan and the gather, one workgroup per instance in one launch,
// barriers only.
extern "C" __global__ void __launch_bounds__(256) k_export_cull_tile_inst(const ExportCullProgArgs a) {
    __shared__ uint64_t s_word[kFilterWords];
    __shared__ uint32_t s_pref[kFilterWords];
    __shared__ uint32_t s_total;
    const uint32_t k = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (k >= a.p.n_inst) return;
    const ExportFilterArgs f = filter_instance_args(a.p, k);
    FilterSource s = filter_source(a.p.f, k);
    if (s.n > kExportFilterTile) s.n = kExportFilterTile;                         // (capacity <= kExportFilterTile: the host launches this kernel for nothing else)
    const uint32_t* key_plane = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.s.slab[k]) + a.s.plane_off);
    mark_tile_by(s, f.capacity, 0u, s_word, tid, [&](uint32_t slot) { return keeps_slot_of_view(f, s.plane, slot); });
    uint32_t kept = tile_prefix(s_word, s_pref, &s_total, tid);
    if (kept > a.s.capacity) kept = a.s.capacity;                                 // (at most s.n bits are set)
    if (tid == 0u) f.state[0] = kept;                                             // kept[k]: the scan's input and the gather's row count
    sort_tile_rows<kSortBatch, true>(a.s, kept, [&](const SortView& v, uint32_t& ork, uint32_t& ornk) {
        for (uint32_t r = 0; r < kFilterRounds; ++r) {
            const uint32_t rbase = r * kExportBlock;
            if (rbase >= s.n) break;
            const uint32_t w = r * kFilterWaves + wave, i = rbase + tid;
            const uint64_t word = s_word[w];
            if (((word >> lane) & 1ull) && i < s.n) {
                const uint32_t at = s_pref[w] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
                if (at < kept) {                                                  // inside the instance's (keys[0], vals[0]) whatever the mask holds
                    const uint32_t slot = s.list[ring_index(s.head, i, f.capacity)];
                    const uint32_t key = key_of_slot(a.s, key_plane, slot);
                    v.keys[at] = key;
                    v.vals[at] = slot;
                    ork |= key; ornk |= ~key;
                }
            }
        }
    });
}
