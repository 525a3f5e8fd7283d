// Filtered, then sorted export (hnb_effect_export_filtered_sorted, include/hanabi_amd.h "Packed output"; DESIGN.md "Filtered, then sorted"): the alive
// particles of ONE effect that a predicate keeps, as packed records in the order of a 32-bit key. A code object of its own, like the three before it:
// nothing here is part of the fat binary of libhanabi_amd.so. Only what joins the filtered export to the sorted one lives here; the rest of a call
// is the kernels of hnb_export_filter.hip and hnb_export_sort.hip, unchanged, and the bodies below are theirs (hnb_export_filter.hip.h,
// hnb_export_sort.hip.h).
//   k_export_cull_keys   above 4096 slots, behind k_export_filter_mark / _scan / _compact: the sorted export's keys kernel over the rows the filter
//                        kept - n = the filter's state word, row i = order[i] - into (keys[0], vals[0]), with the tile's counts of all four digits
//                        and the OR words. k_export_sort_scatter / _hist and the gather k_export_sort_rows_* follow; they take the same count from
//                        the row ExportCullArgs::s.meta names, whose first word IS the filter's state word.
//   k_export_cull_tile   at most 4096 slots: ONE workgroup marks the rows, ranks the kept ones, writes a kept row's (key, slot) straight to its
//                        rank - order[] is not used -, publishes the kept count and the OR words and runs every active pass.
// The simulation is only read. Every loop is bounded by the capacity; every grid is sized from it. No workgroup waits for another.
#include <hip/hip_runtime.h>

#include "hnb_export_filter.hip.h"
#include "hnb_export_sort.hip.h"

#pragma clang fp contract(off)   // predicates and keys are rounded operation by operation (the unit is also built with -ffp-contract=off)

using namespace hnb;

namespace {

// The rows of the keys kernel: what the filter's compaction left. A slot is clamped before it addresses a plane, as the filtered gather clamps it:
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

extern "C" __global__ void __launch_bounds__(256) k_export_cull_keys(const ExportCullArgs a) {
    const uint32_t kept = a.f.state[0];                                           // uniform: a scalar load
    KeptSource s;
    s.order = a.f.order;
    s.plane = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.s.slab[0]) + a.s.plane_off);
    s.n = kept < a.s.capacity ? kept : a.s.capacity;
    sort_keys_rows<kSortEffect>(a.s, s);
}

// Effects of at most kExportSortTile slots: the whole call but the gather by one workgroup in one launch, barriers only.
extern "C" __global__ void __launch_bounds__(256) k_export_cull_tile(const ExportCullArgs a) {
    __shared__ uint64_t s_word[kFilterWords];
    __shared__ uint32_t s_pref[kFilterWords];
    __shared__ uint32_t s_total;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    FilterSource s = filter_source(a.f);
    if (s.n > kExportFilterTile) s.n = kExportFilterTile;                         // (capacity <= kExportFilterTile: the host launches this kernel for nothing else)
    const uint32_t* key_plane = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.s.slab[0]) + a.s.plane_off);
    mark_tile(a.f, s, 0u, s_word, tid);
    uint32_t kept = tile_prefix(s_word, s_pref, &s_total, tid);
    if (kept > a.s.capacity) kept = a.s.capacity;                                 // (at most s.n bits are set)
    if (tid == 0u) a.f.state[0] = kept;                                           // the gather's row count
    sort_tile_rows<kSortEffect, true>(a.s, kept, [&](const SortView& v, uint32_t& ork, uint32_t& ornk) {
        for (uint32_t r = 0; r < kFilterRounds; ++r) {
            const uint32_t rbase = r * kExportBlock;
            if (rbase >= s.n) break;
            const uint32_t w = r * kFilterWaves + wave, i = rbase + tid;
            const uint64_t word = s_word[w];
            if (((word >> lane) & 1ull) && i < s.n) {
                const uint32_t at = s_pref[w] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
                if (at < kept) {                                                  // inside (keys[0], vals[0]) whatever the mask holds
                    const uint32_t slot = s.list[ring_index(s.head, i, a.f.capacity)];
                    const uint32_t key = key_of_slot(a.s, key_plane, slot);
                    v.keys[at] = key;
                    v.vals[at] = slot;
                    ork |= key; ornk |= ~key;
                }
            }
        }
    });
}
