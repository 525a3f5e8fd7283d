// The pieces of the filtered export's kernels (hnb_export_filter.hip) that the filtered-then-sorted export (hnb_export_cull.hip) and the filtered
// program export (hnb_export_filter_prog.hip) run as well: the rows a filter kernel reads, the predicate of a slot, a tile's mask, the prefix of its
// words and its compaction, and an instance's view of a program call's argument block. Included by the three units; the design is described in
// hnb_export_filter.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "hnb_export_rows.hip.h"
#include "hnb_filter_pred.h"

#pragma clang fp contract(off)   // the predicates are rounded operation by operation (the units are also built with -ffp-contract=off)

namespace hnb {
namespace {

constexpr uint32_t kFilterWaves = kExportBlock / 64u;
constexpr uint32_t kFilterRounds = kExportFilterTile / kExportBlock;
constexpr uint32_t kFilterWords = kExportFilterTileWords;
static_assert(kFilterWords == kFilterRounds * kFilterWaves && kFilterWords == 64u, "one mask word per wave and round; the words of a tile are scanned by one wave");

struct FilterSource {
    const uint32_t* list;
    const uint32_t* plane;
    uint32_t head, n;
};

// The rows of instance k of the tables a.slab / a.meta (an effect's own block names one row of each: k = 0)
__device__ __forceinline__ FilterSource filter_source(const ExportFilterArgs& a, uint32_t k) {
    const HnbDeviceMeta m = a.meta[k];                                            // uniform: scalar loads
    const char* base = reinterpret_cast<const char*>(a.slab[k]);
    FilterSource s;
    s.list = reinterpret_cast<const uint32_t*>(base + a.alive_off[m.list_column & 1u]);
    s.plane = reinterpret_cast<const uint32_t*>(base + a.plane_off);
    s.head = m.list_column >> 1;
    s.n = m.alive_count < a.capacity ? m.alive_count : a.capacity;
    return s;
}
__device__ __forceinline__ FilterSource filter_source(const ExportFilterArgs& a) { return filter_source(a, 0u); }

// include/hanabi_amd.h states these formulas; hnb_filter_pred.h evaluates them operation by operation.
__device__ __forceinline__ bool keeps_slot(const ExportFilterArgs& a, const uint32_t* __restrict__ plane, uint32_t slot) {
    bool pass;
    if (a.kind == HNB_FILTER_ATTR_RANGE) {
        pass = filter_pass_range(plane[slot], a.is_f32 != 0u, a.lo_bits, a.hi_bits);
    } else {
        const uint32_t* p = plane + (size_t)slot * 3u;
        const float x = __uint_as_float(p[0]), y = __uint_as_float(p[1]), z = __uint_as_float(p[2]);
        pass = a.kind == HNB_FILTER_PLANES ? filter_pass_planes(x, y, z, a.P, a.n_planes) : filter_pass_sphere(x, y, z, a.P[0]);
    }
    return pass != (a.invert != 0u);
}

// Tile j's mask into s_word[kFilterWords]: word r * kFilterWaves + wave = the ballot of round r's wave; rounds past the count give zero words. Ends behind a barrier.
// keep(slot): the predicate of a slot.
template <class Keep>
__device__ __forceinline__ void mark_tile_by(const FilterSource& s, uint32_t capacity, uint32_t j, uint64_t* s_word, uint32_t tid, Keep keep_slot) {
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    for (uint32_t r = 0; r < kFilterRounds; ++r) {
        const uint32_t rbase = j * kExportFilterTile + r * kExportBlock;
        bool keep = false;
        if (rbase < s.n) {                                                        // uniform
            const uint32_t i = rbase + tid;
            if (i < s.n) keep = keep_slot(s.list[ring_index(s.head, i, capacity)]);
        }
        const uint64_t word = __ballot(keep);
        if (lane == 0u) s_word[r * kFilterWaves + wave] = word;
    }
    __syncthreads();
}
// ... with keeps_slot of the call's own block (spelled out, not an instance of the template: the third and fourth code objects stay bit for bit)
__device__ __forceinline__ void mark_tile(const ExportFilterArgs& a, const FilterSource& s, uint32_t j, uint64_t* s_word, uint32_t tid) {
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    for (uint32_t r = 0; r < kFilterRounds; ++r) {
        const uint32_t rbase = j * kExportFilterTile + r * kExportBlock;
        bool keep = false;
        if (rbase < s.n) {                                                        // uniform
            const uint32_t i = rbase + tid;
            if (i < s.n) keep = keeps_slot(a, s.plane, s.list[ring_index(s.head, i, a.capacity)]);
        }
        const uint64_t word = __ballot(keep);
        if (lane == 0u) s_word[r * kFilterWaves + wave] = word;
    }
    __syncthreads();
}

// s_word[kFilterWords] -> s_pref[w] = kept rows in the words before w; returns the tile's kept count. Ends behind a barrier.
__device__ __forceinline__ uint32_t tile_prefix(const uint64_t* s_word, uint32_t* s_pref, uint32_t* s_total, uint32_t tid) {
    if (tid < kFilterWords) {                                                     // wave 0
        const uint32_t c = (uint32_t)__popcll(s_word[tid]);
        uint32_t incl = c;
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, off, 64); if (tid >= off) incl += y; }
        s_pref[tid] = incl - c;
        if (tid == kFilterWords - 1u) *s_total = incl;
    }
    __syncthreads();
    return *s_total;
}

// The kept rows of tile j, by its mask in s_word and the prefix in s_pref, to order[first + rank]. A row is read from the list only when its bit is
// set; a bit is set only for rows below the count (mark_tile), and the test is made again here: nothing outside the list is read and nothing outside
// order[0, capacity) is written whatever the scratch holds.
__device__ __forceinline__ void compact_tile(const ExportFilterArgs& a, const FilterSource& s, uint32_t j, const uint64_t* s_word, const uint32_t* s_pref, uint32_t first, uint32_t tid) {
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    for (uint32_t r = 0; r < kFilterRounds; ++r) {
        const uint32_t rbase = j * kExportFilterTile + r * kExportBlock;
        if (rbase >= s.n) break;
        const uint32_t w = r * kFilterWaves + wave, i = rbase + tid;
        const uint64_t word = s_word[w];
        if (((word >> lane) & 1ull) && i < s.n) {
            const uint32_t at = first + s_pref[w] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
            if (at < a.capacity) a.order[at] = s.list[ring_index(s.head, i, a.capacity)];
        }
    }
}

// The filtered program export (hnb_export_filter_prog.hip): instance k's view of a call's argument block for mark_tile and compact_tile, as the
// effect form's kernels bind one effect - its sections of the scratch, kept[k] as the state word and, for per-instance filters, row k of the filter
// table. The rows come from filter_source(a.f, k): the view's slab and meta are the tables', not to be indexed by 0. k is uniform: everything here
// is scalar loads and scalar arithmetic; members are set one by one and P is indexed by constants only (keeps_slot_of_view), so the view lives in
// registers.
__device__ __forceinline__ ExportFilterArgs filter_instance_args(const ExportFilterProgArgs& a, uint32_t k) {
    ExportFilterArgs b;
    b.slab = a.f.slab;
    b.meta = a.f.meta;
    b.order = a.f.order + (size_t)k * a.order_pitch;
    b.mask = a.f.mask + (size_t)k * a.f.tiles * kFilterWords;
    b.tile_count = a.f.tile_count + (size_t)k * a.f.tiles;
    b.tile_offset = a.f.tile_offset + (size_t)k * a.f.tiles;
    b.state = a.f.state + (size_t)k * (sizeof(HnbDeviceMeta) / 4u);
    b.alive_off[0] = a.f.alive_off[0]; b.alive_off[1] = a.f.alive_off[1];
    b.plane_off = a.f.plane_off;
    b.capacity = a.f.capacity; b.tiles = a.f.tiles; b.kind = a.f.kind; b.is_f32 = a.f.is_f32;
    const bool own = a.filters != nullptr;
    const ExportFilterRow* r = a.filters + (own ? k : 0u);
    const uint32_t n_planes = own ? r->n_planes : a.f.n_planes;
    b.n_planes = n_planes < HNB_FILTER_MAX_PLANES ? n_planes : HNB_FILTER_MAX_PLANES;
    b.invert = own ? r->invert : a.f.invert;
    b.lo_bits = own ? r->lo_bits : a.f.lo_bits;
    b.hi_bits = own ? r->hi_bits : a.f.hi_bits;
#pragma unroll
    for (uint32_t i = 0; i < HNB_FILTER_MAX_PLANES; ++i)
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) b.P[i][c] = own ? r->P[i][c] : a.f.P[i][c];
    return b;
}

// keeps_slot for such a view: the same formulas, plane by plane with the plane's index a constant - filter_pass_planes over ONE plane gives that
// plane's sum and comparison, operation by operation, and the conjunction is the same.
__device__ __forceinline__ bool keeps_slot_of_view(const ExportFilterArgs& a, const uint32_t* __restrict__ plane, uint32_t slot) {
    bool pass;
    if (a.kind == HNB_FILTER_ATTR_RANGE) {
        pass = filter_pass_range(plane[slot], a.is_f32 != 0u, a.lo_bits, a.hi_bits);
    } else {
        const uint32_t* p = plane + (size_t)slot * 3u;
        const float x = __uint_as_float(p[0]), y = __uint_as_float(p[1]), z = __uint_as_float(p[2]);
        if (a.kind == HNB_FILTER_PLANES) {
            pass = true;
#pragma unroll
            for (uint32_t i = 0; i < HNB_FILTER_MAX_PLANES; ++i)
                if (i < a.n_planes) pass = filter_pass_planes(x, y, z, &a.P[i], 1u) && pass;
        } else pass = filter_pass_sphere(x, y, z, a.P[0]);
    }
    return pass != (a.invert != 0u);
}

}  // namespace
}  // namespace hnb
