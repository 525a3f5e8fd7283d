// The pieces of the filtered export's kernels (hnb_export_filter.hip) that the filtered-then-sorted export (hnb_export_cull.hip) runs as well: the rows
// a filter kernel reads, the predicate of a slot, a tile's mask and the prefix of its words. Included by both units; the design is described in
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

__device__ __forceinline__ FilterSource filter_source(const ExportFilterArgs& a) {
    const HnbDeviceMeta m = a.meta[0];                                            // uniform: scalar loads
    const char* base = reinterpret_cast<const char*>(a.slab[0]);
    FilterSource s;
    s.list = reinterpret_cast<const uint32_t*>(base + a.alive_off[m.list_column & 1u]);
    s.plane = reinterpret_cast<const uint32_t*>(base + a.plane_off);
    s.head = m.list_column >> 1;
    s.n = m.alive_count < a.capacity ? m.alive_count : a.capacity;
    return s;
}

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

}  // namespace
}  // namespace hnb
