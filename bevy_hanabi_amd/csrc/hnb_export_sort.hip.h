// The pieces of the sorted export's kernels (hnb_export_sort.hip) that the filtered-then-sorted export (hnb_export_cull.hip) runs as well: where a
// sort kernel's rows and buffers are, the key of a slot, the digit counting, scanning and ranking of a tile, and the bodies of the keys kernel (generic
// over where row i's slot comes from) and of the one-workgroup sort. Included by both units; the design is described in hnb_export_sort.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "hnb_export_rows.hip.h"

#pragma clang fp contract(off)   // the key arithmetic is rounded operation by operation (the units are also built with -ffp-contract=off)

namespace hnb {
namespace {

constexpr uint32_t kSortWaves = kExportBlock / 64u;
constexpr uint32_t kSortRounds = kExportSortTile / kExportBlock;

// Which rows a sort kernel works on. kSortEffect: one effect (hnb_effect_export_sorted), everything as ExportSortArgs describes it. kSortBatch: the
// instance scope of hnb_program_export_sorted, instance blockIdx.y in its own section of every buffer, by its own meta row and state words.
// kSortGlobal: the program scope, the rows of all instances as one space of offsets[n_inst] rows.
constexpr uint32_t kSortEffect = 0, kSortBatch = 1, kSortGlobal = 2;

struct SortView {
    uint32_t* keys;
    uint32_t* vals;
    uint32_t* hist;
    uint32_t* gsum;
    ExportSortState* state;
};

template <uint32_t MODE>
__device__ __forceinline__ SortView sort_view(const ExportSortArgs& a) {
    SortView v = {a.keys, a.vals, a.hist, a.gsum, a.state};
    if constexpr (MODE == kSortBatch) {
        const size_t k = blockIdx.y;
        v.keys += k * 2u * a.pitch;
        v.vals += k * 2u * a.pitch;
        v.hist += k * kExportSortPasses * a.tiles * 256u;
        v.gsum += k * 2u * kExportSortPasses * a.groups * 256u;
        v.state += k;
    }
    return v;
}

// rows to sort: uniform (scalar loads)
template <uint32_t MODE>
__device__ __forceinline__ uint32_t sort_rows(const ExportSortArgs& a) {
    if constexpr (MODE == kSortGlobal) {
        const uint32_t all = a.offsets[a.n_inst];
        return all < a.total_cap ? all : a.total_cap;
    } else {
        const uint32_t alive = a.meta[MODE == kSortBatch ? blockIdx.y : 0u].alive_count;
        return alive < a.capacity ? alive : a.capacity;
    }
}

// The rows of a keys kernel: n of them, row i names slot(i, capacity) of the key plane. SortSource: the alive list behind its head.
struct SortSource {
    const uint32_t* list;
    const uint32_t* plane;
    uint32_t head, n;
    __device__ __forceinline__ uint32_t slot(uint32_t i, uint32_t capacity) const { return list[ring_index(head, i, capacity)]; }
};

__device__ __forceinline__ SortSource sort_source(const ExportSortArgs& a, uint32_t k = 0u) {
    const HnbDeviceMeta m = a.meta[k];                                            // uniform: scalar loads
    const char* base = reinterpret_cast<const char*>(a.slab[k]);
    SortSource s;
    s.list = reinterpret_cast<const uint32_t*>(base + a.alive_off[m.list_column & 1u]);
    s.plane = reinterpret_cast<const uint32_t*>(base + a.plane_off);
    s.head = m.list_column >> 1;
    s.n = m.alive_count < a.capacity ? m.alive_count : a.capacity;
    return s;
}

// include/hanabi_amd.h states these formulas; every operation is rounded on its own, in this order.
__device__ __forceinline__ uint32_t key_of_slot(const ExportSortArgs& a, const uint32_t* __restrict__ plane, uint32_t slot) {
    if (a.key == HNB_SORT_KEY_ATTR) return sort_key_of(plane[slot], a.is_f32 != 0u, a.descending != 0u);
    const uint32_t* p = plane + (size_t)slot * 3u;
    const float x = __uint_as_float(p[0]), y = __uint_as_float(p[1]), z = __uint_as_float(p[2]);
    float d;
    if (a.key == HNB_SORT_KEY_DEPTH) {
        const float xy = x * a.v[0] + y * a.v[1];
        d = xy + z * a.v[2];
    } else {
        const float ex = x - a.v[0], ey = y - a.v[1], ez = z - a.v[2];
        const float xy = ex * ex + ey * ey;
        d = xy + ez * ez;
    }
    return sort_key_of(__float_as_uint(d), true, a.descending != 0u);
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
    for (uint32_t off = 32; off > 0; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

// One round's digits into a 256-bin LDS histogram. Called by whole waves; the valid lanes of a wave are its first ones. A wave whose valid lanes
// all hold one digit (the upper bytes of most keys; a constant key) adds once instead of queueing 64 atomics on one bank.
__device__ __forceinline__ void hist_add(uint32_t* h, uint32_t digit, bool valid, uint32_t lane) {
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)digit);
    if (__ballot(valid && digit != first) == 0ull) {
        const uint32_t cnt = (uint32_t)__popcll(__ballot(valid));
        if (lane == 0u && cnt) atomicAdd(&h[first], cnt);
    } else if (valid) {
        atomicAdd(&h[digit], 1u);
    }
}

// 256 digit totals (thread d holds digit d's) -> their exclusive prefix sum; s_tmp: kSortWaves words of LDS. Ends behind a barrier.
__device__ __forceinline__ uint32_t digit_scan(uint32_t total, uint32_t* s_tmp, uint32_t lane, uint32_t wave) {
    uint32_t incl = total;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)incl, off, 64); if (lane >= off) incl += y; }
    __syncthreads();
    if (lane == 63u) s_tmp[wave] = incl;
    __syncthreads();
    uint32_t base = incl - total;
    for (uint32_t w = 0; w < wave; ++w) base += s_tmp[w];
    __syncthreads();
    return base;
}

// One round of 256 rows of a scatter pass: stable ranks by wave match, then the move. s_base[d]: where digit d's next row goes; s_cnt: [kSortWaves][256],
// zero on entry and on exit. Ends behind a barrier. Every destination is below n: the bases come from counts of these same keys.
__device__ __forceinline__ void scatter_round(uint32_t key, uint32_t val, bool valid, uint32_t shift, uint32_t* s_base, uint32_t (*s_cnt)[256], uint32_t* dkey, uint32_t* dval,
                                              uint32_t n, uint32_t tid, uint32_t lane, uint32_t wave) {
    const uint32_t digit = (key >> shift) & 0xffu;
    uint64_t same = __ballot(valid);                                              // lanes of this wave holding the same digit (stable: earlier lanes first)
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        same &= bit ? bal : ~bal;
    }
    const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank == 0u) s_cnt[wave][digit] = (uint32_t)__popcll(same);
    __syncthreads();
    if (valid) {
        uint32_t off = s_base[digit] + rank;
        for (uint32_t w = 0; w < wave; ++w) off += s_cnt[w][digit];
        if (off < n) { dkey[off] = key; dval[off] = val; }
    }
    __syncthreads();
    uint32_t add = 0;                                                             // thread d advances digit d's base past this round and clears the round's counters
#pragma unroll
    for (uint32_t w = 0; w < kSortWaves; ++w) { add += s_cnt[w][tid]; s_cnt[w][tid] = 0u; }
    s_base[tid] += add;
    __syncthreads();
}

// The keys kernel of a multi-tile sort over the rows `s` names (SortSource: the alive list; hnb_export_cull.hip: the rows a filter kept): tile
// blockIdx.x's keys and slots into buffer 0, its counts of all four digits into hist and gsum set 0, the OR words.
template <uint32_t MODE, class Rows>
__device__ __forceinline__ void sort_keys_rows(const ExportSortArgs& a, const Rows& s) {
    __shared__ uint32_t s_hist[kExportSortPasses][256];
    const uint32_t j = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const SortView v = sort_view<MODE>(a);
    if (j >= a.tiles || j * kExportSortTile >= s.n) return;
#pragma unroll
    for (uint32_t d = 0; d < kExportSortPasses; ++d) s_hist[d][tid] = 0u;
    __syncthreads();
    uint32_t ork = 0u, ornk = 0u;
    for (uint32_t r = 0; r < kSortRounds; ++r) {
        const uint32_t rbase = j * kExportSortTile + r * kExportBlock;
        if (rbase >= s.n) break;
        const uint32_t i = rbase + tid;
        const bool valid = i < s.n;
        uint32_t key = 0u;
        if (valid) {
            const uint32_t slot = s.slot(i, a.capacity);
            key = key_of_slot(a, s.plane, slot);
            v.keys[i] = key;
            v.vals[i] = slot;
            ork |= key; ornk |= ~key;
        }
#pragma unroll
        for (uint32_t d = 0; d < kExportSortPasses; ++d) hist_add(s_hist[d], (key >> (8u * d)) & 0xffu, valid, lane);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t d = 0; d < kExportSortPasses; ++d) {
        const uint32_t c = s_hist[d][tid];
        v.hist[((size_t)d * a.tiles + j) * 256u + tid] = c;
        if (c) atomicAdd(v.gsum + ((size_t)d * a.groups + j / kExportSortGroup) * 256u + tid, c);
    }
    ork = wave_or(ork); ornk = wave_or(ornk);
    if (lane == 0u) { atomicOr(&v.state->or_keys, ork); atomicOr(&v.state->or_not_keys, ornk); }
}

template <uint32_t MODE>
__device__ __forceinline__ void sort_keys_body(const ExportSortArgs& a) { sort_keys_rows<MODE>(a, sort_source(a, MODE == kSortBatch ? blockIdx.y : 0u)); }

// A one-workgroup sort of n rows: fill(v, ork, ornk) writes every lane's share of the (key, slot) pairs to buffer 0 and ORs the keys and their
// complements into its two words; then the state words for the gather and every active pass. The passes communicate through the key / value buffers in
// global memory as they do across launches (a workgroup sees its own stores behind a barrier).
// BY_COUNT: the passes' loops run over the rounds that hold rows, a count known at run time, instead of all kSortRounds with a test in front of each.
// The compiler unrolls the fixed form and keeps the sixteen rounds' two tests each in scalar registers across the passes - 64 of them, which the
// plain sort affords (with eight of them parked in a vector register's lanes) and a kernel with a filter's arguments in front does not.
template <uint32_t MODE, bool BY_COUNT, class Fill>
__device__ __forceinline__ void sort_tile_rows(const ExportSortArgs& a, uint32_t n, const Fill& fill) {
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_cnt[kSortWaves][256];
    __shared__ uint32_t s_or[2][kSortWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const SortView v = sort_view<MODE>(a);
    const uint32_t rounds = BY_COUNT ? (n + kExportBlock - 1u) / kExportBlock : kSortRounds;
    uint32_t ork = 0u, ornk = 0u;
    fill(v, ork, ornk);
    ork = wave_or(ork); ornk = wave_or(ornk);
    if (lane == 0u) { s_or[0][wave] = ork; s_or[1][wave] = ornk; }
    __syncthreads();
    ork = 0u; ornk = 0u;
#pragma unroll
    for (uint32_t w = 0; w < kSortWaves; ++w) { ork |= s_or[0][w]; ornk |= s_or[1][w]; }
    if (tid == 0u) { v.state->or_keys = ork; v.state->or_not_keys = ornk; }
    const uint32_t varying = ork & ornk;
    if (n == 0u || varying == 0u) return;
    uint32_t src = 0u;
    for (uint32_t pass = 0; pass < kExportSortPasses; ++pass) {
        if (((varying >> (8u * pass)) & 0xffu) == 0u) continue;
        const uint32_t* skey = v.keys + (size_t)src * a.pitch;
        const uint32_t* sval = v.vals + (size_t)src * a.pitch;
        uint32_t* dkey = v.keys + (size_t)(src ^ 1u) * a.pitch;
        uint32_t* dval = v.vals + (size_t)(src ^ 1u) * a.pitch;
        s_base[tid] = 0u;
#pragma unroll
        for (uint32_t w = 0; w < kSortWaves; ++w) s_cnt[w][tid] = 0u;
        __syncthreads();
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t rbase = r * kExportBlock;
            if (rbase >= n) break;
            const bool valid = rbase + tid < n;
            hist_add(s_base, ((valid ? skey[rbase + tid] : 0u) >> (8u * pass)) & 0xffu, valid, lane);
        }
        __syncthreads();
        const uint32_t total = s_base[tid];
        const uint32_t digit_base = digit_scan(total, s_or[0], lane, wave);
        s_base[tid] = digit_base;
        __syncthreads();
        for (uint32_t r = 0; r < rounds; ++r) {
            const uint32_t rbase = r * kExportBlock;
            if (rbase >= n) break;
            const uint32_t i = rbase + tid;
            const bool valid = i < n;
            scatter_round(valid ? skey[i] : 0u, valid ? sval[i] : 0u, valid, 8u * pass, s_base, s_cnt, dkey, dval, n, tid, lane, wave);
        }
        src ^= 1u;   // (== export_sort_pass(varying, pass + 1).src: the gather finds the result where the multi-launch path leaves it)
    }
}

// Instances of at most kExportSortTile slots: the whole sort of one by one workgroup in one launch; the rows are the alive list's.
template <uint32_t MODE>
__device__ __forceinline__ void sort_tile_body(const ExportSortArgs& a) {
    const SortSource s = sort_source(a, MODE == kSortBatch ? blockIdx.y : 0u);
    const uint32_t n = s.n < kExportSortTile ? s.n : kExportSortTile;             // (capacity <= kExportSortTile: the host launches this kernel for nothing else)
    sort_tile_rows<MODE, false>(a, n, [&](const SortView& v, uint32_t& ork, uint32_t& ornk) {
        for (uint32_t r = 0; r < kSortRounds; ++r) {
            const uint32_t i = r * kExportBlock + threadIdx.x;
            if (i >= n) break;
            const uint32_t slot = s.slot(i, a.capacity);
            const uint32_t key = key_of_slot(a, s.plane, slot);
            v.keys[i] = key;
            v.vals[i] = slot;
            ork |= key; ornk |= ~key;
        }
    });
}

}  // namespace
}  // namespace hnb
