// Sorted export (hnb_effect_export_sorted, include/hanabi_amd.h "Packed output"; DESIGN.md "Sorted export"): the alive particles of ONE effect as
// packed records in the order of a 32-bit key computed from their planes - depth along a direction, squared distance from a point, or a scalar
// attribute. A code object of its own, like hnb_export.hip: nothing here is part of the fat binary of libhanabi_amd.so.
//
// The simulation is only read: the alive list, the planes and the metadata row stay as they are, (key, slot) pairs live in scratch the library owns
// per effect. A stable least-significant-digit radix sort, 8 bits per pass, over tiles of 4096 rows with 256 lanes, the design of hnb_sort.hip.h:
//   k_export_sort_keys     row r: slot = list[ring(head, r)], key from plane[slot]; writes key[0][r], val[0][r]; in the same pass the tile's 256-bin
//                          counts of all four digits (LDS) -> hist[d][tile], added into gsum[0][d][tile / 32], and the OR of the keys and of their
//                          complements. A digit's per-tile counts describe the rows IN LIST ORDER: they serve the first pass that runs, whichever
//                          digit that is. (The counts of a later pass depend on where the earlier ones put the rows; knowing them in advance is what
//                          a decoupled look-back buys, and no workgroup here ever waits for another.)
//   k_export_sort_hist     in front of every later pass: its digit's per-tile counts of the rows as they lie now -> hist[d], gsum[1][d].
//   k_export_sort_scatter  once per digit: a tile derives its 256 digit offsets itself (digit totals and the groups before its own from gsum, the
//                          earlier tiles of its group from hist), ranks its keys stably (wave match by ballots, waves in order, rounds in order)
//                          and moves (key, slot) to the other buffer.
//   A pass whose digit is the same in every key (OR of keys & OR of complements has no bit in it) returns after two scalar loads, in both kernels;
//   which buffer a pass reads and which one holds the result follows from the passes that ran (export_sort_pass).
//   k_export_sort_tile     an effect of at most 4096 slots: keys, every pass and the state words by ONE workgroup in one launch.
//   k_export_sort_rows_*   the gather of hnb_export_rows.hip.h with slot = order[r].
// hnb_program_export_sorted (DESIGN.md "Sorted export, program form") runs the same bodies for every instance of a program:
//   k_export_sort_*_inst   instance scope: instance = blockIdx.y, in its own section of every buffer, by its own meta row and state words.
//   k_export_sort_fill, _hist_all, _scatter_all   program scope: all instances' rows as one space, values name (instance, slot).
//   k_export_sort_rows_inst_* / _all_*   their gathers.
// Every loop is bounded by the capacity; every grid is sized from it, and workgroups past alive_count leave after the scalar loads.
#include <hip/hip_runtime.h>

#include "hnb_export_sort.hip.h"   // the rows and buffers of a sort kernel, the key of a slot, the tile primitives, the keys and one-workgroup bodies

#pragma clang fp contract(off)   // the key arithmetic is rounded operation by operation (the unit is also built with -ffp-contract=off)

using namespace hnb;

namespace {

constexpr uint32_t kBlock = kExportBlock;
constexpr uint32_t kWaves = kSortWaves;
constexpr uint32_t kRounds = kSortRounds;

// kSortGlobal: in front of EVERY pass that runs, the first included (the fill kernel's tiles are not the passes': it leaves no counts), into set 1.
template <uint32_t MODE>
__device__ __forceinline__ void sort_hist_body(const ExportSortArgs& a, uint32_t pass) {
    __shared__ uint32_t s_hist[256];
    const SortView v = sort_view<MODE>(a);
    const ExportSortPass sp = export_sort_pass(v.state->or_keys & v.state->or_not_keys, pass);
    if (!sp.active || (MODE != kSortGlobal && sp.ran == 0u)) return;              // (the first pass that runs has the keys kernel's counts)
    const uint32_t j = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t n = sort_rows<MODE>(a);
    if (j >= a.tiles || j * kExportSortTile >= n) return;
    s_hist[tid] = 0u;
    __syncthreads();
    const uint32_t* skey = v.keys + (size_t)sp.src * a.pitch;
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t rbase = j * kExportSortTile + r * kBlock;
        if (rbase >= n) break;
        const uint32_t i = rbase + tid;
        const bool valid = i < n;
        const uint32_t key = valid ? skey[i] : 0u;
        hist_add(s_hist, (key >> (8u * pass)) & 0xffu, valid, lane);
    }
    __syncthreads();
    const uint32_t c = s_hist[tid];
    v.hist[((size_t)pass * a.tiles + j) * 256u + tid] = c;
    if (c) atomicAdd(v.gsum + ((size_t)(kExportSortPasses + pass) * a.groups + j / kExportSortGroup) * 256u + tid, c);
}

template <uint32_t MODE>
__device__ __forceinline__ void sort_scatter_body(const ExportSortArgs& a, uint32_t pass) {
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_cnt[kWaves][256];
    const SortView v = sort_view<MODE>(a);
    const ExportSortPass sp = export_sort_pass(v.state->or_keys & v.state->or_not_keys, pass);
    if (!sp.active) return;
    const uint32_t j = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = sort_rows<MODE>(a);
    if (j >= a.tiles || j * kExportSortTile >= n) return;
    const uint32_t* skey = v.keys + (size_t)sp.src * a.pitch;
    const uint32_t* sval = v.vals + (size_t)sp.src * a.pitch;
    uint32_t* dkey = v.keys + (size_t)(sp.src ^ 1u) * a.pitch;
    uint32_t* dval = v.vals + (size_t)(sp.src ^ 1u) * a.pitch;
    {   // offset(d, j) = sum_{d' < d} total(d') + sum_{groups before mine} gsum(g, d) + sum_{earlier tiles of my group} hist(j', d)
        const uint32_t used_groups = ((n + kExportSortTile - 1u) / kExportSortTile + kExportSortGroup - 1u) / kExportSortGroup;   // groups holding rows; <= a.groups
        const uint32_t* gs = v.gsum + (size_t)((MODE == kSortGlobal || sp.ran ? kExportSortPasses : 0u) + pass) * a.groups * 256u;
        const uint32_t* hist = v.hist + (size_t)pass * a.tiles * 256u;
        const uint32_t my_group = j / kExportSortGroup;
        uint32_t total = 0, before = 0;
        for (uint32_t g = 0; g < used_groups; ++g) { const uint32_t c = gs[(size_t)g * 256u + tid]; total += c; if (g < my_group) before += c; }
        for (uint32_t t = my_group * kExportSortGroup; t < j; ++t) before += hist[(size_t)t * 256u + tid];
        const uint32_t digit_base = digit_scan(total, s_base, lane, wave);
        s_base[tid] = digit_base + before;
    }
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) s_cnt[w][tid] = 0u;
    __syncthreads();
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t rbase = j * kExportSortTile + r * kBlock;
        if (rbase >= n) break;
        const uint32_t i = rbase + tid;
        const bool valid = i < n;
        scatter_round(valid ? skey[i] : 0u, valid ? sval[i] : 0u, valid, 8u * pass, s_base, s_cnt, dkey, dval, n, tid, lane, wave);
    }
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_export_sort_keys(const ExportSortArgs a) { sort_keys_body<kSortEffect>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_hist(const ExportSortArgs a, uint32_t pass) { sort_hist_body<kSortEffect>(a, pass); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_scatter(const ExportSortArgs a, uint32_t pass) { sort_scatter_body<kSortEffect>(a, pass); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_tile(const ExportSortArgs a) { sort_tile_body<kSortEffect>(a); }

// ---- hnb_program_export_sorted, instance scope: the kernels above over (tiles, instances) ----
extern "C" __global__ void __launch_bounds__(256) k_export_sort_keys_inst(const ExportSortArgs a) { sort_keys_body<kSortBatch>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_hist_inst(const ExportSortArgs a, uint32_t pass) { sort_hist_body<kSortBatch>(a, pass); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_scatter_inst(const ExportSortArgs a, uint32_t pass) { sort_scatter_body<kSortBatch>(a, pass); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_tile_inst(const ExportSortArgs a) { sort_tile_body<kSortBatch>(a); }

// ---- hnb_program_export_sorted, program scope: one row space of offsets[n_inst] rows ----
// Grid (tiles of an instance, instances): row r of instance k -> position offsets[k] + r of buffer 0, the value names (k, slot); the OR words. An
// instance's rows start wherever the instances before it end, not on a tile of the passes: no digit counts are left, k_export_sort_hist_all runs
// in front of every pass.
extern "C" __global__ void __launch_bounds__(256) k_export_sort_fill(const ExportSortArgs a) {
    const uint32_t j = blockIdx.x, k = blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
    if (k >= a.n_inst) return;
    const SortSource s = sort_source(a, k);
    if (j * kExportSortTile >= s.n) return;
    const uint32_t first = a.offsets[k];
    uint32_t ork = 0u, ornk = 0u;
    for (uint32_t r = 0; r < kRounds; ++r) {
        const uint32_t rbase = j * kExportSortTile + r * kBlock;
        if (rbase >= s.n) break;
        const uint32_t i = rbase + tid;
        const uint64_t at = (uint64_t)first + i;
        if (i < s.n && at < (uint64_t)a.total_cap) {                              // (offsets are sums of counts <= capacity: always inside; the buffers hold total_cap rows)
            const uint32_t slot = s.list[ring_index(s.head, i, a.capacity)];
            const uint32_t key = key_of_slot(a, s.plane, slot);
            a.keys[at] = key;
            a.vals[at] = export_sort_pack(k, slot, a.slot_bits);
            ork |= key; ornk |= ~key;
        }
    }
    ork = wave_or(ork); ornk = wave_or(ornk);
    if (lane == 0u && (ork | ornk)) { atomicOr(&a.state->or_keys, ork); atomicOr(&a.state->or_not_keys, ornk); }
}
extern "C" __global__ void __launch_bounds__(256) k_export_sort_hist_all(const ExportSortArgs a, uint32_t pass) { sort_hist_body<kSortGlobal>(a, pass); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_scatter_all(const ExportSortArgs a, uint32_t pass) { sort_scatter_body<kSortGlobal>(a, pass); }

extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_sort_rows_32(const ExportArgs a) { export_rows<256u * 32u / 4u, true>(a); }
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_sort_rows_64(const ExportArgs a) { export_rows<256u * 64u / 4u, true>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_rows_128(const ExportArgs a) { export_rows<256u * 128u / 4u, true>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_rows_256(const ExportArgs a) { export_rows<128u * 256u / 4u, true>(a); }

extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_sort_rows_inst_32(const ExportArgs a) { export_rows<256u * 32u / 4u, kRowsOrderedInstance>(a); }
extern "C" __global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) k_export_sort_rows_inst_64(const ExportArgs a) { export_rows<256u * 64u / 4u, kRowsOrderedInstance>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_rows_inst_128(const ExportArgs a) { export_rows<256u * 128u / 4u, kRowsOrderedInstance>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_rows_inst_256(const ExportArgs a) { export_rows<128u * 256u / 4u, kRowsOrderedInstance>(a); }
// (a slab base per lane on top of the four fields in flight: the 64-register budget of the _32 / _64 gathers above would spill)
extern "C" __global__ void __launch_bounds__(256) k_export_sort_rows_all_32(const ExportArgs a) { export_rows<256u * 32u / 4u, kRowsOrderedProgram>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_rows_all_64(const ExportArgs a) { export_rows<256u * 64u / 4u, kRowsOrderedProgram>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_rows_all_128(const ExportArgs a) { export_rows<256u * 128u / 4u, kRowsOrderedProgram>(a); }
extern "C" __global__ void __launch_bounds__(256) k_export_sort_rows_all_256(const ExportArgs a) { export_rows<128u * 256u / 4u, kRowsOrderedProgram>(a); }
