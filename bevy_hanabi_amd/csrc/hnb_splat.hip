// The splat (hnb_effect_splat, hnb_program_splat, include/hanabi_amd_splat.h; DESIGN.md "Splat"): the deposit with the sample's stencil - the alive
// particles of an instance summed into a dense uniform grid, every inside particle spread over the eight cell centres around it. A code object of its
// own, like the deposit's: nothing here is part of the fat binary of libhanabi_amd.so. A sum of integers does not depend on the order, so nothing
// reads the alive list: the walk is the deposit's (hnb_deposit.hip deposit_tile) - a lane takes four quads of consecutive slots per tile, one 4-byte
// load of their alive bytes each, requested ahead, and, unless all four are zero, POSITION's 48 bytes. Then slot by slot: the cell (its count), for an
// inside particle the three axes and the eight (row, weight) pairs (hnb_splat.h splat_axis, splat_corners), and channel by channel one value load,
// the deposit's acceptance on the stored value and eight integer adds (an outside particle: the deposit's one add into row n_cells). One slot's
// corners and one channel's value are live at a time.
//   k_splat_lds     workgroup (g, k): tiles [span g, span g + span) of instance k into a table of its own in LDS (32-bit adds for the counts, 64-bit
//                   adds for the sums), then the table's non-zero entries onto count / sums, lane i entry i of every 256: consecutive addresses.
//   k_splat_global  workgroup (j, k): tile j of instance k, one add per particle onto count and eight per accepted contribution onto sums.
// Every add is a vector atomic whose result is not used (agent scope, relaxed: the call's results are read behind it in stream order). Integer adds
// commute: both kernels and every grouping give the same bits. The simulation is only read. Every loop is bounded by the span, the table's size, 8
// or 4; every grid is sized from host-known numbers; no workgroup waits for another; an instance with nothing alive leaves after the scalar loads.
// A cell is at most n_cells (bin_cell_of) and a corner row below n_cells (sample_axis: both corners of an axis lie in 0 .. dim - 1), so every entry
// addressed lies inside the (n_cells + 1) rows of the table.
#include <hip/hip_runtime.h>

#include "hnb_splat.h"

#pragma clang fp contract(off)   // (the cell, the weights and the products are f32 arithmetic stated operation by operation: hnb_splat.h)

using namespace hnb;

namespace {

struct LaneStats { uint32_t visited, outside, rejected; };

__device__ __forceinline__ void add_u32(uint32_t* p, uint32_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void add_u64(uint64_t* p, uint64_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lds_add_u32(uint32_t* p, uint32_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_add_u64(uint64_t* p, uint64_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

template <bool LDS>
__device__ __forceinline__ void sum_add(uint64_t* p, int64_t q) {
    if (LDS) lds_add_u64(p, (uint64_t)q); else add_u64(p, (uint64_t)q);
}

// One alive slot at (x, y, z). LDS: count / sums are the workgroup's table, else the call's.
template <bool LDS>
__device__ __forceinline__ void splat_slot(const SplatArgs& a, const char* base, uint32_t* count, uint64_t* sums, uint32_t slot, float x, float y, float z, LaneStats& st) {
    const uint32_t cell = bin_cell_of(a.grid, x, y, z);                  // <= n_cells
    const bool inside = cell != a.grid.n_cells;
    if (LDS) lds_add_u32(count + cell, 1u); else add_u32(count + cell, 1u);
    st.visited += 1u;
    st.outside += inside ? 0u : 1u;
    const uint32_t nch = a.n_channels;
    if (nch == 0u) return;                                               // (the same in every lane)
    SplatCorners c = {};
    if (inside) {
        const SplatAxis ax = splat_axis(sample_axis_t(x, a.grid.origin[0], a.grid.inv_cell[0]), a.grid.dims[0]);
        const SplatAxis ay = splat_axis(sample_axis_t(y, a.grid.origin[1], a.grid.inv_cell[1]), a.grid.dims[1]);
        const SplatAxis az = splat_axis(sample_axis_t(z, a.grid.origin[2], a.grid.inv_cell[2]), a.grid.dims[2]);
        c = splat_corners(a.grid.dims, ax, ay, az);                      // every row < n_cells
    }
#pragma unroll 1
    for (uint32_t k = 0; k < nch; ++k) {                                 // (one channel's scalars and one value at a time)
        const uint32_t packed = a.ch[k].packed, nc = deposit_channel_ncomp(packed), comp = deposit_channel_comp(packed), frac = deposit_channel_frac_bits(packed);
        uint32_t v = kSplatOneBits;
        if (!splat_channel_is_one(packed)) v = reinterpret_cast<const uint32_t*>(base + a.ch[k].plane_off)[(uint64_t)slot * nc + comp];   // (slot < capacity)
        const DepositQuant q = deposit_quantise(v, frac);
        if (!q.ok) { st.rejected += 1u; continue; }                      // tested once, on the stored value: nothing of the pair is added
        if (!inside) { sum_add<LDS>(sums + ((size_t)cell * nch + k), q.q); continue; }     // the deposit's contribution, into row n_cells
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) sum_add<LDS>(sums + ((size_t)c.row[i] * nch + k), splat_contribution(v, c.w[i], frac));
    }
}

// Slots [first, first + 4096) below the capacity of one instance, four quads per lane: quad q = round * 256 + tid, so that a wave's loads of one
// round are consecutive. The alive bytes of all four quads are requested before the first plane load. A quad that reaches past the capacity is
// taken slot by slot with 4-byte loads: nothing is read behind the last slot's components.
template <bool LDS>
__device__ __forceinline__ void splat_tile(const SplatArgs& a, const char* base, uint32_t* count, uint64_t* sums, uint32_t first, uint32_t tid, LaneStats& st) {
    const char* flags = base + a.flag_off;
    const char* pos_plane = base + a.pos_off;
    const uint32_t cap = a.capacity;
    uint32_t f[4];
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t s0 = first + (r * kSplatBlock + tid) * 4u;        // (first + 4095 < 2^32: a tile starts below the capacity)
        // the four alive bytes of a quad that starts below the capacity lie inside the bytes' section: it is a multiple of 256 bytes long
        f[r] = s0 < cap ? *reinterpret_cast<const uint32_t*>(flags + s0) : 0u;
    }
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t s0 = first + (r * kSplatBlock + tid) * 4u;
        if (f[r] == 0u) continue;                                        // four free slots (or none below the capacity): no plane is read
        const bool quad = cap - s0 >= 4u;
        const uint32_t n = quad ? 4u : cap - s0;                         // (1..3: the capacity's last slots)
        uint32_t alive = 0u, p[12] = {};
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) alive |= (t < n && ((f[r] >> (8u * t)) & 0xffu) != 0u) ? 1u << t : 0u;
        if (quad) {
            const uint4* src = reinterpret_cast<const uint4*>(pos_plane + (uint64_t)s0 * 12u);     // 16-byte aligned: s0 is a multiple of 4, the plane of 256
#pragma unroll
            for (uint32_t i = 0; i < 3u; ++i) {
                const uint4 q = src[i];
                p[4u * i] = q.x; p[4u * i + 1u] = q.y; p[4u * i + 2u] = q.z; p[4u * i + 3u] = q.w;
            }
        } else {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(pos_plane + (uint64_t)s0 * 12u);
#pragma unroll
            for (uint32_t i = 0; i < 9u; ++i)
                if (i < 3u * n) p[i] = src[i];
        }
#pragma unroll 1
        for (uint32_t t = 0; t < 4u; ++t) {                              // one slot at a time; its position picked by t, which every lane shares
            if (((alive >> t) & 1u) == 0u) continue;                     // (an alive bit is set for slots below the capacity alone)
            const uint32_t xb = t == 0u ? p[0] : t == 1u ? p[3] : t == 2u ? p[6] : p[9];
            const uint32_t yb = t == 0u ? p[1] : t == 1u ? p[4] : t == 2u ? p[7] : p[10];
            const uint32_t zb = t == 0u ? p[2] : t == 1u ? p[5] : t == 2u ? p[8] : p[11];
            splat_slot<LDS>(a, base, count, sums, s0 + t, __uint_as_float(xb), __uint_as_float(yb), __uint_as_float(zb), st);
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// A wave's three numbers onto out_stats: one add per wave and non-zero number
__device__ __forceinline__ void add_stats(const SplatArgs& a, const LaneStats& st, uint32_t tid) {
    if (!a.stats) return;
    const uint32_t v = wave_sum(st.visited), o = wave_sum(st.outside), r = wave_sum(st.rejected);
    if ((tid & 63u) == 0u) {
        if (v != 0u) add_u32(a.stats, v);
        if (o != 0u) add_u32(a.stats + 1, o);
        if (r != 0u) add_u32(a.stats + 2, r);
    }
}

__device__ __forceinline__ void lds_body(const SplatArgs& a, uint64_t* s_tab, uint32_t g, uint32_t k, uint32_t tid) {
    const uint32_t entries = a.grid.n_cells + 1u, n_sums = entries * a.n_channels;   // (the plan: entries * (4 + 8 n_channels) bytes are within kDepositLdsBudget)
    uint32_t* s_count = reinterpret_cast<uint32_t*>(s_tab + n_sums);
    for (uint32_t i = tid; i < n_sums; i += kSplatBlock) s_tab[i] = 0u;
    for (uint32_t i = tid; i < entries; i += kSplatBlock) s_count[i] = 0u;
    __syncthreads();
    LaneStats st = {0u, 0u, 0u};
    const char* base = reinterpret_cast<const char*>(a.slabs[k]);
    const uint32_t j0 = g * a.span, j1 = a.tiles - j0 < a.span ? a.tiles : j0 + a.span;    // (g < groups: j0 < tiles)
    for (uint32_t j = j0; j < j1; ++j) splat_tile<true>(a, base, s_count, s_tab, j * kSplatTile, tid, st);
    __syncthreads();
    for (uint32_t i = tid; i < n_sums; i += kSplatBlock) {
        const uint64_t s = s_tab[i];
        if (s != 0u) add_u64(a.sums + i, s);
    }
    for (uint32_t i = tid; i < entries; i += kSplatBlock) {
        const uint32_t c = s_count[i];
        if (c != 0u) add_u32(a.count + i, c);
    }
    add_stats(a, st, tid);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_splat_lds(const SplatArgs a) {
    extern __shared__ uint64_t s_tab[];                                   // the sums' rows, the counts behind them: SplatPlan::lds_bytes
    const uint32_t g = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    if (k >= a.n_inst || g >= a.groups) return;
    if (a.meta[k].alive_count == 0u) return;                              // nothing alive: no slot is read, nothing is added
    lds_body(a, s_tab, g, k, tid);
}

extern "C" __global__ void __launch_bounds__(256) k_splat_global(const SplatArgs a) {
    const uint32_t j = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    if (k >= a.n_inst || j >= a.tiles) return;
    if (a.meta[k].alive_count == 0u) return;
    LaneStats st = {0u, 0u, 0u};
    splat_tile<false>(a, reinterpret_cast<const char*>(a.slabs[k]), a.count, a.sums, j * kSplatTile, tid, st);
    add_stats(a, st, tid);
}
