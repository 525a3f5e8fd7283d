// The deposit (hnb_effect_deposit, hnb_program_deposit, include/hanabi_amd_deposit.h; DESIGN.md "Deposit"): the alive particles of an instance summed
// into a dense uniform grid - per cell a count and, per channel, the fixed-point sum of one component of an f32 attribute. A code object of its own,
// like the bounds': nothing here is part of the fat binary of libhanabi_amd.so. A sum of integers does not depend on the order, so nothing reads the
// alive list: the walk is over the SLOTS, the bounds' (hnb_bounds.hip fold_tile) - a lane takes four quads of consecutive slots per tile, one 4-byte
// load of their alive bytes each, requested ahead, and, unless all four are zero, POSITION's 48 bytes and the channels' components.
//   k_deposit_lds     workgroup (g, k): tiles [span g, span g + span) of instance k into a table of its own in LDS (32-bit adds for the counts, 64-bit
//                     adds for the sums), then the table's non-zero entries onto count / sums, lane i entry i of every 256: consecutive addresses.
//   k_deposit_global  workgroup (j, k): tile j of instance k, one add per particle onto count and one per accepted contribution onto sums.
// Every add is a vector atomic whose result is not used (agent scope, relaxed: the call's results are read behind it in stream order). Integer adds
// commute: both kernels and every grouping give the same bits. The simulation is only read. Every loop is bounded by the capacity, the span or the
// table's size; every grid is sized from host-known numbers; no workgroup waits for another; an instance with nothing alive leaves after the scalar
// loads. A cell is at most n_cells (bin_cell_of), so every entry addressed lies inside the (n_cells + 1) rows of the table.
#include <hip/hip_runtime.h>

#include "hnb_deposit.h"

#pragma clang fp contract(off)   // (the cell of a particle is f32 arithmetic stated operation by operation: hnb_bin_cell.h)

using namespace hnb;

namespace {

struct LaneStats { uint32_t deposited, outside, rejected; };

__device__ __forceinline__ void add_u32(uint32_t* p, uint32_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void add_u64(uint64_t* p, uint64_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void lds_add_u32(uint32_t* p, uint32_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_add_u64(uint64_t* p, uint64_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// The cells of up to four slots that were loaded together (alive: a bit per slot): the counts, then channel by channel the accepted contributions.
// LDS: count / sums are the workgroup's table, else the call's. `index`: the first slot's; `n`: the slots taken (4 for a quad).
template <bool LDS>
__device__ __forceinline__ void deposit_cells(const DepositArgs& a, const char* base, uint32_t* count, uint64_t* sums, const uint32_t* cell, uint32_t alive, uint32_t index, bool quad,
                                              LaneStats& st) {
#pragma unroll
    for (uint32_t t = 0; t < 4u; ++t) {
        if (((alive >> t) & 1u) == 0u) continue;
        if (LDS) lds_add_u32(count + cell[t], 1u); else add_u32(count + cell[t], 1u);
        st.deposited += 1u;
        st.outside += cell[t] == a.grid.n_cells ? 1u : 0u;
    }
    const uint32_t nch = a.n_channels;
#pragma unroll 1
    for (uint32_t k = 0; k < nch; ++k) {                                 // (one channel's scalars at a time)
        const uint32_t packed = a.ch[k].packed, nc = deposit_channel_ncomp(packed), comp = deposit_channel_comp(packed), frac = deposit_channel_frac_bits(packed);
        const uint32_t* plane = reinterpret_cast<const uint32_t*>(base + a.ch[k].plane_off);
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (quad && nc == 1u) {                                          // 16-byte aligned: index is a multiple of 4, the plane of 256
            const uint4 q = *reinterpret_cast<const uint4*>(plane + index);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (uint32_t t = 0; t < 4u; ++t)
                if ((alive >> t) & 1u) v[t] = plane[(uint64_t)(index + t) * nc + comp];     // (an alive bit is set for slots below the capacity alone)
        }
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) {
            if (((alive >> t) & 1u) == 0u) continue;
            const DepositQuant q = deposit_quantise(v[t], frac);
            if (q.ok) {
                uint64_t* dst = sums + ((size_t)cell[t] * nch + k);
                if (LDS) lds_add_u64(dst, (uint64_t)q.q); else add_u64(dst, (uint64_t)q.q);
            } else st.rejected += 1u;
        }
    }
}

// Slots [first, first + 4096) below the capacity of one instance, four quads per lane: quad q = round * 256 + tid, so that a wave's loads of one
// round are consecutive. The alive bytes of all four quads are requested before the first plane load. A quad that reaches past the capacity is
// taken slot by slot with 4-byte loads: nothing is read behind the last slot's components.
template <bool LDS>
__device__ __forceinline__ void deposit_tile(const DepositArgs& a, const char* base, uint32_t* count, uint64_t* sums, uint32_t first, uint32_t tid, LaneStats& st) {
    const char* flags = base + a.flag_off;
    const char* pos_plane = base + a.pos_off;
    const uint32_t cap = a.capacity;
    uint32_t f[4];
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t s0 = first + (r * kDepositBlock + tid) * 4u;      // (first + 4095 < 2^32: a tile starts below the capacity)
        // the four alive bytes of a quad that starts below the capacity lie inside the bytes' section: it is a multiple of 256 bytes long
        f[r] = s0 < cap ? *reinterpret_cast<const uint32_t*>(flags + s0) : 0u;
    }
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t s0 = first + (r * kDepositBlock + tid) * 4u;
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
        uint32_t cell[4];
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) cell[t] = bin_cell_of(a.grid, __uint_as_float(p[3u * t]), __uint_as_float(p[3u * t + 1u]), __uint_as_float(p[3u * t + 2u]));   // <= n_cells
        deposit_cells<LDS>(a, base, count, sums, cell, alive, s0, quad, st);
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// A wave's three numbers onto out_stats: one add per wave and non-zero number
__device__ __forceinline__ void add_stats(const DepositArgs& a, const LaneStats& st, uint32_t tid) {
    if (!a.stats) return;
    const uint32_t d = wave_sum(st.deposited), o = wave_sum(st.outside), r = wave_sum(st.rejected);
    if ((tid & 63u) == 0u) {
        if (d != 0u) add_u32(a.stats, d);
        if (o != 0u) add_u32(a.stats + 1, o);
        if (r != 0u) add_u32(a.stats + 2, r);
    }
}

__device__ __forceinline__ void lds_body(const DepositArgs& a, uint64_t* s_tab, uint32_t g, uint32_t k, uint32_t tid) {
    const uint32_t entries = a.grid.n_cells + 1u, n_sums = entries * a.n_channels;   // (the plan: entries * (4 + 8 n_channels) bytes are within kDepositLdsBudget)
    uint32_t* s_count = reinterpret_cast<uint32_t*>(s_tab + n_sums);
    for (uint32_t i = tid; i < n_sums; i += kDepositBlock) s_tab[i] = 0u;
    for (uint32_t i = tid; i < entries; i += kDepositBlock) s_count[i] = 0u;
    __syncthreads();
    LaneStats st = {0u, 0u, 0u};
    const char* base = reinterpret_cast<const char*>(a.slabs[k]);
    const uint32_t j0 = g * a.span, j1 = a.tiles - j0 < a.span ? a.tiles : j0 + a.span;    // (g < groups: j0 < tiles)
    for (uint32_t j = j0; j < j1; ++j) deposit_tile<true>(a, base, s_count, s_tab, j * kDepositTile, tid, st);
    __syncthreads();
    for (uint32_t i = tid; i < n_sums; i += kDepositBlock) {
        const uint64_t s = s_tab[i];
        if (s != 0u) add_u64(a.sums + i, s);
    }
    for (uint32_t i = tid; i < entries; i += kDepositBlock) {
        const uint32_t c = s_count[i];
        if (c != 0u) add_u32(a.count + i, c);
    }
    add_stats(a, st, tid);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_deposit_lds(const DepositArgs a) {
    extern __shared__ uint64_t s_tab[];                                   // the sums' rows, the counts behind them: DepositPlan::lds_bytes
    const uint32_t g = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    if (k >= a.n_inst || g >= a.groups) return;
    if (a.meta[k].alive_count == 0u) return;                              // nothing alive: no slot is read, nothing is added
    lds_body(a, s_tab, g, k, tid);
}

extern "C" __global__ void __launch_bounds__(256) k_deposit_global(const DepositArgs a) {
    const uint32_t j = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    if (k >= a.n_inst || j >= a.tiles) return;
    if (a.meta[k].alive_count == 0u) return;
    LaneStats st = {0u, 0u, 0u};
    deposit_tile<false>(a, reinterpret_cast<const char*>(a.slabs[k]), a.count, a.sums, j * kDepositTile, tid, st);
    add_stats(a, st, tid);
}
