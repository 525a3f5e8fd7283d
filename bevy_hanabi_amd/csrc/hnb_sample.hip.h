// The sample's device code that both of its translation units need: hnb_sample.hip (hnb_effect_sample, one instance) and hnb_sample_prog.hip
// (hnb_program_sample, a workgroup per tile and instance). As hnb_export_filter.hip.h is to the filtered export's two units: everything is
// __device__ __forceinline__ in an anonymous namespace, and a unit's kernels are the only symbols its code object holds. The walk of a tile, the
// samples of a particle and the stores of a channel are parameterised by the slab base and the field pointer; everything else they need - the grid,
// the plane offsets, the capacity, the scale, the channels - they read from the unit's own argument block (SampleArgs or SampleProgArgs: the members
// are named alike).
//
// The walk is the deposit's (hnb_deposit.hip deposit_tile): a lane takes four quads of consecutive slots per tile, one 4-byte load of their alive
// bytes each, requested ahead, and, unless all four are zero, POSITION's 48 bytes. The mode and the channel count of a row are template parameters:
// a row of 4 channels is one 16-byte load, of 2 one 8-byte load. Per quad first the samples - one particle's corners live at a time - then the
// destinations, one channel's scalars at a time: a quad whose four slots are all written loads and stores a scalar or a 3-component plane as
// 16-byte vectors (components not named go back with the bits they came with), everything else goes per written dword. A lane stores only into the
// slots of its own quad, whose POSITION it has read before: POSITION may be a destination. Dead slots and particles in the outside bin are never
// stored to. Every loop is bounded by 4, 8 or 12. A corner row is below n_cells (hnb_sample.h sample_axis), so every field word read lies inside
// the n_cells * n_channels words behind `field`; a slot stored to is below the capacity.
#pragma once
#include <hip/hip_runtime.h>

#include "hnb_sample.h"

#pragma clang fp contract(off)   // (the rule is f32 arithmetic stated operation by operation: hnb_sample.h, hnb_bin_cell.h)

namespace {

using namespace hnb;

struct LaneStats { uint32_t visited, sampled, outside; };

__device__ __forceinline__ void add_u32(uint32_t* p, uint32_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Row `row` of the field: its NCH channels
template <uint32_t NCH>
__device__ __forceinline__ void load_row(const float* field, uint32_t row, float* c) {
    const float* src = field + (size_t)row * NCH;                        // (row < n_cells <= 2^24)
    if (NCH == 4u) {
        const float4 q = *reinterpret_cast<const float4*>(src);          // 16-byte aligned: the field is, a row is 16 bytes
        c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
    } else if (NCH == 2u) {
        const float2 q = *reinterpret_cast<const float2*>(src);
        c[0] = q.x; c[1] = q.y;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < NCH; ++k) c[k] = src[k];
    }
}

// s[k], k < NCH, of one inside particle at (x, y, z)
template <uint32_t MODE, uint32_t NCH, class Args>
__device__ __forceinline__ void sample_particle(const Args& a, const float* field, float x, float y, float z, uint32_t cell, float* s) {
    if (MODE == HNB_SAMPLE_NEAREST) {
        load_row<NCH>(field, cell, s);                                   // (inside: cell < n_cells)
        return;
    }
    const SampleAxis ax = sample_axis(sample_axis_t(x, a.grid.origin[0], a.grid.inv_cell[0]), a.grid.dims[0]);
    const SampleAxis ay = sample_axis(sample_axis_t(y, a.grid.origin[1], a.grid.inv_cell[1]), a.grid.dims[1]);
    const SampleAxis az = sample_axis(sample_axis_t(z, a.grid.origin[2], a.grid.inv_cell[2]), a.grid.dims[2]);
    uint32_t rows[8];
    sample_corner_rows(a.grid.dims, ax, ay, az, rows);
    float c[8][NCH];
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) load_row<NCH>(field, rows[i], c[i]);
#pragma unroll
    for (uint32_t k = 0; k < NCH; ++k) {
        float ck[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) ck[i] = c[i][k];
        s[k] = sample_blend(ck, ax.w, ay.w, az.w);
    }
}

// Channel K's destination for the slots of one quad that are written (wr: a bit per slot), s[t] their samples; index: the quad's first slot
__device__ __forceinline__ void store_channel(float scale, char* base, const SampleChannelArg& ch, const float* s, uint32_t wr, uint32_t index, bool quad) {
    const uint32_t nc = sample_channel_ncomp(ch.packed), comp = sample_channel_comp(ch.packed), op = sample_channel_op(ch.packed);
    uint32_t* plane = reinterpret_cast<uint32_t*>(base + ch.plane_off);
    const bool full = quad && wr == 0xFu;                                // 16-byte aligned below: index is a multiple of 4, the plane of 256
    if (full && nc == 1u) {
        uint4* dst = reinterpret_cast<uint4*>(plane + index);
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (op == HNB_SAMPLE_ADD) q = *dst;
        q.x = __float_as_uint(sample_store(op, __uint_as_float(q.x), s[0], scale));
        q.y = __float_as_uint(sample_store(op, __uint_as_float(q.y), s[1], scale));
        q.z = __float_as_uint(sample_store(op, __uint_as_float(q.z), s[2], scale));
        q.w = __float_as_uint(sample_store(op, __uint_as_float(q.w), s[3], scale));
        *dst = q;
    } else if (full && nc == 3u) {
        uint4* dst = reinterpret_cast<uint4*>(plane + (size_t)index * 3u);
        uint32_t w[12];
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            const uint4 q = dst[i];
            w[4u * i] = q.x; w[4u * i + 1u] = q.y; w[4u * i + 2u] = q.z; w[4u * i + 3u] = q.w;
        }
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) {
            const uint32_t old = comp == 0u ? w[3u * t] : comp == 1u ? w[3u * t + 1u] : w[3u * t + 2u];
            const uint32_t v = __float_as_uint(sample_store(op, __uint_as_float(old), s[t], scale));
#pragma unroll
            for (uint32_t c = 0; c < 3u; ++c) w[3u * t + c] = c == comp ? v : w[3u * t + c];     // (the other components: the bits they came with)
        }
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) dst[i] = make_uint4(w[4u * i], w[4u * i + 1u], w[4u * i + 2u], w[4u * i + 3u]);
    } else {
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) {
            if (((wr >> t) & 1u) == 0u) continue;                        // (a written bit is set for alive slots below the capacity alone)
            uint32_t* p = plane + ((size_t)(index + t) * nc + comp);
            const uint32_t old = op == HNB_SAMPLE_ADD ? *p : 0u;
            *p = __float_as_uint(sample_store(op, __uint_as_float(old), s[t], scale));
        }
    }
}

// Slots [first, first + 4096) below the capacity, four quads per lane: quad q = round * 256 + tid, so that a wave's loads of one round are
// consecutive. The alive bytes of all four quads are requested before the first plane load. A quad that reaches past the capacity is taken slot by
// slot with 4-byte loads and stores: nothing is read or written behind the last slot's components.
template <uint32_t MODE, uint32_t NCH, class Args>
__device__ __forceinline__ void sample_tile(const Args& a, char* base, const float* field, uint32_t first, uint32_t tid, LaneStats& st) {
    const char* flags = base + a.flag_off;
    const char* pos_plane = base + a.pos_off;
    const uint32_t cap = a.capacity;
    uint32_t f[4];
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t s0 = first + (r * kSampleBlock + tid) * 4u;       // (first + 4095 < 2^32: a tile starts below the capacity)
        // the four alive bytes of a quad that starts below the capacity lie inside the bytes' section: it is a multiple of 256 bytes long
        f[r] = s0 < cap ? *reinterpret_cast<const uint32_t*>(flags + s0) : 0u;
    }
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t s0 = first + (r * kSampleBlock + tid) * 4u;
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
        uint32_t wr = 0u;
        float s[NCH][4];                                                 // s[k][t]: channel k of slot s0 + t
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) {
            if (((alive >> t) & 1u) == 0u) continue;
            const float x = __uint_as_float(p[3u * t]), y = __uint_as_float(p[3u * t + 1u]), z = __uint_as_float(p[3u * t + 2u]);
            const uint32_t cell = bin_cell_of(a.grid, x, y, z);          // <= n_cells
            st.visited += 1u;
            if (cell == a.grid.n_cells) { st.outside += 1u; continue; }  // the outside bin: nothing of the particle is written
            st.sampled += 1u;
            wr |= 1u << t;
            float sk[NCH];
            sample_particle<MODE, NCH>(a, field, x, y, z, cell, sk);
#pragma unroll
            for (uint32_t k = 0; k < NCH; ++k) s[k][t] = sk[k];
        }
        if (wr == 0u) continue;
#pragma unroll
        for (uint32_t k = 0; k < NCH; ++k) store_channel(a.scale, base, a.ch[k], s[k], wr, s0, quad);
    }
}

// The tile by the channel count of a row (the same in every lane: a scalar branch)
template <uint32_t MODE, class Args>
__device__ __forceinline__ void sample_tile_by_channels(const Args& a, char* base, const float* field, uint32_t first, uint32_t tid, LaneStats& st) {
    switch (a.n_channels) {
        case 1u: sample_tile<MODE, 1u>(a, base, field, first, tid, st); break;
        case 2u: sample_tile<MODE, 2u>(a, base, field, first, tid, st); break;
        case 3u: sample_tile<MODE, 3u>(a, base, field, first, tid, st); break;
        case 4u: sample_tile<MODE, 4u>(a, base, field, first, tid, st); break;
        default: break;                                                  // (refused by sample_check_desc)
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

}  // namespace
