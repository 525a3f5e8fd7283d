// Particle bounds (hnb_effect_bounds, hnb_program_bounds, include/hanabi_amd.h "Bounds"; DESIGN.md "Bounds"): per component of one f32 attribute the
// smallest and the largest stored value among the alive particles of an instance, in the order of the sorted export's key, with the alive and the NaN
// particles counted. A code object of its own, like the exports': nothing here is part of the fat binary of libhanabi_amd.so. A min / max fold does
// not depend on the order, so nothing reads the alive list: the walk is over the SLOTS, the alive byte of a slot says whether it takes part.
//   k_bounds_tile    workgroup (j, k): slots [4096 j, 4096 j + 4096) of instance k -> one 64-byte BoundsPartial in the scratch. A lane takes four quads
//                    of consecutive slots: one 4-byte load of their alive bytes and, unless all four are zero, the plane's ncomp * 16 bytes as 16-byte
//                    loads. Folded in key space with integer min / max; lanes through the wave's shuffles, the four waves through 192 bytes of LDS.
//   k_bounds_finish  ONE workgroup per instance: its tiles' partials -> its HnbBounds record.
//   k_bounds_union   ONE workgroup: the instances' records -> the record behind them (program form).
//   k_bounds_small   instances of at most 4096 slots: tile and record by ONE workgroup per instance, no scratch.
// The simulation is only read. Every loop is bounded by the capacity, the tile count or the instance count; every grid is sized from them; every
// partial and record is written by every call (an instance with nothing alive leaves after the scalar loads with the empty one): nothing is zeroed in
// front, there is no atomic, and no workgroup waits for another.
#include <hip/hip_runtime.h>

#include "hnb_bounds.h"

#pragma clang fp contract(off)   // (nothing here rounds: integer min / max of keys; the unit is built with -ffp-contract=off like the exports')

using namespace hnb;

namespace {

// What a lane has seen: the members of a BoundsPartial for the NC components of the attribute, in registers
template <uint32_t NC>
struct LaneBounds {
    uint32_t lo[NC], hi[NC], alive, nan;
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (uint32_t c = 0; c < NC; ++c) { lo[c] = kBoundsEmptyLoKey; hi[c] = kBoundsEmptyHiKey; }
        alive = nan = 0u;
    }
    // one slot (bounds_fold_slot, the liveness and the NaNs as masks)
    __device__ __forceinline__ void slot(const uint32_t* bits, bool is_alive) {
        bool any_nan = false;
#pragma unroll
        for (uint32_t c = 0; c < NC; ++c) {
            const bool is_nan = bounds_is_nan(bits[c]), use = is_alive && !is_nan;
            const uint32_t k = sort_key_f32(bits[c]);
            lo[c] = bounds_min(lo[c], use ? k : kBoundsEmptyLoKey);
            hi[c] = bounds_max(hi[c], use ? k : kBoundsEmptyHiKey);
            any_nan = any_nan || is_nan;
        }
        alive += is_alive ? 1u : 0u;
        nan += is_alive && any_nan ? 1u : 0u;
    }
};

// Slots [first, first + 4096) below `capacity` of one instance, four quads per lane: quad q = round * 256 + tid, so that a wave's loads of one
// round are consecutive. The alive bytes of all four quads are requested before the first plane load. A quad that reaches past the capacity is
// taken slot by slot with 4-byte loads: nothing is read behind the last slot's components.
template <uint32_t NC>
__device__ __forceinline__ void fold_tile(LaneBounds<NC>& b, const char* base, const BoundsArgs& a, uint32_t first, uint32_t tid) {
    const char* flags = base + a.flag_off;
    const char* plane = base + a.plane_off;
    const uint32_t cap = a.capacity;
    uint32_t f[4];
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t s0 = first + (r * kBoundsBlock + tid) * 4u;       // (first + 4095 < 2^32: a tile starts below the capacity)
        // the four alive bytes of a quad that starts below the capacity lie inside the bytes' section: it is a multiple of 256 bytes long
        f[r] = s0 < cap ? *reinterpret_cast<const uint32_t*>(flags + s0) : 0u;
    }
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t s0 = first + (r * kBoundsBlock + tid) * 4u;
        if (f[r] == 0u) continue;                                        // four free slots (or none below the capacity): the plane is not read
        if (cap - s0 >= 4u) {
            uint32_t v[4u * NC];
            const uint4* src = reinterpret_cast<const uint4*>(plane + (uint64_t)s0 * (NC * 4u));   // 16-byte aligned: s0 is a multiple of 4, the plane of 256
#pragma unroll
            for (uint32_t i = 0; i < NC; ++i) {
                const uint4 q = src[i];
                v[4u * i] = q.x; v[4u * i + 1u] = q.y; v[4u * i + 2u] = q.z; v[4u * i + 3u] = q.w;
            }
#pragma unroll
            for (uint32_t t = 0; t < 4u; ++t) b.slot(v + t * NC, ((f[r] >> (8u * t)) & 0xffu) != 0u);
        } else {
            for (uint32_t t = 0; t < cap - s0; ++t) {                    // the capacity's last 1..3 slots
                uint32_t v[NC];
                const uint32_t* src = reinterpret_cast<const uint32_t*>(plane + (uint64_t)(s0 + t) * (NC * 4u));
#pragma unroll
                for (uint32_t c = 0; c < NC; ++c) v[c] = src[c];
                b.slot(v, ((f[r] >> (8u * t)) & 0xffu) != 0u);
            }
        }
    }
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = bounds_min(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = bounds_max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// The workgroup's lanes into one: lane tid < 10 returns word tid of the folded partial (lo[0..3], hi[0..3], alive, nan; components at and past NC
// empty), the lanes behind them 0. s_part: [4 waves][12] words.
template <uint32_t NC>
__device__ __forceinline__ uint32_t block_fold(const LaneBounds<NC>& b, uint32_t* s_part, uint32_t tid) {
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    uint32_t w[10];
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c) {
        w[c] = kBoundsEmptyLoKey; w[4u + c] = kBoundsEmptyHiKey;
    }
#pragma unroll
    for (uint32_t c = 0; c < NC; ++c) { w[c] = wave_min(b.lo[c]); w[4u + c] = wave_max(b.hi[c]); }
    w[8] = wave_sum(b.alive);
    w[9] = wave_sum(b.nan);
    if (lane == 0u) {
#pragma unroll
        for (uint32_t i = 0; i < 10u; ++i) s_part[wave * 12u + i] = w[i];
    }
    __syncthreads();
    uint32_t r = 0u;
    if (tid < 10u) {
        const uint32_t x0 = s_part[tid], x1 = s_part[12u + tid], x2 = s_part[24u + tid], x3 = s_part[36u + tid];
        r = tid < 4u ? bounds_min(bounds_min(x0, x1), bounds_min(x2, x3)) : tid < 8u ? bounds_max(bounds_max(x0, x1), bounds_max(x2, x3)) : x0 + x1 + x2 + x3;
    }
    return r;
}

// Word tid of the empty partial
__device__ __forceinline__ uint32_t empty_word(uint32_t tid) { return tid < 4u ? kBoundsEmptyLoKey : tid < 8u ? kBoundsEmptyHiKey : 0u; }

template <uint32_t NC>
__device__ __forceinline__ void tile_body(const BoundsArgs& a, uint32_t j, uint32_t k, uint32_t* s_part, uint32_t tid) {
    LaneBounds<NC> b;
    b.clear();
    fold_tile<NC>(b, reinterpret_cast<const char*>(a.slabs[k]), a, j * kBoundsTile, tid);
    const uint32_t r = block_fold<NC>(b, s_part, tid);
    uint32_t* out = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.partials) + (uint64_t)k * a.pitch_bytes + (uint64_t)j * sizeof(BoundsPartial));
    if (tid < 16u) out[tid] = r;                                          // (words 10..15: the padding, 0)
}

template <uint32_t NC>
__device__ __forceinline__ void small_body(const BoundsArgs& a, uint32_t k, uint32_t* s_part, uint32_t tid) {
    LaneBounds<NC> b;
    b.clear();
    fold_tile<NC>(b, reinterpret_cast<const char*>(a.slabs[k]), a, 0u, tid);
    const uint32_t r = block_fold<NC>(b, s_part, tid);
    if (tid < 12u) a.dst[(size_t)k * 12u + tid] = bounds_record_word(tid, r, NC);
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_bounds_tile(const BoundsArgs a) {
    __shared__ uint32_t s_part[48];
    const uint32_t j = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    if (k >= a.n_inst || j >= a.tiles) return;
    if (a.meta[k].alive_count == 0u) {                                    // nothing alive: the empty partial, no slot is read
        uint32_t* out = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(a.partials) + (uint64_t)k * a.pitch_bytes + (uint64_t)j * sizeof(BoundsPartial));
        if (tid < 16u) out[tid] = empty_word(tid);
        return;
    }
    switch (a.ncomp) {
        case 1u: tile_body<1u>(a, j, k, s_part, tid); break;
        case 2u: tile_body<2u>(a, j, k, s_part, tid); break;
        case 3u: tile_body<3u>(a, j, k, s_part, tid); break;
        default: tile_body<4u>(a, j, k, s_part, tid); break;
    }
}

extern "C" __global__ void __launch_bounds__(256) k_bounds_finish(const BoundsArgs a) {
    __shared__ uint32_t s_part[48];
    const uint32_t k = blockIdx.y, tid = threadIdx.x;
    if (k >= a.n_inst) return;
    const uint4* part = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(a.partials) + (uint64_t)k * a.pitch_bytes);
    LaneBounds<4u> b;
    b.clear();
    for (uint32_t j = tid; j < a.tiles; j += kBoundsBlock) {              // (every tile's partial was written by this call's k_bounds_tile)
        const uint4 lo = part[(size_t)j * 4u], hi = part[(size_t)j * 4u + 1u], n = part[(size_t)j * 4u + 2u];
        b.lo[0] = bounds_min(b.lo[0], lo.x); b.lo[1] = bounds_min(b.lo[1], lo.y); b.lo[2] = bounds_min(b.lo[2], lo.z); b.lo[3] = bounds_min(b.lo[3], lo.w);
        b.hi[0] = bounds_max(b.hi[0], hi.x); b.hi[1] = bounds_max(b.hi[1], hi.y); b.hi[2] = bounds_max(b.hi[2], hi.z); b.hi[3] = bounds_max(b.hi[3], hi.w);
        b.alive += n.x;
        b.nan += n.y;
    }
    const uint32_t r = block_fold<4u>(b, s_part, tid);
    if (tid < 12u) a.dst[(size_t)k * 12u + tid] = bounds_record_word(tid, r, a.ncomp);
}

extern "C" __global__ void __launch_bounds__(256) k_bounds_union(const BoundsArgs a) {
    __shared__ uint32_t s_part[48];
    const uint32_t tid = threadIdx.x;
    LaneBounds<4u> b;
    b.clear();
    for (uint32_t k = tid; k < a.n_inst; k += kBoundsBlock) {             // (bounds_fold_record; the records are this call's)
        const uint4* rec = reinterpret_cast<const uint4*>(a.dst + (size_t)k * 12u);
        const uint4 lo = rec[0], hi = rec[1], n = rec[2];
        const uint32_t l[4] = {lo.x, lo.y, lo.z, lo.w}, h[4] = {hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c) {
            const bool has = c < a.ncomp;
            b.lo[c] = bounds_min(b.lo[c], has ? sort_key_f32(l[c]) : kBoundsEmptyLoKey);
            b.hi[c] = bounds_max(b.hi[c], has ? sort_key_f32(h[c]) : kBoundsEmptyHiKey);
        }
        b.alive += n.x;
        b.nan += n.y;
    }
    const uint32_t r = block_fold<4u>(b, s_part, tid);
    if (tid < 12u) a.dst[(size_t)a.n_inst * 12u + tid] = bounds_record_word(tid, r, a.ncomp);
}

extern "C" __global__ void __launch_bounds__(256) k_bounds_small(const BoundsArgs a) {
    __shared__ uint32_t s_part[48];
    const uint32_t k = blockIdx.y, tid = threadIdx.x;
    if (k >= a.n_inst) return;
    if (a.meta[k].alive_count == 0u) {                                    // nothing alive: the empty record, no slot is read
        if (tid < 12u) a.dst[(size_t)k * 12u + tid] = bounds_record_word(tid, empty_word(tid), a.ncomp);
        return;
    }
    switch (a.ncomp) {
        case 1u: small_body<1u>(a, k, s_part, tid); break;
        case 2u: small_body<2u>(a, k, s_part, tid); break;
        case 3u: small_body<3u>(a, k, s_part, tid); break;
        default: small_body<4u>(a, k, s_part, tid); break;
    }
}
