// The 32-bit sort keys of hnb_effect_export_sorted (include/hanabi_amd.h "Packed output", Sorted export): plain C++ that a host compiler and
// hipcc both take, so that the host-side tests state the order with the function the kernels call.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HNB_SORT_KEY_FN __host__ __device__ inline
#else
#define HNB_SORT_KEY_FN inline
#endif

namespace hnb {

// The bits of an f32 as a u32 whose unsigned order is the total order -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN: negative values have every
// bit flipped (a larger magnitude sorts first), the others the sign bit alone. No special case.
HNB_SORT_KEY_FN uint32_t sort_key_f32(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }

// A value of the key source -> the key that is sorted ascending: f32 through sort_key_f32, anything else as its bits; a descending sort
// complements the key, which keeps the sort stable (rows with equal keys stay in list order in both directions).
HNB_SORT_KEY_FN uint32_t sort_key_of(uint32_t bits, bool is_f32, bool descending) {
    const uint32_t k = is_f32 ? sort_key_f32(bits) : bits;
    return descending ? ~k : k;
}

}  // namespace hnb
