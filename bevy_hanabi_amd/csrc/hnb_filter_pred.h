// The predicates of hnb_effect_export_filtered (include/hanabi_amd.h "Packed output", Filtered export): plain C++ that a host compiler and hipcc both
// take, so that the host-side tests state which rows pass with the functions the kernels call, and the runtime validates lo <= hi with the same key.
// Every f32 operation is a statement of its own, in the order the header writes it; nothing may be contracted into a fused multiply-add (the pragma
// for clang / hipcc; a host compiler builds this with -ffp-contract=off). A comparison with a NaN is false: the row does not pass.
#pragma once
#include <stdint.h>

#include "hnb_sort_key.h"

namespace hnb {

constexpr uint32_t kFilterMaxPlanes = 6;   // HNB_FILTER_MAX_PLANES

// keep p iff for every i < n_planes: ((p.x*P[i][0] + p.y*P[i][1]) + p.z*P[i][2]) + P[i][3] >= 0
HNB_SORT_KEY_FN bool filter_pass_planes(float x, float y, float z, const float (*P)[4], uint32_t n_planes) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    bool pass = true;
    for (uint32_t i = 0; i < kFilterMaxPlanes; ++i) {
        if (i >= n_planes) break;
        const float ax = x * P[i][0];
        const float by = y * P[i][1];
        const float xy = ax + by;
        const float cz = z * P[i][2];
        const float xyz = xy + cz;
        const float s = xyz + P[i][3];
        pass = pass && (s >= 0.0f);
    }
    return pass;
}

// e = p - S[0..2] per component; keep iff (e.x*e.x + e.y*e.y) + e.z*e.z <= S[3]
HNB_SORT_KEY_FN bool filter_pass_sphere(float x, float y, float z, const float* S) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float ex = x - S[0];
    const float ey = y - S[1];
    const float ez = z - S[2];
    const float xx = ex * ex;
    const float yy = ey * ey;
    const float xy = xx + yy;
    const float zz = ez * ez;
    const float d = xy + zz;
    return d <= S[3];
}

// keep iff key(lo) <= key(value) <= key(hi), key = sort_key_of(bits, is_f32, false): f32 in its total order (a NaN is a key like any other, outside the
// infinities by its sign), everything else as unsigned bits
HNB_SORT_KEY_FN bool filter_pass_range(uint32_t bits, bool is_f32, uint32_t lo_bits, uint32_t hi_bits) {
    const uint32_t k = sort_key_of(bits, is_f32, false);
    return sort_key_of(lo_bits, is_f32, false) <= k && k <= sort_key_of(hi_bits, is_f32, false);
}

}  // namespace hnb
