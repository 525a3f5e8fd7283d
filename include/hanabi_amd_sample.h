/* hanabi_amd_sample.h - the sample of libhanabi_amd.so: one entry point next to the 61 of hanabi_amd.h, in a header of its own. It uses the types, the
 * error codes and the contract of hanabi_amd.h and the grid of hanabi_amd_binned.h, and is exported by the same library; a caller that carries no
 * grid field back to the particles does not need this header. */
#ifndef HANABI_AMD_SAMPLE_H
#define HANABI_AMD_SAMPLE_H

#include "hanabi_amd.h"
#include "hanabi_amd_binned.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sample: the deposit's way back. For every alive particle of one effect whose POSITION lies inside a uniform grid, up to four channels of an f32
 * field resident on the device - the value of the particle's cell, or the trilinear blend of the eight cell centres around it - are scaled and stored
 * or added into one component of an f32 attribute each. What a torch convolution, a pressure or wind solve or a learned force field over a deposited
 * grid hands back to the particles. One call, enqueued on the simulation stream: no host synchronisation, no readback, no scratch, no allocation.
 * Grid and cell
 *   hnb_effect_export_binned's, unchanged (hanabi_amd_binned.h "Cell of a particle"): p = POSITION as stored, no transform. Every f32 operation
 *   is rounded on its own, in the order written: per axis c, t[c] = (p[c] - origin[c]) * inv_cell[c]; inside iff t[c] >= 0 and t[c] < (float)dims[c]
 *   (-0 is inside, a NaN or an infinity is not); i[c] = (uint32_t)t[c], the range tested BEFORE the conversion. A particle is SAMPLED iff it is
 *   inside on all three axes. Every other alive particle is in the OUTSIDE BIN: it keeps every bit of every plane and is counted. Particles with a
 *   NaN or an infinite position land there.
 *   The grid rules are the deposit's: dims[c] >= 1, product n_cells at most HNB_BIN_MAX_CELLS (taken in 64 bits), origin and inv_cell finite,
 *   inv_cell > 0.
 * Field
 *   field[((z * dims[1] + y) * dims[0] + x) * n_channels + k]: f32, channel-minor, n_cells rows, 16-byte aligned: the deposit's shape without the
 *   outside row, so a deposit-shaped tensor of n_cells + 1 rows may be passed - the last row is never read. The call only reads the field; it must
 *   stay valid until the stream has run the call. F_k(x, y, z) below is channel k of that row.
 * HNB_SAMPLE_NEAREST
 *   s_k = F_k(i[0], i[1], i[2]).
 * HNB_SAMPLE_TRILINEAR
 *   Cell-centred, clamped to the edge. Every f32 operation is rounded on its own, in this order, with no contraction:
 *   per axis c: u = t[c] - 0.5f; fl = floorf(u); w[c] = u - fl; j = (int32_t)fl (j is in -1 .. dims[c] - 1: the conversion is exact);
 *   corners: lo[c] = max(j, 0); hi[c] = min(j + 1, dims[c] - 1);
 *   along x, four times: a = F(lo0, y, z) + w[0] * (F(hi0, y, z) - F(lo0, y, z)) for (y, z) = (lo1, lo2), (hi1, lo2), (lo1, hi2), (hi1, hi2):
 *   a00, a10, a01, a11; along y: b0 = a00 + w[1] * (a10 - a00), b1 = a01 + w[1] * (a11 - a01); along z: s = b0 + w[2] * (b1 - b0).
 *   w may round to exactly 1.0 for a tiny negative u: both corners are then cell 0, and the formula is followed as written.
 * Store
 *   r = s * scale. HNB_SAMPLE_SET: v' = r. HNB_SAMPLE_ADD: v' = v + r, v the stored value. Each is one rounded f32 operation; denormals are kept.
 *   A NaN result is stored as a NaN; which NaN is unspecified. A non-finite field value propagates by these formulas: an infinite corner under
 *   clamping gives inf - inf, and that is the contract.
 * Destinations
 *   Channel k writes component `comp` of the f32 attribute `attr` of the layout: the attributes hnb_effect_bounds accepts, but AGE (a sampled age
 *   has no use hnb_effect_import does not serve, and the age cohorts stay out of the call). Packed u32 attributes such as COLOR are refused, and so
 *   are two channels that name one (attr, comp). POSITION is allowed: a particle's position is read before anything of it is stored.
 * Untouched state
 *   Slots of dead particles keep every bit of every plane; so do alive particles in the outside bin; attributes and components not named keep
 *   every bit. A wide store may cover a slot or a component it is not writing, but only with the bits it already holds. The lists, the alive
 *   bytes and the counters are never touched.
 * Stats
 *   out_stats[0] = the alive particles visited, [1] = those sampled, [2] = those in the outside bin, [3] = 0. Modulo 2^32; the call clears them
 *   first. out_stats may be NULL.
 * State after the call
 *   Later frames compute exactly what they would after hnb_effect_write_attr of planes holding the same values: the call makes the resets
 *   hnb_effect_write_attr and hnb_effect_import make. Frozen instances accept the call. It may be interleaved with every export, import, bounds
 *   and deposit call and with frames; hnb_simulate_steps is covered by the same resets.
 * Errors: HNB_ERR_INVALID_ARG (with hnb_last_error text; nothing is enqueued) for a NULL argument, another struct_size, flags != 0, an unknown
 *   mode, a dims[c] of 0, a product above HNB_BIN_MAX_CELLS, an origin or inv_cell that is not finite, an inv_cell that is not > 0, n_channels 0
 *   or above HNB_SAMPLE_MAX_CHANNELS, a channel whose attr is not an f32 attribute of the layout or is AGE, whose comp is at or past its component
 *   count, whose op is unknown, whose reserved is not 0 or whose (attr, comp) an earlier channel names, a channel entry at or past n_channels that
 *   is not all 0, a scale that is not finite, field NULL or not 16-byte aligned, out_stats not 16-byte aligned, a layout without POSITION.
 * Out of scope: a program form (the resets are per instance), AGE and packed-u32 destinations, f16 / bf16 fields, boundary modes other than
 *   clamp, a transform of the positions or a rotation of vectors, a filter in front, interpolation in time between two fields, per-channel scales.
 * The kernels: two, one per mode, in a code object of their own that the library carries and loads on first use (HNB_ERR_HIP if it cannot be
 *   loaded): the deposit's slot-major walk with eight gathers and a read-modify-write of a plane at the end. */
#define HNB_SAMPLE_MAX_CHANNELS 4
#define HNB_SAMPLE_NEAREST      0u
#define HNB_SAMPLE_TRILINEAR    1u
#define HNB_SAMPLE_SET          0u
#define HNB_SAMPLE_ADD          1u
typedef struct HnbSampleChannel {
    uint32_t attr;        /* an f32 attribute of the layout, not AGE */
    uint32_t comp;        /* its component, below the attribute's component count */
    uint32_t op;          /* HNB_SAMPLE_SET or HNB_SAMPLE_ADD */
    uint32_t reserved;    /* 0 */
} HnbSampleChannel;       /* 16 bytes */
typedef struct HnbSampleDesc {             /* 136 bytes */
    uint32_t struct_size;                  /* sizeof(HnbSampleDesc) of the caller */
    uint32_t flags;                        /* 0 */
    uint32_t dims[3];                      /* the binned export's grid: cells along x, y, z, each >= 1, product n_cells <= HNB_BIN_MAX_CELLS */
    uint32_t n_channels;                   /* 1..HNB_SAMPLE_MAX_CHANNELS: the channels of a field row */
    float    origin[3];                    /* the grid's lowest corner, finite */
    float    inv_cell[3];                  /* 1 / cell edge per axis, finite and > 0 */
    uint32_t mode;                         /* HNB_SAMPLE_NEAREST or HNB_SAMPLE_TRILINEAR */
    float    scale;                        /* finite: r = s * scale */
    HnbSampleChannel channels[HNB_SAMPLE_MAX_CHANNELS];   /* channel k of the field goes to channels[k]; entries at and past n_channels all 0 */
    const float* field;   /* device, 16-byte aligned: [n_cells * n_channels], channel-minor; only read */
    uint32_t* out_stats;  /* device, 16-byte aligned: [4]; may be NULL */
} HnbSampleDesc;
int hnb_effect_sample(HnbEffect* fx, const HnbSampleDesc* desc);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_AMD_SAMPLE_H */
