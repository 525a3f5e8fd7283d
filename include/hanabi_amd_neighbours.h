/* hanabi_amd_neighbours.h - the neighbour sums of libhanabi_amd.so: one entry point next to the 61 of hanabi_amd.h, in a header of its own. It uses
 * the types, the error codes and the contract of hanabi_amd.h, the grid of hanabi_amd_binned.h and HNB_SPLAT_ATTR_ONE of hanabi_amd_splat.h, and is
 * exported by the same library; a caller whose particles do not look at each other does not need this header. */
#ifndef HANABI_AMD_NEIGHBOURS_H
#define HANABI_AMD_NEIGHBOURS_H

#include "hanabi_amd.h"
#include "hanabi_amd_binned.h"
#include "hanabi_amd_splat.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Neighbours: particle <-> particle. For every alive particle of one effect inside a uniform grid, up to four weighted sums over the particles within
 * `radius` of it - a count, an SPH-style density, boids cohesion or alignment, XSPH smoothing - are taken in fixed point and stored or added into
 * one component of an f32 attribute each, where the effect's own update program reads them. The library runs the 27-cell walk over the cell list of
 * hnb_effect_export_binned itself. One call, enqueued on the simulation stream behind the frames enqueued so far: no host synchronisation and no
 * readback on the steady path. Everything below is exact to the bit.
 * Grid and cell
 *   hnb_effect_export_binned's, unchanged (hanabi_amd_binned.h "Cell of a particle"): dims, origin, inv_cell and the same validity rules. An alive
 *   particle is INSIDE iff its cell is not the outside bin. Particles in the OUTSIDE BIN are neither queries nor sources: they keep every bit of
 *   every plane and are counted. Particles with a NaN or an infinite position land there.
 * Coverage
 *   radius is finite and > 0, and radius * inv_cell[c] <= 1 on every axis, evaluated in double on the host: a ball of that radius around a point
 *   of a cell reaches no further than the 26 cells around it. The call is refused otherwise.
 * Neighbourhood
 *   Every f32 operation is rounded on its own, in the order written, with no contraction. r2 = radius * radius and inv_r2 = 1.0f / r2 are computed
 *   by the library on the host in f32; the call is refused unless both are finite and r2 is a normal number. For a query i and a source j, both
 *   inside: dx = xj - xi, dy = yj - yi, dz = zj - zi; xx = dx * dx, yy = dy * dy, zz = dz * dz; s = xx + yy; d2 = s + zz.
 *   j is a NEIGHBOUR of i iff (1) j and i are different slots - a coincident particle is a neighbour, the particle itself is not -, (2) their
 *   cell indices differ by at most 1 on every axis, and (3) d2 < r2. The cell restriction (2) is part of the contract: under the coverage rule it
 *   differs from the plain ball only for pairs within rounding of the radius across two cell borders, and it makes the 27-cell walk the
 *   definition, not an approximation. The relation is symmetric bit for bit.
 * Crowding guard
 *   candidates(i) = the inside particles in the at most 27 cells around i's cell, i itself included; cells beyond the grid's edge do not exist.
 *   A query with candidates(i) > candidate_limit is CROWDED: it is not gathered, keeps every bit and is counted; it remains a source for others.
 *   candidate_limit is 1 .. HNB_NEIGHBOUR_MAX_CANDIDATES. The guard bounds every loop of the call by the limit - a degenerate state, everything
 *   in one cell, cannot turn a call into minutes - and it is deterministic: a function of the state alone.
 * Weight
 *   q = d2 * inv_r2; u = 1.0f - q. HNB_NEIGHBOUR_W_ONE: W = 1 (q and u are not formed); _W_U1: W = u; _W_U2: W = u * u; _W_U3: W = (u * u) * u.
 *   u may round to 0 or to a tiny negative number: the formula is followed as written.
 * Channels
 *   n_channels is 1 .. HNB_NEIGHBOUR_MAX_CHANNELS. Channel k has a SOURCE (src_attr, src_comp): an f32 attribute of the layout as
 *   hnb_effect_deposit accepts them, or HNB_SPLAT_ATTR_ONE with comp 0, whose stored value is 1.0f; the flag HNB_NEIGHBOUR_DIFF; frac_bits in
 *   0..32; and a DESTINATION (dst_attr, dst_comp, op) under exactly hnb_effect_sample's rules: an f32 attribute, not AGE, not packed u32, no two
 *   channels with one destination, op HNB_SAMPLE_SET or HNB_SAMPLE_ADD.
 *   The contribution of neighbour j to channel k: v = v_j, the stored value (1.0f for HNB_SPLAT_ATTR_ONE); with HNB_NEIGHBOUR_DIFF v = v_j - v_i,
 *   one rounded operation (DIFF with HNB_SPLAT_ATTR_ONE is refused). cv = v * W, one rounded product; under HNB_NEIGHBOUR_W_ONE cv = v.
 *   q_int = the deposit's quantisation of cv in units of 2^-frac_bits (hanabi_amd_deposit.h: nearest, ties to even; a NaN, an infinity or a
 *   magnitude at or above 2^62 units is REJECTED). A rejected contribution is counted and leaves the other channels in. S_k = the
 *   two's-complement sum of the accepted q_int over the neighbours of i, modulo 2^64: it does not depend on the order or grouping of the sum.
 * Store
 *   r = (float)S_k (int64 to binary32, to nearest, ties to even); r = r * 2^-frac_bits; r = r * scale (scale is finite). HNB_SAMPLE_SET: v' = r.
 *   HNB_SAMPLE_ADD: v' = v + r, v the stored value. A gathered particle with no neighbours has S_k = 0, and the formula is followed.
 * No hazards by construction
 *   Positions and sources are taken from a snapshot the call makes before anything is stored. A destination may therefore be POSITION or the
 *   source of any channel: the result is that of reading the whole state first.
 * Untouched state
 *   As in hnb_effect_sample: slots of dead particles, particles in the outside bin, crowded particles and attributes and components not named
 *   keep every bit. The lists, the alive bytes and the counters are never touched. Ring lists are read through their head. Stale AGE is
 *   materialised first when AGE is a source.
 * Stats
 *   out_stats: [8] u32 on the device, 16-byte aligned, may be NULL; the call clears them first; modulo 2^32. [0] = the alive particles visited,
 *   [1] = those gathered, [2] = those in the outside bin, [3] = those crowded, [4] = rejected contributions, [5..7] = 0.
 * State after the call
 *   Later frames compute exactly what they would after hnb_effect_write_attr of planes holding the same values: the call makes the resets
 *   hnb_effect_sample makes. Frozen instances accept the call. It may be interleaved with every export, import, bounds, deposit, splat and
 *   sample call, with frames and with hnb_simulate_steps.
 * Errors: HNB_ERR_INVALID_ARG (with hnb_last_error text; nothing is enqueued) for a NULL argument, another struct_size, flags != 0, a dims[c] of
 *   0, a product above HNB_BIN_MAX_CELLS, an origin or inv_cell that is not finite, an inv_cell that is not > 0, a radius that is not finite and
 *   > 0, radius * inv_cell[c] > 1, r2 or inv_r2 not finite or r2 not normal, an unknown weight, candidate_limit 0 or above
 *   HNB_NEIGHBOUR_MAX_CANDIDATES, n_channels 0 or above HNB_NEIGHBOUR_MAX_CHANNELS, a channel whose source is not HNB_SPLAT_ATTR_ONE or an f32
 *   attribute of the layout, whose src_comp is at or past the component count (not 0 for HNB_SPLAT_ATTR_ONE), whose flags hold another bit than
 *   HNB_NEIGHBOUR_DIFF or DIFF with HNB_SPLAT_ATTR_ONE, whose frac_bits is above 32, whose destination hnb_effect_sample would refuse, whose
 *   reserved is not 0, a channel entry at or past n_channels that is not all 0, a scale that is not finite, out_stats not 16-byte aligned, a
 *   layout without POSITION, an effect of more than 0xFFFFFF00 slots.
 * Scratch: owned by the library, per effect, and apart from every other call's: the sorted export's layout (hanabi_amd_binned.h "Scratch"), a
 *   snapshot of 16 bytes per slot (x, y, z, slot) plus 4 bytes per slot and source channel, and a cell_start table of n_cells + 2 words.
 *   Allocated by the effect's first call and grown by a call that needs more; only such a call may synchronise the device, once. Freed with the
 *   effect.
 * Out of scope: a program form, pairs across effects, a transform of the positions, other weight kernels, per-channel scales, u32
 *   destinations, a neighbour list as output.
 * The kernels: the binned export's cell keys, stable sort and table, unchanged, run into this call's scratch; then two of a code object of their
 *   own that the library carries and loads on first use (HNB_ERR_HIP if it cannot be loaded): the snapshot in cell order, and the gather, one lane
 *   per inside particle walking at most nine contiguous row ranges of the snapshot. */
#define HNB_NEIGHBOUR_MAX_CHANNELS   4
#define HNB_NEIGHBOUR_MAX_CANDIDATES 65536u
#define HNB_NEIGHBOUR_W_ONE 0u
#define HNB_NEIGHBOUR_W_U1  1u
#define HNB_NEIGHBOUR_W_U2  2u
#define HNB_NEIGHBOUR_W_U3  3u
#define HNB_NEIGHBOUR_DIFF  0x1u     /* HnbNeighbourChannel::flags: v = v_j - v_i */
typedef struct HnbNeighbourChannel {
    uint32_t src_attr;    /* an f32 attribute of the layout, or HNB_SPLAT_ATTR_ONE */
    uint32_t src_comp;    /* its component; 0 for HNB_SPLAT_ATTR_ONE */
    uint32_t flags;       /* 0 or HNB_NEIGHBOUR_DIFF */
    uint32_t frac_bits;   /* 0..32: the sum is taken in units of 2^-frac_bits */
    uint32_t dst_attr;    /* an f32 attribute of the layout, not AGE */
    uint32_t dst_comp;    /* its component */
    uint32_t op;          /* HNB_SAMPLE_SET or HNB_SAMPLE_ADD */
    uint32_t reserved;    /* 0 */
} HnbNeighbourChannel;    /* 32 bytes */
typedef struct HnbNeighbourDesc {          /* 200 bytes */
    uint32_t struct_size;                  /* sizeof(HnbNeighbourDesc) of the caller */
    uint32_t flags;                        /* 0 */
    uint32_t dims[3];                      /* the binned export's grid: cells along x, y, z, each >= 1, product n_cells <= HNB_BIN_MAX_CELLS */
    uint32_t n_channels;                   /* 1..HNB_NEIGHBOUR_MAX_CHANNELS */
    float    origin[3];                    /* the grid's lowest corner, finite */
    float    inv_cell[3];                  /* 1 / cell edge per axis, finite and > 0 */
    float    radius;                       /* finite, > 0, radius * inv_cell[c] <= 1 */
    float    scale;                        /* finite: the last factor of the store */
    uint32_t weight;                       /* HNB_NEIGHBOUR_W_* */
    uint32_t candidate_limit;              /* 1..HNB_NEIGHBOUR_MAX_CANDIDATES: queries with more candidates are crowded */
    HnbNeighbourChannel channels[HNB_NEIGHBOUR_MAX_CHANNELS];   /* entries at and past n_channels all 0 */
    uint32_t* out_stats;  /* device, 16-byte aligned: [8]; may be NULL */
} HnbNeighbourDesc;
int hnb_effect_neighbours(HnbEffect* fx, const HnbNeighbourDesc* desc);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_AMD_NEIGHBOURS_H */
