/* hanabi_amd_neighbours_from.h - the neighbour sums across two effects of libhanabi_amd.so: one entry point next to the 61 of hanabi_amd.h, in a
 * header of its own. It uses the types, the error codes and the contract of hanabi_amd.h and the description, the pair rule and the store of
 * hanabi_amd_neighbours.h, and is exported by the same library; a caller whose effects do not look at each other does not need this header. */
#ifndef HANABI_AMD_NEIGHBOURS_FROM_H
#define HANABI_AMD_NEIGHBOURS_FROM_H

#include "hanabi_amd.h"
#include "hanabi_amd_neighbours.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Neighbours across effects: species <-> species. hnb_effect_neighbours and hnb_effect_pairs stop at the border of one effect and list pairs across
 * effects as out of scope; this call lifts that item for the sums. For every alive particle of `fx` inside a uniform grid, up to four weighted sums
 * over the particles of ANOTHER effect, `source`, within `radius` of it - sparks pushed out of a smoke volume, boids that avoid predators, trails
 * that thin out where rockets pass, a density of effect B felt by effect A - are taken in fixed point and stored or added into one component of an
 * f32 attribute of fx each. QUERIES are the alive particles of fx, SOURCES the alive particles of source, DESTINATIONS planes of fx. One call,
 * enqueued on the simulation stream behind the frames enqueued so far: no host synchronisation and no readback on the steady path. The description is
 * HnbNeighbourDesc unchanged. The rule is hnb_effect_neighbours' rule word for word (hanabi_amd_neighbours.h) except where this text says otherwise,
 * and everything is exact to the bit.
 * Grid, coverage, r2 / inv_r2, d2, weight, quantisation, S_k modulo 2^64, store
 *   Unchanged (hanabi_amd_neighbours.h "Grid and cell", "Coverage", "Neighbourhood", "Weight", "Channels", "Store"), and computed by the same
 *   functions. One grid serves both sides.
 * Cells
 *   A query is INSIDE iff its cell in the grid is not the OUTSIDE BIN; the same holds for a source. A NaN or infinite position lands in the outside
 *   bin on either side. Outside queries keep every bit of every plane and are counted. Outside sources contribute to nobody.
 * Neighbourhood
 *   Source j is a NEIGHBOUR of query i iff (1) their cell indices differ by at most 1 on every axis and (2) d2 < r2, d2 the header's eight
 *   statements ending in d2 = s + zz. There is no self-exclusion: the two particles belong to different effects, so equal slot numbers mean
 *   nothing, and a coincident source is a neighbour.
 * Crowding guard
 *   candidates(i) = the inside SOURCES in the at most 27 cells around i's cell; the query is not among them. A query with candidates(i) >
 *   candidate_limit is CROWDED: it is not gathered, keeps every bit and is counted. Every loop of the call is bounded by 9, by candidate_limit or
 *   by a capacity.
 * Channels
 *   src_attr / src_comp are looked up in SOURCE's layout, or are HNB_SPLAT_ATTR_ONE. dst_attr / dst_comp / op are looked up in FX's layout, under
 *   hnb_effect_sample's rules. With HNB_NEIGHBOUR_DIFF v = v_j - v_i, v_i the query's own stored src_attr[src_comp]: the attribute must then also
 *   be an f32 attribute of fx's layout with src_comp below its component count; otherwise the call is refused.
 * No hazards by construction
 *   A lane reads its own particle's position and its own v_i before it stores, no lane reads another query's planes, and source is only ever
 *   read. A destination may therefore be fx's POSITION or a DIFF operand: the result is that of reading both states first.
 * AGE
 *   Stale AGE is materialised first on source when a channel reads AGE, and on fx too when that channel is DIFF.
 * Stats
 *   out_stats: [8] u32 on the device, 16-byte aligned, may be NULL; the call clears them first; modulo 2^32. [0] = the alive queries visited,
 *   [1] = queries gathered, [2] = queries in the outside bin, [3] = crowded queries, [4] = rejected contributions, [5] = inside sources, [6] = the
 *   alive sources visited, [7] = 0.
 * State after the call
 *   On fx: later frames compute exactly what they would after hnb_effect_write_attr of planes holding the same values - the resets
 *   hnb_effect_neighbours makes. Dead slots, outside and crowded queries and attributes and components not named keep every bit; lists, alive
 *   bytes and counters are never touched. On source: source is untouched - no plane, list, counter or cached proof changes (AGE materialised as
 *   above is what hnb_effect_materialise leaves), and its later frames are bit-identical to those of a context that never made the call. Frozen
 *   instances are accepted on both sides. The call may be interleaved with every other call, with frames and with hnb_simulate_steps.
 * Allowed
 *   fx and source may be instances of one program or of different programs. They must belong to the same context: the call is ordered on that
 *   context's stream.
 * Errors: HNB_ERR_INVALID_ARG (with hnb_last_error text; nothing is enqueued) for a NULL argument; fx == source (the sums within one effect are
 *   hnb_effect_neighbours'); effects of different contexts; then hnb_effect_neighbours' refusals in their order, a channel's source checked against
 *   source's layout and its destination against fx's - another struct_size, flags != 0, a dims[c] of 0, a product above HNB_BIN_MAX_CELLS, an
 *   origin or inv_cell that is not finite, an inv_cell that is not > 0, a radius that is not finite and > 0, radius * inv_cell[c] > 1, r2 or inv_r2
 *   not finite or r2 not normal, an unknown weight, candidate_limit 0 or above HNB_NEIGHBOUR_MAX_CANDIDATES, n_channels 0 or above
 *   HNB_NEIGHBOUR_MAX_CHANNELS, a channel whose source is not HNB_SPLAT_ATTR_ONE or an f32 attribute of source's layout, whose src_comp is at or
 *   past the component count (not 0 for HNB_SPLAT_ATTR_ONE), whose flags hold another bit than HNB_NEIGHBOUR_DIFF or DIFF with
 *   HNB_SPLAT_ATTR_ONE, a DIFF attribute missing from fx's layout (or not f32 there, or with fewer components), a frac_bits above 32, a
 *   destination hnb_effect_sample would refuse on fx, a reserved that is not 0, a channel entry at or past n_channels that is not all 0, a scale
 *   that is not finite, out_stats not 16-byte aligned - and then fx's layout without a POSITION of 3 f32 components, source's layout without one,
 *   fx above 0xFFFFFF00 slots, source above 0xFFFFFF00 slots.
 * Scratch: owned by the library, by fx, apart from every other call's and freed with fx: a sort layout (hanabi_amd_binned.h "Scratch") for fx's
 *   capacity and one for source's, a snapshot of 16 bytes per source slot (x, y, z, slot) plus 4 bytes per source slot and channel, and one
 *   cell_start table of n_cells + 2 words, for the sources. Grown by a call that needs more; only such a call may synchronise the device, once.
 * Out of scope: a program form, a pair list across effects, more than one source effect per call, different grids for the two sides, a transform
 *   between the effects' spaces, effects of different contexts.
 * The kernels: for source the binned export's cell keys, stable sort and table and the neighbour sums' snapshot, unchanged, run into this call's
 *   scratch; for fx the same sort alone, so that the lanes of a wave hold queries of the same cells; then one kernel of a code object of its own
 *   that the library carries and loads on first use (HNB_ERR_HIP if it cannot be loaded): the gather, one lane per sorted query walking at most
 *   nine contiguous row ranges of source's snapshot. */
int hnb_effect_neighbours_from(HnbEffect* fx, HnbEffect* source, const HnbNeighbourDesc* desc);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_AMD_NEIGHBOURS_FROM_H */
