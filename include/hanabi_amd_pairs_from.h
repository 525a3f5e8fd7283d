/* hanabi_amd_pairs_from.h - the neighbour list across two effects of libhanabi_amd.so: one entry point next to the 61 of hanabi_amd.h, in a header
 * of its own. It uses the types, the error codes and the contract of hanabi_amd.h, the grid of hanabi_amd_binned.h, the pair rule of
 * hanabi_amd_neighbours.h and the description of hanabi_amd_pairs.h, and is exported by the same library; a caller whose effects do not look at each
 * other does not need this header. */
#ifndef HANABI_AMD_PAIRS_FROM_H
#define HANABI_AMD_PAIRS_FROM_H

#include "hanabi_amd.h"
#include "hanabi_amd_binned.h"
#include "hanabi_amd_neighbours.h"
#include "hanabi_amd_pairs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs across effects: the fixed-radius neighbour list between two effects as CSR, on the device. hanabi_amd_pairs.h lists "pairs across effects"
 * and hanabi_amd_neighbours_from.h "a pair list across effects" as out of scope; this call lifts that item. hnb_effect_neighbours_from covers what
 * is a weighted sum of v_j or v_j - v_i over another effect; sparks that collide with debris, boids that steer at the NEAREST predator, an arc drawn
 * from every rocket to the trail particles around it or any pair force between species that is no such sum need the pairs themselves, in the
 * consumer's own kernel. QUERIES are the alive particles of `fx`, SOURCES the alive particles of `source`. The call writes, for the queries inside
 * a uniform grid in the binned export's order of fx, the slot of every row (out_rows), the offsets of its run (out_start) and the slots of its
 * neighbours IN SOURCE (out_pairs), optionally with their squared distances (out_d2). The description is HnbPairsDesc unchanged. One call, enqueued
 * on the simulation stream behind the frames enqueued so far: no host synchronisation and no readback. The rule is hnb_effect_pairs' rule word for
 * word (hanabi_amd_pairs.h) except where this text says otherwise; everything below is exact to the bit and a function of the two states alone.
 * Grid, inside and outside, coverage, d2
 *   Unchanged (hanabi_amd_neighbours.h "Grid and cell", "Coverage", "Neighbourhood"), computed by the same functions. One grid serves both sides.
 *   A query is INSIDE iff its cell in the grid is not the OUTSIDE BIN; the same holds for a source. A NaN or an infinite position lands in the
 *   outside bin on either side. Outside queries have no row; outside sources are in no run. radius is finite and > 0 with radius * inv_cell[c] <= 1
 *   on every axis, evaluated in double on the host; r2 = radius * radius in f32. d2 is the header's eight statements, ending in d2 = s + zz, with the
 *   query as i and the source as j.
 * Neighbourhood
 *   hnb_effect_neighbours_from's rule: source j is a NEIGHBOUR of query i iff (1) their cell indices differ by at most 1 on every axis and (2)
 *   d2 < r2. There is no self-exclusion: the two particles belong to different effects, so equal slot numbers mean nothing, and a coincident source
 *   is a neighbour.
 * Crowding guard
 *   candidates(i) = the inside SOURCES in the at most 27 cells around i's cell; the query is not among them. A query with candidates(i) >
 *   candidate_limit is CROWDED: it lists nothing - its run is empty - and is counted. candidate_limit is 1 .. HNB_NEIGHBOUR_MAX_CANDIDATES; the
 *   guard bounds every loop of the call.
 * Rows
 *   n_inside = the number of inside QUERIES. Row r, 0 <= r < n_inside, is the r-th record of hnb_effect_export_binned of FX in this grid: ascending
 *   by cell, and within a cell in list order (the sort is stable). Ring lists are read through their head, on both sides. out_rows[r] = fx's slot
 *   of row r; entries r with n_inside <= r < capacity are HNB_PAIRS_NO_ROW. capacity is FX's slot count: it sizes out_rows [capacity] and
 *   out_start [capacity + 1]. The source's slot count sizes nothing of the caller's.
 * Runs
 *   The run of row r holds SOURCE slots, in ascending sorted-row order of the source - the order of hnb_effect_export_binned of source in this
 *   grid. (The walk takes nine row ranges of the source, index i = (dy + 1) + 3 * (dz + 1); a range covers the up to three cells along x of one
 *   (y, z), and the cell index grows with y and then with z, so the ranges in index order are disjoint and already ascending in rows: the walk's
 *   order IS ascending row order.)
 *   The list of fx from source and the list of source from fx are transposes of each other where neither side is crowded: d2 is symmetric bit for
 *   bit.
 * Flags
 *   flags must be 0. HNB_PAIRS_HALF is refused, with a text of its own: it lists a pair under the lower slot, and a slot order across two effects
 *   means nothing.
 * Offsets and truncation
 *   hnb_effect_pairs' rule exactly. T[r] = the 64-bit exclusive sum of the run lengths of the rows in front of r; T[n_inside] = the true total.
 *   out_start[r] = min(T[r], pair_capacity) for every r <= n_inside; every later entry up to index capacity repeats out_start[n_inside].
 *   Pair g of the list (global index, CSR order) is written iff g < pair_capacity: exactly a prefix of the list, so the table always describes
 *   exactly what is in out_pairs - run r is out_pairs[out_start[r] .. out_start[r + 1]), a truncated run is a prefix of the whole one.
 *   Entries of out_pairs / out_d2 at and past out_start[n_inside] keep every bit. out_d2[g], when given, is the d2 of pair g, bit for bit.
 *   pair_capacity == 0 is legal: the call counts only (out_pairs may then be NULL), every out_start entry is 0 and stats hold the true total.
 * Stats
 *   out_stats: [8] u32 on the device, 16-byte aligned, may be NULL; the call clears them first. [0] = the alive queries visited, [1] = n_inside,
 *   [2] = queries in the outside bin, [3] = crowded queries, [4], [5] = the low and the high word of the true total T[n_inside], [6] = the pairs
 *   written = min(T[n_inside], pair_capacity), [7] = the inside sources.
 * State
 *   The call writes nothing of either effect: no plane, list, counter or cached proof. Later frames of both are bit-identical to those of a context
 *   that never made the call. Frozen instances are accepted on both sides. It may be interleaved with every other call, with frames and with
 *   hnb_simulate_steps. It runs in stream order with no host synchronisation and no readback; only a call that allocates or grows its scratch may
 *   synchronise, once.
 * Allowed
 *   fx and source may be instances of one program or of different programs. They must belong to the same context: the call is ordered on that
 *   context's stream.
 * Errors: HNB_ERR_INVALID_ARG (with hnb_last_error text; nothing is enqueued), in this order: a NULL argument; fx == source (the list within one
 *   effect is hnb_effect_pairs'); effects of different contexts; another struct_size, HNB_PAIRS_HALF, any other flag bit, a dims[c] of 0, a product
 *   above HNB_BIN_MAX_CELLS, an origin or inv_cell that is not finite, an inv_cell that is not > 0, a radius that is not finite and > 0,
 *   radius * inv_cell[c] > 1, r2 or its reciprocal not finite or r2 not normal, candidate_limit 0 or above HNB_NEIGHBOUR_MAX_CANDIDATES; fx's
 *   layout without a POSITION of 3 f32 components, source's layout without one, fx above 0xFFFFFF00 slots, source above 0xFFFFFF00 slots; a NULL
 *   out_rows, a NULL out_start, a NULL out_pairs with pair_capacity > 0, a destination that is not 4-byte aligned, out_stats not 16-byte aligned,
 *   and any two destination ranges that overlap: out_rows [capacity], out_start [capacity + 1], out_pairs and out_d2 [pair_capacity] each,
 *   out_stats [8], in words, capacity being fx's, computed on the host from these sizes.
 * Scratch: owned by the library, by fx, apart from every other call's and freed with fx: a sort layout (hanabi_amd_binned.h "Scratch") for
 *   source's capacity and one for fx's, a snapshot of 16 bytes per source slot (x, y, z, slot), 4 bytes per slot of fx of run lengths, 8 bytes per
 *   tile of 256 query rows, and one cell_start table of n_cells + 2 words, for the sources. Grown by a call that needs more; only such a call may
 *   synchronise the device, once.
 * Out of scope: a program form, more than one source effect per call, different grids for the two sides, a transform between the effects' spaces,
 *   ELL (fixed-stride) output, a HALF form.
 * The kernels: for source the binned export's cell keys, stable sort and table and the neighbour sums' snapshot, unchanged, run into this call's
 *   scratch; for fx the same sort alone, so that the lanes of a wave hold queries of the same cells; then the count of every query's run with a
 *   sum per tile and the fill, which walks again and stores - two kernels of a code object of their own that the library carries and loads on first
 *   use (HNB_ERR_HIP if it cannot be loaded) -, with hnb_effect_pairs' scan of the tile sums by one workgroup, unchanged, between them. */
int hnb_effect_pairs_from(HnbEffect* fx, HnbEffect* source, const HnbPairsDesc* desc);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_AMD_PAIRS_FROM_H */
