/* hanabi_amd_pairs.h - the neighbour list of libhanabi_amd.so: one entry point next to the 61 of hanabi_amd.h, in a header of its own. It uses the
 * types, the error codes and the contract of hanabi_amd.h, the grid of hanabi_amd_binned.h and the pair rule of hanabi_amd_neighbours.h, and is
 * exported by the same library; a caller that needs sums only (hnb_effect_neighbours) does not need this header. */
#ifndef HANABI_AMD_PAIRS_H
#define HANABI_AMD_PAIRS_H

#include "hanabi_amd.h"
#include "hanabi_amd_binned.h"
#include "hanabi_amd_neighbours.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pairs: the fixed-radius neighbour list of one effect as CSR, on the device. hnb_effect_neighbours covers what is a weighted sum of v_j or
 * v_j - v_i; an SPH pressure force, a soft-sphere collision, a constraint solver or a line between every two particles closer than r need the
 * pairs themselves, in the consumer's own kernel. The call writes, for the alive particles inside a uniform grid in the binned export's order, the
 * slot of every row (out_rows), the offsets of its run (out_start) and the slots of its neighbours (out_pairs), optionally with their squared
 * distances (out_d2). One call, enqueued on the simulation stream behind the frames enqueued so far: no host synchronisation and no readback.
 * Everything below is exact to the bit and a function of the state alone.
 * Grid, inside and outside, coverage, neighbourhood, crowding guard
 *   hnb_effect_neighbours' rules, word for word (hanabi_amd_neighbours.h "Grid and cell", "Coverage", "Neighbourhood", "Crowding guard"), computed
 *   by the same functions. An alive particle is INSIDE iff its cell is not the OUTSIDE BIN; particles with a NaN or an infinite position land
 *   there; outside particles have no row and are in no run. radius is finite and > 0 with radius * inv_cell[c] <= 1 on every axis, evaluated in
 *   double on the host; r2 = radius * radius in f32. d2 is the header's eight statements, ending in d2 = s + zz.
 *   j is a NEIGHBOUR of i iff all three hold: (1) j and i are different slots - a coincident particle is a neighbour, the particle itself is
 *   not -, (2) their cell indices differ by at most 1 on every axis, and (3) d2 < r2. The relation is symmetric bit for bit.
 *   A query with candidates(i) > candidate_limit is CROWDED: it lists nothing - its run is empty - and is counted; it still appears in the runs
 *   of other queries. candidate_limit is 1 .. HNB_NEIGHBOUR_MAX_CANDIDATES; the guard bounds every loop of the call.
 * Rows
 *   n_inside = the number of inside particles. Row r, 0 <= r < n_inside, is the r-th record of hnb_effect_export_binned's order: ascending by
 *   cell, and within a cell in list order (the sort is stable). Ring lists are read through their head. out_rows[r] = the slot of row r;
 *   entries r with n_inside <= r < capacity are HNB_PAIRS_NO_ROW. capacity is the effect's slot count.
 * Runs
 *   The run of row r holds the slots of its neighbours in ascending sorted-row order. (The walk takes nine row ranges, index i = (dy + 1) +
 *   3 * (dz + 1); a range covers the up to three cells along x of one (y, z), and the cell index grows with y and then with z, so the ranges in
 *   index order are disjoint and already ascending in rows: the walk's order IS ascending row order.)
 *   With HNB_PAIRS_HALF only neighbours with slot_j > slot_i are listed: the pair {i, j} stands once, under the particle with the lower slot.
 *   A half list loses the pair whose lower slot is crowded - that query lists nothing, and the higher slot does not list downwards -, so a half
 *   list is complete iff stats[3] == 0. Without the flag, for two particles that are both not crowded, j is in i's run iff i is in j's.
 * Offsets and truncation
 *   T[r] = the 64-bit exclusive sum of the run lengths of the rows in front of r; T[n_inside] = the true total.
 *   out_start[r] = min(T[r], pair_capacity) for every r <= n_inside; every later entry up to index capacity repeats out_start[n_inside].
 *   Pair g of the list (global index, CSR order) is written iff g < pair_capacity: exactly a prefix of the list, so the table always describes
 *   exactly what is in out_pairs - run r is out_pairs[out_start[r] .. out_start[r + 1]), a truncated run is a prefix of the whole one.
 *   Entries of out_pairs / out_d2 at and past out_start[n_inside] keep every bit. out_d2[g], when given, is the d2 of pair g, bit for bit.
 *   pair_capacity == 0 is legal: the call counts only (out_pairs may then be NULL), every out_start entry is 0 and stats hold the true total.
 * Stats
 *   out_stats: [8] u32 on the device, 16-byte aligned, may be NULL; the call clears them first. [0] = the alive particles visited, [1] = n_inside,
 *   [2] = those in the outside bin, [3] = those crowded, [4], [5] = the low and the high word of the true total T[n_inside], [6] = the pairs
 *   written = min(T[n_inside], pair_capacity), [7] = 0.
 * State
 *   The call writes nothing of the effect: no plane, list, counter or cached proof. Later frames are bit-identical to those of a context that
 *   never made the call. Frozen instances accept it. It may be interleaved with every other call, with frames and with hnb_simulate_steps. It runs
 *   in stream order with no host synchronisation and no readback; only a call that allocates or grows its scratch may synchronise, once.
 * Errors: HNB_ERR_INVALID_ARG (with hnb_last_error text; nothing is enqueued) for a NULL argument, another struct_size, a flag bit other than
 *   HNB_PAIRS_HALF, a dims[c] of 0, a product above HNB_BIN_MAX_CELLS, an origin or inv_cell that is not finite, an inv_cell that is not > 0, a
 *   radius that is not finite and > 0, radius * inv_cell[c] > 1, r2 or its reciprocal not finite or r2 not normal, candidate_limit 0 or above
 *   HNB_NEIGHBOUR_MAX_CANDIDATES, a layout without POSITION, an effect of more than 0xFFFFFF00 slots, a NULL out_rows, a NULL out_start, a NULL
 *   out_pairs with pair_capacity > 0, a destination that is not 4-byte aligned, out_stats not 16-byte aligned, and any two destination ranges
 *   that overlap: out_rows [capacity], out_start [capacity + 1], out_pairs and out_d2 [pair_capacity] each, out_stats [8], in words, computed
 *   on the host from these sizes.
 * Scratch: owned by the library, per effect, and apart from every other call's: the sorted export's layout (hanabi_amd_binned.h "Scratch"), a
 *   snapshot of 16 bytes per slot (x, y, z, slot), 4 bytes per slot of run lengths, 8 bytes per tile of 256 rows, and a cell_start table of
 *   n_cells + 2 words. Allocated by the effect's first call and grown by a call that needs more; only such a call may synchronise the device,
 *   once. Freed with the effect.
 * Out of scope: a program form, pairs across effects, ELL (fixed-stride) output, row indices instead of slots, a per-query cap other than the
 *   crowding guard.
 * The kernels: the binned export's cell keys, stable sort and table and the neighbour sums' snapshot, unchanged, run into this call's scratch;
 *   then three of a code object of their own that the library carries and loads on first use (HNB_ERR_HIP if it cannot be loaded): the count
 *   of every row's run with a sum per tile, the scan of the tile sums by one workgroup, and the fill, which walks again and stores. */
#define HNB_PAIRS_HALF   0x1u          /* list the pair {i, j} once: under i iff slot_j > slot_i */
#define HNB_PAIRS_NO_ROW 0xFFFFFFFFu
typedef struct HnbPairsDesc {          /* 96 bytes */
    uint32_t struct_size;              /* sizeof(HnbPairsDesc) of the caller */
    uint32_t flags;                    /* 0 or HNB_PAIRS_HALF */
    uint32_t dims[3];                  /* the binned export's grid: cells along x, y, z, each >= 1, product n_cells <= HNB_BIN_MAX_CELLS */
    uint32_t candidate_limit;          /* 1..HNB_NEIGHBOUR_MAX_CANDIDATES: the crowding guard */
    float    origin[3];                /* the grid's lowest corner, finite */
    float    inv_cell[3];              /* 1 / cell edge per axis, finite and > 0 */
    float    radius;                   /* finite, > 0, radius * inv_cell[c] <= 1: hnb_effect_neighbours' coverage rule */
    uint32_t pair_capacity;            /* entries of out_pairs / out_d2; 0 is legal: count only */
    uint32_t* out_rows;                /* device [capacity]:     slot of sorted inside row r */
    uint32_t* out_start;               /* device [capacity + 1]: CSR offsets into out_pairs */
    uint32_t* out_pairs;               /* device [pair_capacity]: neighbour slots; may be NULL iff pair_capacity == 0 */
    float*    out_d2;                  /* device [pair_capacity] or NULL: d2 of every written pair */
    uint32_t* out_stats;               /* device [8], 16-byte aligned, or NULL */
} HnbPairsDesc;
int hnb_effect_pairs(HnbEffect* fx, const HnbPairsDesc* desc);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_AMD_PAIRS_H */
