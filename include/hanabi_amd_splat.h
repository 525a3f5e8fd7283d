/* hanabi_amd_splat.h - the splat of libhanabi_amd.so: two entry points next to the 61 of hanabi_amd.h, in a header of their own. They use the
 * description, the destinations and the fixed-point sums of hanabi_amd_deposit.h and the cell-centred stencil of hanabi_amd_sample.h, and are
 * exported by the same library; a caller that does not need the trilinear transfer does not need this header. */
#ifndef HANABI_AMD_SPLAT_H
#define HANABI_AMD_SPLAT_H

#include "hanabi_amd_deposit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Splat: the deposit with the sample's stencil - the alive particles of an effect, or of every instance of a program, summed into a dense uniform
 * grid on the device, every inside particle spread over the eight cell centres around it with the weights hnb_effect_sample (TRILINEAR) reads them
 * with. The cloud-in-cell transfer of a fog volume, a wind or pressure solve or a learned force field: the adjoint of the trilinear sample, where
 * the deposit is the adjoint of the nearest one. The description is the deposit's, HnbDepositDesc, unchanged: count is [n_cells + 1], sums
 * [(n_cells + 1) * n_channels], a pair of tensors serves both calls, and the two calls may accumulate into one grid. One call, no order, no
 * records, no readback, and - the accumulation being integer - the same bits whatever the grouping of the particles into lanes, workgroups and
 * calls.
 * Grid, cell of a particle, inside / OUTSIDE BIN
 *   The deposit's, unchanged (hanabi_amd_deposit.h "Cell of a particle"): per axis c, t[c] = (p[c] - origin[c]) * inv_cell[c], every f32 operation
 *   rounded on its own; inside iff t[c] >= 0 and t[c] < (float)dims[c] on all three axes, the range tested BEFORE the conversion; otherwise
 *   cell = n_cells, the outside bin. Particles with a NaN or an infinite position land there.
 * Count
 *   The deposit's, exactly: count[c] = the number of alive particles whose OWN cell is c, modulo 2^32, for c = 0 .. n_cells. It is not weighted.
 * Channels
 *   The deposit's: component `comp` of an f32 attribute `attr` of the layout, frac_bits in 0..32; AGE is allowed and stale AGE is materialised
 *   first. In addition attr == HNB_SPLAT_ATTR_ONE, with comp == 0: a channel whose stored value is 1.0f for every particle, so that its sums are
 *   the weights themselves (mass). hnb_effect_deposit keeps refusing that attr.
 * Acceptance
 *   A (particle, channel) pair is tested once, on the stored value v, with the deposit's rule: it is REJECTED iff v is a NaN or an infinity or
 *   |v * 2^frac_bits| >= 2^62. A rejected pair adds nothing to any row and counts once in out_stats[2]; the particle's count and its other channels
 *   stay in.
 * Contribution of an outside particle
 *   What the deposit adds: q = v * 2^frac_bits rounded to the nearest integer, ties to even, into row n_cells.
 * Contribution of an inside particle
 *   The stencil is hnb_effect_sample's (hanabi_amd_sample.h, TRILINEAR). Every f32 operation is rounded on its own, in the order written, and
 *   nothing is contracted. Per axis c: u = t[c] - 0.5f; fl = floorf(u); w1[c] = u - fl; w0[c] = 1.0f - w1[c]; j = (int32_t)fl; lo[c] = max(j, 0);
 *   hi[c] = min(j + 1, dims[c] - 1). For each of the eight corners (a, b, c) in {0,1}^3, with index lo for 0 and hi for 1:
 *   W = (w_a[0] * w_b[1]) * w_c[2] (two rounded products, in that order); cv = v * W (one rounded product); q = cv * 2^frac_bits rounded to the
 *   nearest integer, ties to even, exactly as the deposit quantises a stored value; q is added to sums[row(a, b, c) * n_channels + k],
 *   row = (z * dims[1] + y) * dims[0] + x, a two's-complement sum modulo 2^64. Every w is in [0, 1], so |cv| <= |v|: an accepted v has eight
 *   accepted corners. Under clamping two or more corners name the same row, and all their q are added to it; a dims[c] of 1 puts both corners of
 *   that axis in cell 0. When w1 rounds to exactly 1.0 (a tiny negative u) the formula is followed as written: w0 = 0. Any |cv| < 2^-33 quantises
 *   to 0 at every allowed frac_bits, so whether the hardware keeps or flushes f32 denormals (|cv| < 2^-126) cannot show in the result. With
 *   HNB_SPLAT_ATTR_ONE at frac_bits 30 the eight q of a particle sum to 2^30 within 2^-22 of it (the weights' own rounding): sums.to(torch.float32) * 2.0**-frac_bits is the
 *   density.
 * Stats
 *   out_stats[0] = the alive particles visited (the outside bin's included), [1] = those in the outside bin, [2] = the rejected (particle,
 *   channel) pairs, [3] = 0. Modulo 2^32. out_stats may be NULL.
 * Accumulate
 *   The deposit's: without HNB_DEPOSIT_ACCUMULATE the call first clears count, sums and out_stats; with the flag it adds onto what is there,
 *   out_stats included - also onto what hnb_effect_deposit left.
 * Program form
 *   Every instance of the program goes into the one grid; the result is what the effect form gives over the instances with
 *   HNB_DEPOSIT_ACCUMULATE. A program with 0 instances is refused, and so are more than 65,535.
 * Everything else is the deposit's: the call is enqueued on the simulation stream behind the frames enqueued so far; no host synchronisation and no
 *   readback; the simulation is only read; no scratch at all and no allocation; every grid is sized from the capacity, the instance count and the
 *   description; no workgroup waits for another. The call may be interleaved with frames and every export, import, bounds, deposit and sample
 *   call.
 * Errors: HNB_ERR_INVALID_ARG (with hnb_last_error text; nothing is enqueued) for everything hnb_effect_deposit refuses but the attr
 *   HNB_SPLAT_ATTR_ONE, and for HNB_SPLAT_ATTR_ONE with comp != 0.
 * Out of scope: packed-u32 channels, per-particle weights from a second attribute, transforms, a filter in front, an f32 grid, higher-order
 *   (quadratic / cubic) kernels, boundary modes other than clamp, wave-level combining of equal rows, a sort-first path.
 * The kernels: two, in a code object of their own that the library carries and loads on first use (HNB_ERR_HIP if it cannot be loaded), chosen as
 *   the deposit chooses: a table of (n_cells + 1) * (4 + 8 * n_channels) bytes that fits a workgroup's LDS is accumulated there and flushed; a
 *   larger grid takes eight integer atomics per accepted contribution of an inside particle. Both give the same bits. */
#define HNB_SPLAT_ATTR_ONE 0xFFFFFFFFu   /* a channel whose value is 1.0f for every particle: the weights themselves (mass) */
int hnb_effect_splat(HnbEffect* fx, const HnbDepositDesc* desc);
int hnb_program_splat(HnbProgram* prog, const HnbDepositDesc* desc);   /* every instance into the one grid */

#ifdef __cplusplus
}
#endif
#endif /* HANABI_AMD_SPLAT_H */
