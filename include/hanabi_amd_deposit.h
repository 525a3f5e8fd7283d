/* hanabi_amd_deposit.h - the deposit of libhanabi_amd.so: two entry points next to the 61 of hanabi_amd.h, in a header of their own. They use the
 * types, the error codes and the contract of hanabi_amd.h and the grid of hanabi_amd_binned.h, and are exported by the same library; a caller that
 * does not need a dense grid does not need this header. */
#ifndef HANABI_AMD_DEPOSIT_H
#define HANABI_AMD_DEPOSIT_H

#include "hanabi_amd.h"
#include "hanabi_amd_binned.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Deposit: the alive particles of an effect - or of every instance of a program - summed into a dense uniform grid on the device: per cell how many
 * particles lie in it and, for up to four channels, the sum of one component of an f32 attribute in fixed point. What a fog volume, a density-driven
 * level of detail or a 3-D convolution starts from: count is [D, H, W] (+ 1), sums [D, H, W, k] (+ 1 row). One call, no order, no records, no
 * readback, and - the accumulation being integer - the same bits whatever the grouping of the particles into lanes, workgroups and calls.
 * Cell of a particle
 *   hnb_effect_export_binned's, unchanged (hanabi_amd_binned.h "Cell of a particle"): p = POSITION as stored, no transform. Every f32 operation
 *   is rounded on its own, in the order written: per axis c, t = (p[c] - origin[c]) * inv_cell[c]; inside iff t >= 0 and t < (float)dims[c] (-0 is
 *   inside, a NaN or an infinity is not); i[c] = (uint32_t)t, the range tested BEFORE the conversion. Inside on all three axes:
 *   cell = (i[2] * dims[1] + i[1]) * dims[0] + i[0]; otherwise cell = n_cells = dims[0] * dims[1] * dims[2], the OUTSIDE BIN: entry n_cells of
 *   count and row n_cells of sums. Particles with a NaN or an infinite position land there.
 *   The grid rules are the binned export's: dims[c] >= 1, product at most HNB_BIN_MAX_CELLS (taken in 64 bits), origin and inv_cell finite,
 *   inv_cell > 0.
 * Count
 *   count[c] = the number of alive particles whose cell is c, modulo 2^32, for c = 0 .. n_cells.
 * Channels
 *   Channel k reads component `comp` of the f32 attribute `attr` of the layout: the attributes hnb_effect_bounds accepts (HDR_COLOR among them;
 *   packed u32 attributes such as COLOR are refused).
 * Contribution
 *   Of a stored value v to channel k: q = v * 2^frac_bits rounded to the nearest integer, ties to even, frac_bits in 0..32. It is REJECTED when v is
 *   a NaN or an infinity or when |v * 2^frac_bits| >= 2^62. sums[c * n_channels + k] = the sum of the accepted q over the alive particles of cell
 *   c, a two's-complement sum modulo 2^64. A rejected contribution leaves the particle's count and its other channels in.
 *   q is a function of the 32 stored bits in integer arithmetic alone (sign, exponent, 24-bit significand, a shift with round-half-even): no
 *   rounding mode and no contraction can enter. In numpy, exactly: d = float64(v) * 2.0**frac_bits; ok = isfinite(d) & (abs(d) < 2**62);
 *   q = rint(d).astype(int64). As f32 again: sums.to(torch.float32) * 2.0**-frac_bits.
 * Stats
 *   out_stats[0] = the particles deposited (the alive particles, the outside bin's included), [1] = those in the outside bin, [2] = the rejected
 *   contributions, [3] = 0. Modulo 2^32. out_stats may be NULL.
 * Accumulate
 *   Without HNB_DEPOSIT_ACCUMULATE the call first clears count, sums and out_stats: every entry is defined by every call, and an effect with
 *   nothing alive leaves zeros. With the flag the call adds onto what is there, out_stats included: how several effects, or several programs,
 *   fill one fog volume (the first call of a frame without the flag, the others with it).
 * Program form
 *   Every instance of the program goes into the one grid, each with its positions as stored; out_stats are the totals. The result is what the effect
 *   form gives over the instances with HNB_DEPOSIT_ACCUMULATE. A program with 0 instances is refused, as hnb_program_bounds refuses it, and so are
 *   more than 65,535.
 * Everything else is hnb_effect_bounds': the call is enqueued on the simulation stream behind the frames enqueued so far; no host synchronisation
 *   and no readback; the simulation is only read; stale AGE is materialised first when a channel reads AGE; no scratch at all; every grid is sized
 *   from the capacity, the instance count and the description, all known to the host; no workgroup waits for another. The call may be interleaved
 *   with every export, import, bounds call and frame.
 * Errors: HNB_ERR_INVALID_ARG (with hnb_last_error text; nothing is enqueued) for a NULL argument, another struct_size, a flag that is not
 *   defined, a dims[c] of 0, a product above HNB_BIN_MAX_CELLS, an origin or inv_cell that is not finite, an inv_cell that is not > 0,
 *   n_channels > HNB_DEPOSIT_MAX_CHANNELS, a channel whose attr is not an f32 attribute of the layout, whose comp is at or past its component count,
 *   whose frac_bits is above 32 or whose reserved is not 0, a channel entry at or past n_channels that is not all 0, count NULL or not 16-byte
 *   aligned, sums NULL with channels, not NULL without, or not 16-byte aligned, out_stats not 16-byte aligned, a layout without POSITION.
 * Out of scope: packed-u32 channels, weights or products of attributes, transforms of the positions, a filter in front, an f32 output grid,
 *   multi-cell (trilinear) splats.
 * The kernels: two, in a code object of their own that the library carries and loads on first use (HNB_ERR_HIP if it cannot be loaded). A grid
 *   whose table of (n_cells + 1) * (4 + 8 * n_channels) bytes fits a workgroup's LDS is accumulated there over a span of slots and flushed with
 *   integer atomics at consecutive addresses; a larger grid takes one integer atomic per particle and per accepted contribution. Both give the
 *   same bits. */
#define HNB_DEPOSIT_MAX_CHANNELS 4
#define HNB_DEPOSIT_ACCUMULATE   0x1u
typedef struct HnbDepositChannel {
    uint32_t attr;        /* an f32 attribute of the layout */
    uint32_t comp;        /* its component, below the attribute's component count */
    uint32_t frac_bits;   /* 0..32: the sums are in units of 2^-frac_bits */
    uint32_t reserved;    /* 0 */
} HnbDepositChannel;      /* 16 bytes */
typedef struct HnbDepositDesc {            /* 136 bytes */
    uint32_t struct_size;                  /* sizeof(HnbDepositDesc) of the caller */
    uint32_t flags;                        /* 0 or HNB_DEPOSIT_ACCUMULATE */
    uint32_t dims[3];                      /* the binned export's grid: cells along x, y, z, each >= 1, product n_cells <= HNB_BIN_MAX_CELLS */
    uint32_t n_channels;                   /* 0..HNB_DEPOSIT_MAX_CHANNELS */
    float    origin[3];                    /* the grid's lowest corner, finite */
    float    inv_cell[3];                  /* 1 / cell edge per axis, finite and > 0 */
    HnbDepositChannel channels[HNB_DEPOSIT_MAX_CHANNELS];   /* entries at and past n_channels all 0 */
    uint32_t* count;      /* device, 16-byte aligned: [n_cells + 1] */
    int64_t*  sums;       /* device, 16-byte aligned: [(n_cells + 1) * n_channels], channel-minor; NULL iff n_channels == 0 */
    uint32_t* out_stats;  /* device, 16-byte aligned: [4]; may be NULL */
} HnbDepositDesc;
int hnb_effect_deposit(HnbEffect* fx, const HnbDepositDesc* desc);
int hnb_program_deposit(HnbProgram* prog, const HnbDepositDesc* desc);   /* every instance into the one grid */

#ifdef __cplusplus
}
#endif
#endif /* HANABI_AMD_DEPOSIT_H */
