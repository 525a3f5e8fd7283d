/* hanabi_amd_sample_program.h - the program form of the sample of libhanabi_amd.so: one entry point next to the 61 of hanabi_amd.h and the one of
 * hanabi_amd_sample.h, in a header of its own. hanabi_amd_sample.h lists a program form as out of its scope; this is where it lives. It uses that
 * header's description, rule and contract, and is exported by the same library; a caller that samples one instance at a time does not need it. */
#ifndef HANABI_AMD_SAMPLE_PROGRAM_H
#define HANABI_AMD_SAMPLE_PROGRAM_H

#include "hanabi_amd_sample.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sample, program form: a grid field into every instance of a program in one call - what a consumer that deposits or splats a whole program into
 * one grid (hnb_program_deposit, hnb_program_splat) and solves a wind or pressure field over it hands back to all instances, without walking them
 * on the host.
 * Contract
 *   For every instance i of the program, in instance order, the planes afterwards hold bit for bit what
 *   hnb_effect_sample(instance_i, &desc->sample) would have left, with `field` replaced by instance i's field. The rule, the grid and the cell of
 *   a particle, the OUTSIDE BIN, both modes, the store, the destinations and the untouched state are hanabi_amd_sample.h's, unchanged.
 * Field of an instance
 *   field_instance_stride == 0: every instance reads desc->sample.field. Otherwise instance i reads sample.field + i * field_instance_stride
 *   (f32 elements, the product taken in 64 bits): the stride is a multiple of 4 - so every instance's field is 16-byte aligned - and at least
 *   n_cells * n_channels; a stride of (n_cells + 1) * n_channels rounded up to 4 takes deposit-shaped tensors, whose outside rows are never read.
 *   The call only reads the fields; they must stay valid until the stream has run the call.
 * Stats
 *   sample.out_stats[0..3] = hanabi_amd_sample.h's four numbers summed over all instances, modulo 2^32. out_instance_stats[i][0..3] = the four
 *   numbers of instance i, what hnb_effect_sample's out_stats would hold for it. The call clears both first. Either or both may be NULL.
 * State after the call
 *   hanabi_amd_sample.h's, for every instance - those with nothing alive and the frozen ones included: later frames and hnb_simulate_steps compute
 *   exactly what they would after hnb_effect_write_attr of planes holding the same values. The resets behind it are made on the device, by a
 *   kernel over all instances.
 * The call is enqueued on the simulation stream behind the frames enqueued so far: no host synchronisation, no readback, no allocation, no
 *   scratch. The number of enqueues - at most four - does not depend on the instance count. It may be interleaved with everything
 *   hnb_effect_sample may be interleaved with.
 * Errors: HNB_ERR_INVALID_ARG (with hnb_last_error text; nothing is enqueued) for a NULL argument, another outer struct_size, outer flags != 0,
 *   reserved != 0, everything hnb_effect_sample refuses in `sample`, a field_instance_stride that is not 0 and not a multiple of 4 or below
 *   n_cells * n_channels, out_instance_stats not 16-byte aligned, a program of 0 or more than HNB_PROGRAM_SAMPLE_MAX_INSTANCES instances.
 * Out of scope: per-instance grids or transforms, AGE destinations, a change of the effect form's stats path, several small instances packed
 *   into one workgroup (an instance of 256 slots still takes a workgroup of its own), and everything hanabi_amd_sample.h leaves out.
 * The kernels: three, in a code object of their own that the library carries and loads on first use (HNB_ERR_HIP if it cannot be loaded): one per
 *   mode, a workgroup per tile and instance, and the one that makes the resets. */
#define HNB_PROGRAM_SAMPLE_MAX_INSTANCES 65535u
typedef struct HnbProgramSampleDesc {      /* 168 bytes */
    uint32_t struct_size;                  /* sizeof(HnbProgramSampleDesc) of the caller */
    uint32_t flags;                        /* 0 */
    HnbSampleDesc sample;                  /* hnb_effect_sample's description, with its own struct_size and flags 0: grid, mode, scale, channels;
                                              field = instance 0's field; out_stats = the totals over all instances, or NULL */
    uint64_t field_instance_stride;        /* in f32 elements. 0: every instance reads the one field. Otherwise instance i reads
                                              field + i * stride; a multiple of 4, at least n_cells * n_channels */
    uint32_t* out_instance_stats;          /* device, 16-byte aligned: [n_instances][4], row i = what hnb_effect_sample's out_stats would hold
                                              for instance i; may be NULL */
    uint64_t reserved;                     /* 0 */
} HnbProgramSampleDesc;
int hnb_program_sample(HnbProgram* prog, const HnbProgramSampleDesc* desc);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_AMD_SAMPLE_PROGRAM_H */
