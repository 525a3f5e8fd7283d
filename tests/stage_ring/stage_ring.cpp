// Host build of plan::stage_ring_begin / _end / _drained (bevy_hanabi_amd/csrc/hnb_plan.h) behind a C interface: tests/test_stage_ring_plan.py
// drives the bookkeeping of the staging ring without a device and holds its invariant against a brute-force model of the stream.
// The product includes the same header; nothing here is product code.
#include "../../bevy_hanabi_amd/csrc/hnb_plan.h"

using namespace hnb::plan;

extern "C" {
void* srp_new() { return new StageRing(); }
void srp_free(void* h) { delete static_cast<StageRing*>(h); }
// out[0] = kStageSlots, out[1] = kStageGroup, out[2] = kStageGroups
void srp_consts(uint32_t* out) { out[0] = kStageSlots; out[1] = kStageGroup; out[2] = kStageGroups; }
// in front of the frame: *slot, and what to wait for (-1 nothing, -2 the stream, else the event's index)
int srp_begin(void* h, int stages, uint32_t* slot) {
    const StageStep st = stage_ring_begin(*static_cast<StageRing*>(h), stages != 0);
    *slot = st.slot;
    return st.wait;
}
void srp_drained(void* h) { stage_ring_drained(*static_cast<StageRing*>(h)); }
// behind the frame: the event to record (-1: none)
int srp_end(void* h, int stages, int written, int ok) { return stage_ring_end(*static_cast<StageRing*>(h), stages != 0, written != 0, ok != 0); }
uint32_t srp_staged(void* h) { return static_cast<StageRing*>(h)->staged; }
void srp_set_staged(void* h, uint32_t v) { static_cast<StageRing*>(h)->staged = v; }
}
