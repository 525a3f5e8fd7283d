// Host build of plan::prove_fused_span (bevy_hanabi_amd/csrc/hnb_plan.h) behind a C interface: tests/test_fused_span_plan.py drives every premise of
// "the next S frames of this program may run as one launch" without a device, and replays prove_skip_lists step by step beside it.
// The product includes the same header; nothing here is product code.
#include "../../bevy_hanabi_amd/csrc/hnb_plan.h"

#include <vector>

using namespace hnb::plan;

extern "C" {
struct Row { uint32_t simulated, has_parent, spawn_count, event_capacity; uint32_t ublock[8]; };   // operand k reads ublock[k]
struct State { SkipFacts facts; SkipHistory hist; };

void* fsp_new(int eligible, uint32_t dt_operand) { State* s = new State(); s->facts.eligible = eligible != 0; s->facts.dt_operand = dt_operand; return s; }
void* fsp_clone(void* h) { return new State(*static_cast<State*>(h)); }
void fsp_free(void* h) { delete static_cast<State*>(h); }
void fsp_mark_dirty(void* h) { static_cast<State*>(h)->hist.dirty = true; }
// 1: both histories are the same, bit for bit (cum_tick ring, last_dirty, dirty)
int fsp_same_history(void* a, void* b) {
    const SkipHistory &x = static_cast<State*>(a)->hist, &y = static_cast<State*>(b)->hist;
    return std::memcmp(x.cum_tick, y.cum_tick, sizeof x.cum_tick) == 0 && x.last_dirty == y.last_dirty && x.dirty == y.dirty;
}
static std::vector<InstanceFrame> frames_of(const Row* rows, uint32_t count) {
    std::vector<InstanceFrame> v(count);
    for (uint32_t i = 0; i < count; ++i) {
        v[i].simulated = rows[i].simulated != 0; v[i].has_parent = rows[i].has_parent != 0;
        v[i].spawn_count = rows[i].spawn_count; v[i].event_capacity = rows[i].event_capacity; v[i].ublock = rows[i].ublock;
    }
    return v;
}
// one single frame: prove_skip_lists
int fsp_single(void* h, uint32_t frame_no, const Row* rows, uint32_t n, uint32_t tag, uint32_t bound_bits, int option) {
    State* s = static_cast<State*>(h);
    const std::vector<InstanceFrame> v = frames_of(rows, n);
    return prove_skip_lists(s->facts, s->hist, frame_no, v.data(), n, SkipPublished{tag, bound_bits}, option != 0) ? 1 : 0;
}
// rows: [n_steps][n], step-major
uint32_t fsp_span(void* h, uint32_t frame_no, const Row* rows, uint32_t n, uint32_t n_steps, uint32_t n_uregs, uint32_t tag, uint32_t bound_bits,
                  int opt_skip_lists, int opt_fuse, int program_eligible, uint32_t max_steps, uint32_t block_words) {
    State* s = static_cast<State*>(h);
    const std::vector<InstanceFrame> v = frames_of(rows, n * n_steps);
    FuseLimits lim;
    lim.max_steps = max_steps; lim.block_words = block_words;
    return prove_fused_span(s->facts, s->hist, frame_no, v.data(), n, n_steps, n_uregs, SkipPublished{tag, bound_bits}, opt_skip_lists != 0, opt_fuse != 0,
                            program_eligible != 0, lim);
}
uint32_t fsp_cap(uint32_t n, uint32_t n_uregs, uint32_t max_steps, uint32_t block_words) {
    FuseLimits lim;
    lim.max_steps = max_steps; lim.block_words = block_words;
    return fused_span_cap(n, n_uregs, lim);
}
}
