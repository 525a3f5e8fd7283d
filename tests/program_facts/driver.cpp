// TEST-ONLY: csrc/hnb_program.h on the host, built by tests/test_program_facts.py with g++ and the address / undefined-behaviour sanitizers.
//   driver validate <file>   records [u32 size][bytes]: rc and text of program::validate_blob for every blob, each copied into a heap buffer of
//                            exactly its size (an out-of-bounds read is a report) and run a second time at an odd address (buffer + 1)
//   driver layout            stdin lines "capacity n_attrs n_channels ribbons": program::slab_layout, every section offset
//   driver facts <file>      records [u32 size][u32 age_cohort][u32 cull_lifetime][u32 horizon][u32 list_order_slot][bytes]: program::facts
//   driver ribbon <file>     the same records: program::ribbon_facts alone, whether or not the update streams (facts() asks that first)
//   driver reject <n>        program::reject with a message of n characters: what is left of it
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "hnb_program.h"

using namespace hnb;

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static uint32_t word(const std::vector<uint8_t>& d, size_t at) {
    uint32_t w;
    if (at + 4 > d.size()) { fprintf(stderr, "truncated input\n"); exit(2); }
    memcpy(&w, d.data() + at, 4);
    return w;
}

static int run_validate(const char* path) {
    const std::vector<uint8_t> d = slurp(path);
    for (size_t at = 0; at < d.size();) {
        const uint32_t n = word(d, at);
        at += 4;
        if (at + n > d.size()) return 2;
        uint8_t* exact = static_cast<uint8_t*>(malloc(n));              // (size 0: the validator must not read a byte)
        uint8_t* odd = static_cast<uint8_t*>(malloc((size_t)n + 1));
        memcpy(exact, d.data() + at, n);
        memcpy(odd + 1, d.data() + at, n);
        program::Verdict v, w;
        HnbProgramHeader h0, h1;
        const int rc = program::validate_blob(exact, n, &h0, v);
        const int rc_odd = program::validate_blob(odd + 1, n, &h1, w);
        if (rc != v.code || rc_odd != w.code || rc != rc_odd || strcmp(v.text, w.text) != 0) {
            fprintf(stderr, "the verdict depends on the address: %d '%s' vs %d '%s'\n", rc, v.text, rc_odd, w.text);
            return 3;
        }
        printf("%d\t%s\n", rc, v.text);
        free(exact);
        free(odd);
        at += n;
    }
    return 0;
}

static int run_layout() {
    unsigned long long cap, n_attrs, n_ch, ribbons;
    while (scanf("%llu %llu %llu %llu", &cap, &n_attrs, &n_ch, &ribbons) == 4) {
        HnbProgramHeader h{};
        h.capacity = (uint32_t)cap; h.n_attrs = (uint32_t)n_attrs; h.n_event_channels = (uint32_t)n_ch; h.flags = ribbons ? HNB_PROG_HAS_RIBBONS : 0u;
        HnbAttrEntry attrs[kMaxAttrs] = {};
        for (uint32_t i = 0; i < h.n_attrs; ++i) attrs[i].ncomp = (uint8_t)(1 + i % 4);   // components 1, 2, 3, 4, 1, ...
        const program::SlabLayout l = program::slab_layout(h, attrs);
        printf("%u %u %d %llu %d", l.chunks_per_inst, l.sort_chunks, l.ribbons ? 1 : 0, (unsigned long long)l.total, l.fits ? 1 : 0);
        auto put = [](uint64_t v) { printf(" %llu", (unsigned long long)v); };
        put(l.alive[0]); put(l.alive[1]); put(l.dead);
        for (uint32_t i = 0; i < h.n_attrs; ++i) put(l.plane[i]);
        put(l.alive_flag); put(l.lmin); put(l.died_bits); put(l.row_mask); put(l.horizon);
        for (uint32_t c = 0; c < h.n_event_channels; ++c) put(l.ev_cnt[c]);
        if (l.ribbons) { put(l.sort_key[0]); put(l.sort_key[1]); put(l.sort_val[0]); put(l.sort_val[1]); put(l.sort_hist); put(l.sort_gsum); put(l.sort_bits); }
        printf("\n");
    }
    return 0;
}

static int run_facts(const char* path, bool ribbon_only) {
    const std::vector<uint8_t> d = slurp(path);
    const program::WaveBudget waves = {6, 5, 4};
    for (size_t at = 0; at < d.size();) {
        const uint32_t n = word(d, at);
        program::ProgramOptions opt;
        opt.age_cohort = word(d, at + 4); opt.cull_lifetime = word(d, at + 8) != 0; opt.horizon = word(d, at + 12) != 0;
        const bool list_order_slot = word(d, at + 16) != 0;
        at += 20;
        if (at + n > d.size()) return 2;
        uint8_t* odd = static_cast<uint8_t*>(malloc((size_t)n + 1));   // exactly its size, at an odd address
        uint8_t* b = odd + 1;
        memcpy(b, d.data() + at, n);
        at += n;
        program::Verdict v;
        HnbProgramHeader h;
        if (program::validate_blob(b, n, &h, v) != HNB_OK) { printf("rejected %s\n", v.text); free(odd); continue; }
        HnbAttrEntry attrs[kMaxAttrs];
        memcpy(attrs, b + h.attrs_off, h.n_attrs * sizeof(HnbAttrEntry));
        if (ribbon_only) {
            const plan::RibbonFacts r = program::ribbon_facts(b, h, attrs);
            printf("provable=%d front_static=%d age_init_set=%d rid_set=%d tick_operand=%u age_init_operand=%u rid_operand=%u life_operand=%u\n", r.provable, r.front_static,
                   r.age_init_set, r.rid_set, r.tick_operand, r.age_init_operand, r.rid_operand, r.life_operand);
            free(odd);
            continue;
        }
        const program::ProgramFacts f = program::facts(b, h, attrs, opt, list_order_slot, waves);
        printf("has_ribbons=%d slot_order=%d wide_file=%d update_streams=%d slot_init_eligible=%d cull_lifetime=%d cull_dt_operand=%u age_cohort=%d auto_materialise=%d "
               "lean=%d stream_waves=%d kills=%d provable=%d front_static=%d age_init_set=%d rid_set=%d tick_operand=%u age_init_operand=%u rid_operand=%u life_operand=%u "
               "skip_eligible=%d skip_dt_operand=%u horizon_eligible=%d\n",
               f.has_ribbons, f.slot_order, f.wide_file, f.update_streams, f.slot_init_eligible, f.cull_lifetime, f.cull_dt_operand, f.age_cohort, f.auto_materialise,
               f.lean, f.stream_waves, f.kills, f.ribbon.provable, f.ribbon.front_static, f.ribbon.age_init_set, f.ribbon.rid_set, f.ribbon.tick_operand,
               f.ribbon.age_init_operand, f.ribbon.rid_operand, f.ribbon.life_operand, f.skip.eligible, f.skip.dt_operand, f.horizon_eligible);
        free(odd);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "validate")) return run_validate(argv[2]);
    if (argc >= 2 && !strcmp(argv[1], "layout")) return run_layout();
    if (argc >= 3 && !strcmp(argv[1], "facts")) return run_facts(argv[2], false);
    if (argc >= 3 && !strcmp(argv[1], "ribbon")) return run_facts(argv[2], true);
    if (argc >= 3 && !strcmp(argv[1], "reject")) {
        const std::vector<char> msg(std::vector<char>::size_type(atoi(argv[2])), 'x');
        program::Verdict v;
        const int rc = program::reject(v, "%.*s", (int)msg.size(), msg.data());
        printf("%d %d %zu %s\n", rc, v.code, strlen(v.text), v.text);
        return 0;
    }
    return 2;
}
