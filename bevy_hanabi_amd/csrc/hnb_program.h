// What the bytes of a program blob decide, before any device is involved: whether a caller's blob is safe to run (validate_blob), how an
// instance's slab is laid out (slab_layout), and which shortcuts the frame code may take for the program's whole life (facts). Pure host
// C++ like hnb_plan.h, whose per-frame proofs consume what facts() establishes: no device call, no global, no allocation, and no assumption
// about the alignment of the blob - hnb_program_validate takes whatever pointer a caller has, so every word is read with memcpy.
// tests/test_program_facts.py builds all of it with g++ alone, under the address and undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "hnb_dev.h"
#include "hnb_plan.h"

namespace hnb {

// Items per workgroup in the sort kernels (measured: 16384-item tiles leave the GPU under-filled at 4M keys
// and are 30 % slower overall), and tiles per group of the two-level digit offsets (the ribbon sort, hnb_sort; the slab holds their scratch).
constexpr uint32_t kSortTile = 4096;
constexpr uint32_t kSortGroup = 32;
constexpr uint32_t kSceneMaxChunks = 16;       // a program is "small" this frame: <= 65,536 slots over all of its instances ... (hnb_simulate: merged launches)

namespace program {

// ---- the validator -----------------------------------------------------------------------------------------------------
// Return code and message of a rejected blob (the C entry points copy `text` into hnb_last_error)
struct Verdict {
    int code = HNB_OK;
    char text[512] = "";
};
#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline int reject(Verdict& v, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(v.text, sizeof v.text, fmt, ap);
    va_end(ap);
    v.code = HNB_ERR_BAD_PROGRAM;
    return v.code;
}

inline Ins ins_at(const uint8_t* code, uint32_t i) {
    Ins w;
    memcpy(&w, code + (size_t)i * 8, 8);
    return w;
}

// Components of every HnbAttr (src/attributes.rs:549-675): the streaming kernels and the sort address the planes of
// POSITION / VELOCITY / AGE / LIFETIME / RIBBON_ID by these sizes, so the attribute table must agree with them.
constexpr uint8_t kAttrComponents[HNB_ATTR_COUNT] = {
    1, 1,              // ID, PARTICLE_COUNTER (pseudo, never stored)
    3, 3, 1, 1,        // POSITION, VELOCITY, AGE, LIFETIME
    1, 4, 1,           // COLOR, HDR_COLOR, ALPHA
    1, 2, 3,           // SIZE, SIZE2, SIZE3
    1, 1,              // PREV, NEXT
    3, 3, 3,           // AXIS_X, AXIS_Y, AXIS_Z
    1,                 // SPRITE_INDEX
    1, 1, 1, 1,        // F32_0..3
    2, 2, 2, 2,        // F32X2_0..3
    3, 3, 3, 3,        // F32X3_0..3
    4, 4, 4, 4,        // F32X4_0..3
    1, 1, 1, 1,        // U32_0..3
    1,                 // RIBBON_ID
};

// Operand span check: V operands must stay inside the V file, U operands inside the
// parameter block.
inline bool operand_ok(uint32_t operand, uint32_t span, uint32_t nregs, uint32_t n_uregs, bool ustream) {
    if (ustream) return operand + span <= n_uregs;
    if (operand & HNB_OPERAND_DECODED_U) return (operand & 0xffu) + span <= n_uregs;
    return operand + span <= nregs;
}

inline int validate_stream(const uint8_t* blob_base, const uint8_t* code, uint32_t len, uint32_t nregs, const HnbProgramHeader& h, int which, Verdict& v) {
    const bool ustream = which == 0;
    const char* sname = which == 0 ? "uniform" : which == 1 ? "init" : "update";
    const uint32_t file_regs = ustream ? h.n_uregs : nregs;
    for (uint32_t i = 0; i < len; ++i) {
        uint32_t w[2];
        memcpy(w, code + (size_t)i * 8, 8);
        const uint32_t op = w[0] & 0xff, d = (w[0] >> 8) & 0xff, wd = ((w[1] >> 8) & 3u) + 1u;
        // same decode as vm_exec
        const uint32_t a = ustream ? (w[0] >> 16) & 0xff : HNB_OPERAND_DECODE((w[0] >> 16) & 0xff, w[1] >> 13);
        const uint32_t b = ustream ? w[0] >> 24 : HNB_OPERAND_DECODE(w[0] >> 24, w[1] >> 14);
        const uint32_t c = ustream ? w[1] & 0xff : HNB_OPERAND_DECODE(w[1] & 0xff, w[1] >> 15);
        const bool ba = (w[1] >> 10) & 1u, bb = (w[1] >> 11) & 1u, bc = (w[1] >> 12) & 1u;
#define BAD(msg) return reject(v, "%s stream, instruction %u (op %u): %s", sname, i, op, msg)
        if (op >= HNB_OP_COUNT || op == HNB_OP_NOP) BAD("invalid opcode");
        if (op == HNB_OP_LOADK || op == HNB_OP_LDB || op == HNB_OP_LDP) {
            if (!ustream) BAD("uniform-only opcode in a per-particle stream");
            const uint32_t span = op == HNB_OP_LDP ? (a & 3u) + 1u : 1u;
            if (d + span > file_regs) BAD("destination out of range");
            if (op == HNB_OP_LDB && a > 5) BAD("bad sim-params field");
            if (op == HNB_OP_LDP && (uint64_t)w[1] + span > h.prop_words) BAD("property offset out of range");
            continue;
        }
        if (ustream && !(vm_op_is_elementwise(op) || (op >= HNB_OP_ALL && op <= HNB_OP_UNPACK4SNORM)))
            BAD("per-particle opcode in the uniform stream");
        const bool is_init = which == 1;
        if (!ustream && (d & HNB_OPERAND_U)) BAD("destination must be a V register");
        auto OK = [&](uint32_t operand, uint32_t span) { return operand_ok(operand, span, nregs, h.n_uregs, ustream); };
        if (vm_op_is_elementwise(op)) {
            const bool two = (op >= HNB_OP_FADD && op <= HNB_OP_FPOW) || (op >= HNB_OP_FLT && op <= HNB_OP_FGE) ||
                             (op >= HNB_OP_FMIX && op <= HNB_OP_FSMOOTH) || (op >= HNB_OP_IADD && op <= HNB_OP_UGE);
            const bool three = (op >= HNB_OP_FMIX && op <= HNB_OP_FSMOOTH) || op == HNB_OP_ICLAMP || op == HNB_OP_UCLAMP;
            if (d + wd > file_regs) BAD("destination out of range");
            if (!OK(a, ba ? 1 : wd)) BAD("operand a out of range");
            // b and c are read unconditionally by the interpreter: they must always be addressable
            if (!OK(b, (two && !bb) ? wd : 1)) BAD("operand b out of range");
            if (!OK(c, (three && !bc) ? wd : 1)) BAD("operand c out of range");
            continue;
        }
        switch (op) {
            case HNB_OP_LDID: case HNB_OP_LDPC: case HNB_OP_LDALIVE:
                if (d >= file_regs) BAD("destination out of range");
                break;
            case HNB_OP_LDA: case HNB_OP_STA: {
                const uint32_t ai = w[1] >> 16;
                if (ai >= h.n_attrs) BAD("attribute index out of range");
                HnbAttrEntry ae;
                memcpy(&ae, blob_base + h.attrs_off + ai * sizeof ae, sizeof ae);
                if (ae.reg != HNB_REG_NONE || ae.ncomp != wd) BAD("LDA/STA must address a whole non-pinned attribute");
                if (op == HNB_OP_LDA) { if (d + wd > file_regs) BAD("destination out of range"); }
                else if (!OK(a, ba ? 1 : wd)) BAD("operand out of range");
            } break;
            case HNB_OP_ALL: case HNB_OP_ANY: case HNB_OP_LENGTH:
                if (d >= file_regs || !OK(a, wd)) BAD("operand out of range");
                break;
            case HNB_OP_DOT: case HNB_OP_DISTANCE:
                if (d >= file_regs || !OK(a, wd) || !OK(b, wd)) BAD("operand out of range");
                break;
            case HNB_OP_NORMALIZE:
                if (d + wd > file_regs || !OK(a, wd)) BAD("operand out of range");
                break;
            case HNB_OP_CROSS:
                if (d + 3 > file_regs || !OK(a, 3) || !OK(b, 3)) BAD("operand out of range");
                break;
            case HNB_OP_PACK4UNORM: case HNB_OP_PACK4SNORM:
                if (d >= file_regs || !OK(a, 4)) BAD("operand out of range");
                break;
            case HNB_OP_UNPACK4UNORM: case HNB_OP_UNPACK4SNORM:
                if (d + 4 > file_regs || !OK(a, 1)) BAD("operand out of range");
                break;
            case HNB_OP_FRAND:
                if (d + wd > file_regs) BAD("destination out of range");
                break;
            case HNB_OP_RANDU: case HNB_OP_RANDN:
                if (d + wd > file_regs || !OK(a, ba ? 1 : wd) || !OK(b, bb ? 1 : wd)) BAD("operand out of range");
                break;
            case HNB_OP_ALIVE_SET: case HNB_OP_ALIVE_AND: case HNB_OP_KILL_IF:
            case HNB_OP_M_AGE_TICK: case HNB_OP_M_EULER: case HNB_OP_M_VEL_SCALE:
                if (!OK(a, 1)) BAD("operand out of range");
                break;
            case HNB_OP_M_VEL_ADD:
                if (!OK(a, 3)) BAD("operand out of range");
                break;
            case HNB_OP_M_PIN_SET:
                if (!(d == HNB_REG_POSITION || d == HNB_REG_VELOCITY || d == HNB_REG_AGE || d == HNB_REG_LIFETIME)) BAD("M_PIN_SET needs a pinned destination");
                if (!OK(a, (d == HNB_REG_POSITION || d == HNB_REG_VELOCITY) ? 3 : 1)) BAD("operand out of range");
                break;
            case HNB_OP_M_RADIAL_ACCEL: case HNB_OP_M_KILL_SPHERE: case HNB_OP_M_VEL_SPHERE:
                if (!OK(a, 3) || !OK(b, 1)) BAD("operand out of range");
                break;
            case HNB_OP_M_TANGENT_ACCEL:
                if (!OK(a, 3) || !OK(b, 3) || !OK(c, 1)) BAD("operand out of range");
                break;
            case HNB_OP_M_CONFORM_SPHERE:
                if (!OK(a, 9) || !OK(b, 1)) BAD("operand out of range");
                break;
            case HNB_OP_M_KILL_AABB:
                if (!OK(a, 3) || !OK(b, 3)) BAD("operand out of range");
                break;
            case HNB_OP_M_POS_CIRCLE: case HNB_OP_M_VEL_CIRCLE: case HNB_OP_M_VEL_TANGENT:
                if (!OK(a, 7)) BAD("operand out of range");
                break;
            case HNB_OP_M_POS_SPHERE:
                if (!OK(a, 4)) BAD("operand out of range");
                break;
            case HNB_OP_M_POS_CONE3D:
                if (!OK(a, 3)) BAD("operand out of range");
                break;
            case HNB_OP_M_ADD_XLATE: break;
            case HNB_OP_LDPARENT:
                if (!is_init) BAD("LDPARENT outside the init stream");
                if (d + wd > file_regs) BAD("destination out of range");
                {
                    const uint32_t id = w[1] >> 16;
                    if (id >= HNB_ATTR_COUNT || id < HNB_ATTR_POSITION) BAD("parent attribute id out of range");
                    if (wd != kAttrComponents[id]) BAD("LDPARENT must read a whole attribute");
                    bool listed = false;  // hnb_effect_set_parent checks the parent's layout against this list
                    for (uint32_t k = 0; k < h.parent_n_attrs && !listed; ++k) {
                        uint32_t pid;
                        memcpy(&pid, blob_base + h.parent_attrs_off + k * 4, 4);
                        listed = pid == id;
                    }
                    if (!listed) BAD("LDPARENT of an attribute that is not in the program's parent attribute list");
                }
                break;
            case HNB_OP_M_EMIT_EVENTS:
                if (is_init) BAD("M_EMIT_EVENTS outside the update stream");
                if (!OK(a, 1)) BAD("operand out of range");
                if (((w[1] >> 16) & 0xffu) >= h.n_event_channels) BAD("event channel out of range");
                break;
            default: BAD("unhandled opcode");
        }
#undef BAD
    }
    return HNB_OK;
}

// ---- the slab layout, as data ----------------------------------------------------------------------------------------------
// Slab layout of one effect instance: [alive list column 0][column 1][dead list][attribute planes...][alive byte per slot]
// [per-chunk lifetime bounds + "completely alive" flags][died bits][row mask][death horizons][spawn-event staging][ribbon-sort scratch],
// 256-byte aligned sections, as byte offsets. The alive list moves to the other column only in frames where particles died (k_compact).
// Every section offset is a u32 in the device structs: the layout is computed in 64 bits and rejected as a whole when it does not fit
// (offsets grow monotonically, so the total bounds every one of them).
struct SlabLayout {
    uint32_t chunks_per_inst = 0;   // ceil(capacity / kChunk)
    uint32_t sort_chunks = 0;       // ceil(capacity / kSortTile)
    uint64_t alive[2] = {}, dead = 0;
    uint64_t plane[kMaxAttrs] = {};
    uint64_t alive_flag = 0;        // alive byte per slot, zeroed with the attribute planes
    uint64_t lmin = 0;              // four u32 / f32 arrays per chunk: lifetime bound (0 = unknown), "completely alive" flag, age-cohort state, age-cohort value; zeroed too
    uint64_t died_bits = 0, row_mask = 0;   // one bit per slot "died this frame", one bit per list row "survives" (k_count_rows / k_compact)
    uint64_t horizon = 0;           // death horizons: clock, D[2][chunks], BF[2][chunks] (zero = "may die")
    uint64_t ev_cnt[HNB_MAX_EVENT_CHANNELS] = {};   // per-slot staging of spawn events (k_update_slots_generic -> k_emit_count / k_emit_events)
    bool ribbons = false;           // radix-sort scratch: 64-bit keys and values ping-pong, per-chunk digit histograms, key OR/AND
    uint64_t sort_key[2] = {}, sort_val[2] = {}, sort_hist = 0, sort_gsum = 0, sort_bits = 0;
    uint64_t total = 0;
    bool fits = false;              // (offsets are kept in 256-byte units: 1 TiB)
};
inline uint64_t align_up64(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }
inline SlabLayout slab_layout(const HnbProgramHeader& h, const HnbAttrEntry* attrs) {
    SlabLayout l;
    l.chunks_per_inst = (uint32_t)(((uint64_t)h.capacity + kChunk - 1) / kChunk);   // (in 64 bits: capacity + 4095 wraps above 4,294,963,200 slots, and a slab with no chunks would pass as small)
    uint64_t off = 0;
    const uint64_t list_bytes = align_up64((uint64_t)h.capacity * 4, 256);
    auto place = [&](uint64_t bytes) { const uint64_t at = off; off += bytes; return at; };
    l.alive[0] = place(list_bytes); l.alive[1] = place(list_bytes); l.dead = place(list_bytes);
    for (uint32_t i = 0; i < h.n_attrs; ++i) l.plane[i] = place(align_up64((uint64_t)h.capacity * attrs[i].ncomp * 4, 256));
    l.alive_flag = place(align_up64((uint64_t)h.capacity, 256));
    l.lmin = place(align_up64((uint64_t)l.chunks_per_inst * 16, 256));
    const uint64_t bit_bytes = align_up64((uint64_t)l.chunks_per_inst * (kChunk / 8), 256);
    l.died_bits = place(bit_bytes); l.row_mask = place(bit_bytes);
    l.horizon = place(align_up64(256 + (uint64_t)l.chunks_per_inst * 24, 256));
    for (uint32_t c = 0; c < h.n_event_channels; ++c) l.ev_cnt[c] = place(list_bytes);
    l.ribbons = (h.flags & HNB_PROG_HAS_RIBBONS) != 0;
    l.sort_chunks = (uint32_t)(((uint64_t)h.capacity + kSortTile - 1) / kSortTile);
    if (l.ribbons) {
        for (int i = 0; i < 2; ++i) l.sort_key[i] = place(align_up64((uint64_t)h.capacity * 8, 256));
        for (int i = 0; i < 2; ++i) l.sort_val[i] = place(list_bytes);
        l.sort_hist = place(align_up64((uint64_t)256 * l.sort_chunks * 4, 256));
        l.sort_gsum = place(align_up64((uint64_t)8 * ((l.sort_chunks + kSortGroup - 1) / kSortGroup) * 256 * 4, 256));
        l.sort_bits = place(256);
    }
    l.total = off;
    l.fits = off <= ((uint64_t)0xffffffffu << 8);
    return l;
}

inline int validate_blob(const void* blob, size_t size, HnbProgramHeader* out_hdr, Verdict& v) {
    if (!blob || size < sizeof(HnbProgramHeader)) return reject(v, "program blob too small");
    HnbProgramHeader h;
    memcpy(&h, blob, sizeof h);
    if (h.magic != HNB_PROGRAM_MAGIC) return reject(v, "bad program magic 0x%08x", h.magic);
    if (h.version != HNB_PROGRAM_VERSION) return reject(v, "unsupported program version %u", h.version);
    if (h.total_size != size) return reject(v, "program size mismatch (%u vs %zu)", h.total_size, size);
    if (h.capacity == 0) return reject(v, "capacity must be > 0");
    if (h.n_attrs == 0 || h.n_attrs > kMaxAttrs) return reject(v, "invalid attribute count %u", h.n_attrs);
    auto in_range = [&](uint64_t off, uint64_t bytes) { return off <= size && bytes <= size - off; };
    if (!in_range(h.attrs_off, (uint64_t)h.n_attrs * sizeof(HnbAttrEntry)) ||
        !in_range(h.props_off, (uint64_t)h.n_props * sizeof(HnbPropEntry)) ||
        !in_range(h.uniform_off, (uint64_t)h.uniform_len * 8) || !in_range(h.init_off, (uint64_t)h.init_len * 8) ||
        !in_range(h.update_off, (uint64_t)h.update_len * 8) || !in_range(h.parent_attrs_off, (uint64_t)h.parent_n_attrs * 4))
        return reject(v, "program section out of bounds");
    if (h.prop_words > 4ull * h.n_props) return reject(v, "%u property words for %u properties", h.prop_words, h.n_props);
    if (h.n_event_channels > HNB_MAX_EVENT_CHANNELS)
        return reject(v, "program appends to %u event channels, limit %u", h.n_event_channels, HNB_MAX_EVENT_CHANNELS);
    if (h.parent_n_attrs > HNB_ATTR_COUNT) return reject(v, "invalid parent attribute count %u", h.parent_n_attrs);
    static_assert(HNB_ATTR_COUNT <= 64, "HnbProgramHeader::render_reads_* is a 64-bit mask");
    if ((((uint64_t)h.render_reads_hi << 32) | h.render_reads_lo) >> HNB_ATTR_COUNT) return reject(v, "render_reads mask names attributes that do not exist");
    if ((h.uniform_off & 7) || (h.init_off & 7) || (h.update_off & 7)) return reject(v, "code sections must be 8-byte aligned");
    if (h.init_regs > HNB_VM_MAX_REGS_WIDE || h.update_regs > HNB_VM_MAX_REGS_WIDE)
        return reject(v, "program needs %u V registers, the VM has %u", std::max(h.init_regs, h.update_regs),
                      HNB_VM_MAX_REGS_WIDE);
    if (h.init_regs < HNB_REG_FIRST_FREE || h.update_regs < HNB_REG_FIRST_FREE)
        return reject(v, "register counts must cover the pinned registers");
    if (h.n_uregs > HNB_VM_MAX_UREGS) return reject(v, "program needs %u U registers, limit %u", h.n_uregs, HNB_VM_MAX_UREGS);
    const uint8_t* p = static_cast<const uint8_t*>(blob);
    bool has_position = false, has_age = false, has_ribbon_id = false;
    uint64_t seen = 0;
    HnbAttrEntry attrs[kMaxAttrs];
    for (uint32_t i = 0; i < h.n_attrs; ++i) {
        HnbAttrEntry& a = attrs[i];
        memcpy(&a, p + h.attrs_off + i * sizeof a, sizeof a);
        if (a.attr >= HNB_ATTR_COUNT || a.attr < HNB_ATTR_POSITION) return reject(v, "attribute %u is not storable", a.attr);
        if (a.ncomp != kAttrComponents[a.attr]) return reject(v, "attribute %u has %u components, not %u", a.attr, a.ncomp, kAttrComponents[a.attr]);
        if (seen >> a.attr & 1u) return reject(v, "attribute %u appears twice in the layout", a.attr);
        seen |= 1ull << a.attr;
        if (a.attr == HNB_ATTR_POSITION) has_position = true;
        if (a.attr == HNB_ATTR_AGE) has_age = true;
        if (a.attr == HNB_ATTR_RIBBON_ID) has_ribbon_id = true;
        const bool pinned = a.attr == HNB_ATTR_POSITION || a.attr == HNB_ATTR_VELOCITY || a.attr == HNB_ATTR_AGE ||
                            a.attr == HNB_ATTR_LIFETIME;
        const uint32_t want = a.attr == HNB_ATTR_POSITION ? HNB_REG_POSITION
                              : a.attr == HNB_ATTR_VELOCITY ? HNB_REG_VELOCITY
                              : a.attr == HNB_ATTR_AGE ? HNB_REG_AGE : HNB_REG_LIFETIME;
        if (pinned && a.reg != want) return reject(v, "pinned attribute %u in register %u", a.attr, a.reg);
        if (!pinned && a.reg != HNB_REG_NONE) return reject(v, "attribute %u must be a memory operand", a.attr);
    }
    // The POSITION attribute is mandatory (src/lib.rs:838-845).
    if (!has_position) return reject(v, "the particle layout is missing the POSITION attribute");
    // Ribbons: the flag and the RIBBON_ID attribute go together, and AGE is mandatory (src/lib.rs:846-856).
    if (((h.flags & HNB_PROG_HAS_RIBBONS) != 0) != has_ribbon_id)
        return reject(v, "HNB_PROG_HAS_RIBBONS must be set exactly when the layout has RIBBON_ID");
    if (has_ribbon_id && !has_age) return reject(v, "a layout with RIBBON_ID needs the AGE attribute");
    if (((h.flags & HNB_PROG_READS_PARENT) != 0) != (h.parent_n_attrs != 0))
        return reject(v, "HNB_PROG_READS_PARENT must be set exactly when parent attributes are listed");
    if (((h.flags & HNB_PROG_EMITS_EVENTS) != 0) != (h.n_event_channels != 0))
        return reject(v, "HNB_PROG_EMITS_EVENTS must be set exactly when the program has event channels");
    for (uint32_t i = 0; i < h.parent_n_attrs; ++i) {
        uint32_t id;
        memcpy(&id, p + h.parent_attrs_off + i * 4, 4);
        if (id >= HNB_ATTR_COUNT || id < HNB_ATTR_POSITION) return reject(v, "parent attribute %u is not storable", id);
    }
    for (uint32_t i = 0; i < h.n_props; ++i) {
        HnbPropEntry pe;
        memcpy(&pe, p + h.props_off + i * sizeof pe, sizeof pe);
        if (pe.ncomp < 1 || pe.ncomp > 4 || (uint64_t)pe.word_offset + pe.ncomp > h.prop_words) return reject(v, "bad property entry %u", i);
        if (!memchr(pe.name, 0, sizeof pe.name)) return reject(v, "unterminated property name %u", i);
    }
    int rc = validate_stream(p, p + h.uniform_off, h.uniform_len, 0, h, 0, v);
    if (rc != HNB_OK) return rc;
    rc = validate_stream(p, p + h.init_off, h.init_len, h.init_regs, h, 1, v);
    if (rc != HNB_OK) return rc;
    rc = validate_stream(p, p + h.update_off, h.update_len, h.update_regs, h, 2, v);
    if (rc != HNB_OK) return rc;
    // the instance slab is addressed with 32-bit section offsets in 256-byte units (1 TiB)
    if (!slab_layout(h, attrs).fits) return reject(v, "effect slab exceeds 1 TiB (capacity %u)", h.capacity);
    if (out_hdr) *out_hdr = h;
    return HNB_OK;
}

// ---- the creation-time facts -------------------------------------------------------------------------------------------------
// What hnb_program_create fixes in a program (hnb_ctx_set_option before the program is created; hnb_jit_precompile uses the defaults)
struct ProgramOptions {
    uint32_t age_cohort = HNB_AGE_COHORT_AUTO;   // HNB_OPT_AGE_COHORT
    bool cull_lifetime = true;                   // HNB_OPT_CULL_LIFETIME
    bool horizon = true;                         // HNB_OPT_HORIZON
};
// Waves per SIMD the streaming kernels are register-budgeted for: the lean stacks, the others, and the age-cohort instantiations
// (HNB_STREAM_WAVES / HNB_STREAM_WAVES_FULL of the kernels, HNB_STREAM_WAVES_COHORT of the runtime)
struct WaveBudget { int lean, full, cohort; };

// Streaming eligibility of an update stream: only macro ops on pinned registers, every operand in
// the parameter block, and no non-pinned attribute touched by the update program.
inline bool update_is_streamable(const uint8_t* b, const HnbProgramHeader& h, const HnbAttrEntry* attrs) {
    bool streams = true;
    for (uint32_t i = 0; i < h.update_len; ++i) {
        uint32_t w[2];
        memcpy(w, b + h.update_off + (size_t)i * 8, 8);
        const uint32_t op = w[0] & 0xffu, a = (w[0] >> 16) & 0xffu, bb = w[0] >> 24, c = w[1] & 0xffu;
        bool ok = vm_op_is_streamable(op) && (a & HNB_OPERAND_U);
        if (ok && (op == HNB_OP_M_RADIAL_ACCEL || op == HNB_OP_M_TANGENT_ACCEL || op == HNB_OP_M_CONFORM_SPHERE ||
                   op == HNB_OP_M_KILL_SPHERE || op == HNB_OP_M_KILL_AABB))
            ok = (bb & HNB_OPERAND_U) != 0;
        if (ok && op == HNB_OP_M_TANGENT_ACCEL) ok = (c & HNB_OPERAND_U) != 0;
        if (!ok) streams = false;
    }
    for (uint32_t i = 0; i < h.n_attrs; ++i)
        if (attrs[i].update_flags && attrs[i].reg == HNB_REG_NONE) streams = false;
    return streams;
}

// Lifetime culling (hnb_kernels): the streaming update reads LIFETIME only for the AGE_TICK's `age < lifetime`.
// Eligible: the stream starts with the only AGE_TICK, which tests the lifetime; nothing else writes AGE or LIFETIME. The age
// cohorts rest on the same structure (nothing but that one AGE_TICK changes AGE) and on nobody else reading the AGE plane on
// the device (no ribbon sort).
inline bool cull_eligible(const uint8_t* b, const HnbProgramHeader& h, const HnbAttrEntry* attrs, bool streams, const ProgramOptions& opt, uint32_t* dt_operand) {
    if (!streams || h.update_len == 0 || !opt.cull_lifetime) return false;
    const uint8_t* uc = b + h.update_off;
    const Ins first = ins_at(uc, 0);
    bool ok = (first.x & 0xffu) == HNB_OP_M_AGE_TICK && ((first.y >> 16) & 1u);
    for (uint32_t i = 1; i < h.update_len && ok; ++i) {
        const Ins in = ins_at(uc, i);
        const uint32_t op = in.x & 0xffu, dst = (in.x >> 8) & 0xffu;
        if (op == HNB_OP_M_AGE_TICK) ok = false;
        if (op == HNB_OP_M_PIN_SET && (dst == HNB_REG_AGE || dst == HNB_REG_LIFETIME)) ok = false;
    }
    bool loads_life = false, stores_life = false, has_age = false;
    for (uint32_t a = 0; a < h.n_attrs; ++a) {
        if (attrs[a].reg == HNB_REG_LIFETIME) { loads_life = (attrs[a].update_flags & HNB_ATTR_UPD_LOAD) != 0; stores_life = (attrs[a].update_flags & HNB_ATTR_UPD_STORE) != 0; }
        if (attrs[a].reg == HNB_REG_AGE) has_age = (attrs[a].update_flags & HNB_ATTR_UPD_LOAD) != 0;
    }
    if (!(ok && loads_life && !stores_life && has_age)) return false;
    if (dt_operand) *dt_operand = HNB_OPERAND_DECODE((first.x >> 16) & 0xffu, first.y >> 13);
    return true;
}
// the update consists of lean (bandwidth-bound) macro ops only
inline bool update_is_lean(const uint8_t* b, const HnbProgramHeader& h) {
    for (uint32_t i = 0; i < h.update_len; ++i)
        if (!vm_op_is_lean(ins_at(b + h.update_off, i).x & 0xffu)) return false;
    return true;
}
constexpr uint32_t kAutoMaterialiseMinSlots = kSceneMaxChunks * kChunk;   // HNB_AGE_COHORT_AUTO: from this capacity on (65,536: an instance no longer "small" for the merged launches) an AGE-reading asset keeps the cohorts and its update keeps the plane current
inline bool age_cohort_eligible(const uint8_t* b, const HnbProgramHeader& h, const HnbAttrEntry* attrs, bool streams, const ProgramOptions& opt) {
    if (!cull_eligible(b, h, attrs, streams, opt, nullptr) || (h.flags & HNB_PROG_HAS_RIBBONS) || opt.age_cohort == HNB_AGE_COHORT_OFF) return false;
    // HNB_AGE_COHORT_AUTO (the default) chooses from the asset: where the RENDER modifiers read AGE after every frame (HnbProgramHeader::
    // render_reads_*: ColorOverLifetime / SizeOverLifetime, src/modifier/output.rs:310-312) the plane must be current after every frame.
    // Effects of 65,536 slots or more per instance keep the cohorts and their update kernel writes the common age of a cohort chunk into the plane
    // as it goes (SlotArgs::age_current: write-only, 4 of the 8 bytes per particle the cohort saves; round 5 ran a k_materialise_age pass behind
    // every update instead - one more launch and 16 us per frame at 16.7M particles - and only from 2^20 slots on). Smaller ones - the programs
    // that share the merged launches of a scene - keep their ages in the plane: at those sizes the bytes do not matter and the cohort
    // instantiation only costs registers. Assets whose renderer does not read AGE get LEAN.
    if (opt.age_cohort == HNB_AGE_COHORT_AUTO && (h.render_reads_lo >> HNB_ATTR_AGE & 1u) && h.capacity < kAutoMaterialiseMinSlots) return false;
    // only the lean (bandwidth-bound) stacks: an update that is bound by VALU issue (ConformToSphere, Radial / TangentAccel: divisions, square
    // roots) gains nothing from 8 bytes less per particle and pays for the bookkeeping (force_field: 0.0955 -> 0.099 ms with it, measured)
    // (HNB_AGE_COHORT_ALL: every eligible stack, for A/B runs)
    if (opt.age_cohort == HNB_AGE_COHORT_ALL) return true;
    return update_is_lean(b, h);
}

// Slot-major init of large spawns (hnb_kernels): what a spawn writes must not depend on its rank among the frame's spawns
inline bool slot_init_eligible(const uint8_t* b, const HnbProgramHeader& h) {
    if (h.flags & (HNB_PROG_HAS_RIBBONS | HNB_PROG_READS_PARENT)) return false;
    for (uint32_t i = 0; i < h.init_len; ++i) {
        const uint32_t op = ins_at(b + h.init_off, i).x & 0xffu;
        if (op == HNB_OP_LDPC || op == HNB_OP_LDPARENT) return false;
    }
    return true;
}

// The static part of the ribbon proofs of a streamable ribbon program: "the head stays sorted" (plan::RibbonFacts::provable) and
// "the spawns sort in front" (front_static)
inline plan::RibbonFacts ribbon_facts(const uint8_t* b, const HnbProgramHeader& h, const HnbAttrEntry* attrs) {
    plan::RibbonFacts rf;
    bool ok = true;
    uint32_t ticks = 0;
    const uint8_t* uc = b + h.update_off;
    for (uint32_t i = 0; i < h.update_len && ok; ++i) {
        const Ins in = ins_at(uc, i);
        const uint32_t op = in.x & 0xffu, dst = (in.x >> 8) & 0xffu;
        if (op == HNB_OP_M_AGE_TICK) { ticks += 1; rf.tick_operand = HNB_OPERAND_DECODE((in.x >> 16) & 0xffu, in.y >> 13); ok = (rf.tick_operand & HNB_OPERAND_DECODED_U) != 0; }
        if (op == HNB_OP_M_PIN_SET && dst == HNB_REG_AGE) ok = false;
    }
    ok = ok && ticks == 1;
    for (uint32_t a = 0; a < h.n_attrs; ++a)   // (a streamable update touches no non-pinned attribute, RIBBON_ID included)
        if (attrs[a].attr == HNB_ATTR_RIBBON_ID && (attrs[a].update_flags & HNB_ATTR_UPD_STORE)) ok = false;
    const uint8_t* ic = b + h.init_off;
    for (uint32_t i = 0; i < h.init_len && ok; ++i) {
        const Ins in = ins_at(ic, i);
        const uint32_t op = in.x & 0xffu, dst = (in.x >> 8) & 0xffu, wd = ((in.y >> 8) & 3u) + 1u;
        if (op == HNB_OP_M_PIN_SET && dst == HNB_REG_AGE) {
            rf.age_init_operand = HNB_OPERAND_DECODE((in.x >> 16) & 0xffu, in.y >> 13);
            rf.age_init_set = true;
            ok = (rf.age_init_operand & HNB_OPERAND_DECODED_U) != 0;   // a per-particle age could be negative: key order != age order
        } else if (op != HNB_OP_STA && op != HNB_OP_ALIVE_SET && op != HNB_OP_ALIVE_AND && op != HNB_OP_KILL_IF && !(op >= HNB_OP_M_AGE_TICK) &&
                   dst <= HNB_REG_AGE && dst + wd > HNB_REG_AGE) {
            ok = false;  // some other instruction writes the AGE register
        }
    }
    rf.provable = ok;
    // the front proof (see plan::RibbonFacts::front_static): RIBBON_ID stored at most once by the init, from a uniform value
    int rid_index = -1;
    for (uint32_t a = 0; a < h.n_attrs; ++a) if (attrs[a].attr == HNB_ATTR_RIBBON_ID) rid_index = (int)a;
    uint32_t rid_stores = 0;
    bool front = ok && rid_index >= 0;
    for (uint32_t i = 0; i < h.init_len && front; ++i) {
        const Ins in = ins_at(ic, i);
        const uint32_t op = in.x & 0xffu;
        if (op == HNB_OP_STA && (in.y >> 16) == (uint32_t)rid_index) {
            rid_stores += 1;
            rf.rid_operand = HNB_OPERAND_DECODE((in.x >> 16) & 0xffu, in.y >> 13);
            front = (rf.rid_operand & HNB_OPERAND_DECODED_U) != 0;
        }
    }
    rf.rid_set = rid_stores == 1;
    // ... and every spawn must still be in the list when it is sorted (the rotation moves exactly `spawned` rows): nothing but old age
    // kills, and the lifetime - one uniform value, compared with the tick per frame - outlasts the first frame
    uint32_t life_sets = 0;
    for (uint32_t i = 0; i < h.init_len && front; ++i) {
        const Ins in = ins_at(ic, i);
        const uint32_t op = in.x & 0xffu, dst = (in.x >> 8) & 0xffu, wd = ((in.y >> 8) & 3u) + 1u;
        if (op == HNB_OP_M_PIN_SET && dst == HNB_REG_LIFETIME) {
            life_sets += 1;
            rf.life_operand = HNB_OPERAND_DECODE((in.x >> 16) & 0xffu, in.y >> 13);
            front = (rf.life_operand & HNB_OPERAND_DECODED_U) != 0;
        } else if (op != HNB_OP_STA && op != HNB_OP_ALIVE_SET && op != HNB_OP_ALIVE_AND && op != HNB_OP_KILL_IF && !(op >= HNB_OP_M_AGE_TICK) &&
                   dst <= HNB_REG_LIFETIME && dst + wd > HNB_REG_LIFETIME) {
            front = false;  // some other instruction writes the LIFETIME register
        }
    }
    for (uint32_t i = 0; i < h.update_len && front; ++i) {
        const Ins in = ins_at(uc, i);
        const uint32_t op = in.x & 0xffu, dst = (in.x >> 8) & 0xffu;
        if (op == HNB_OP_M_KILL_SPHERE || op == HNB_OP_M_KILL_AABB || op == HNB_OP_KILL_IF || op == HNB_OP_ALIVE_SET || op == HNB_OP_ALIVE_AND) front = false;
        if (op == HNB_OP_M_PIN_SET && dst == HNB_REG_LIFETIME) front = false;
    }
    rf.front_static = front && rid_stores <= 1 && life_sets == 1;
    return rf;
}

// Everything program creation decides from the blob, the options that are fixed in a program, and the context's list order. Values only:
// nothing here points into the blob.
struct ProgramFacts {
    bool has_ribbons = false;           // layout has RIBBON_ID: the alive list is sorted after every update (hnb_sort)
    bool slot_order = false;            // HNB_LIST_ORDER_SLOT: lists rebuilt in slot order every frame (ribbons are re-sorted anyway)
    bool wide_file = false;             // init_regs / update_regs above HNB_VM_MAX_REGS: generic kernels use the wide V file
    bool update_streams = false;        // update stream runs on the streaming kernel (macro ops, U operands)
    bool slot_init_eligible = false;    // the init reads neither PARTICLE_COUNTER nor a parent particle, no ribbons: large spawns may run slot-major (plan::plan_slot_init)
    bool cull_lifetime = false;         // the streaming update keeps the chunks' lifetime bounds up to date and uses them
    uint32_t cull_dt_operand = 0;       // lifetime culling: decoded operand a of the update stream's AGE_TICK
    bool age_cohort = false;            // chunks whose alive particles share one AGE keep it in a word (hnb_kernels "Age cohorts")
    bool auto_materialise = false;      // HNB_AGE_COHORT_AUTO, the render modifiers read AGE and the effect is large: cohorts, and the update keeps the plane current (SlotArgs::age_current)
    bool lean = false;                  // every op of the update is bandwidth-bound (vm_op_is_lean)
    int stream_waves = 0;               // waves per SIMD a streaming kernel specialised for this update is budgeted for
    bool kills = false;                 // the update has a kill modifier (KillSphere / KillAabb): particles die by more than their lifetime
    plan::RibbonFacts ribbon;           // what program creation established about AGE / RIBBON_ID / LIFETIME of a ribbon effect
    plan::SkipFacts skip;               // list-free frames: eligible = streamable, lifetime-culled, no kill modifier, no spawn events in or out
    bool horizon_eligible = false;      // streamable, lifetime-culled, no kill modifier, no ribbons: row-chunk death horizons are maintained (hnb_kernels)
};
inline ProgramFacts facts(const uint8_t* b, const HnbProgramHeader& h, const HnbAttrEntry* attrs, const ProgramOptions& opt, bool list_order_slot, const WaveBudget& waves) {
    ProgramFacts f;
    f.has_ribbons = (h.flags & HNB_PROG_HAS_RIBBONS) != 0;
    f.slot_order = list_order_slot && !f.has_ribbons;
    f.wide_file = std::max(h.init_regs, h.update_regs) > HNB_VM_MAX_REGS;
    f.update_streams = update_is_streamable(b, h, attrs);
    f.slot_init_eligible = slot_init_eligible(b, h);
    f.cull_lifetime = cull_eligible(b, h, attrs, f.update_streams, opt, &f.cull_dt_operand);
    f.age_cohort = age_cohort_eligible(b, h, attrs, f.update_streams, opt);
    f.auto_materialise = opt.age_cohort == HNB_AGE_COHORT_AUTO && f.age_cohort && (h.render_reads_lo >> HNB_ATTR_AGE & 1u) != 0u;
    f.lean = update_is_lean(b, h);
    f.stream_waves = f.lean ? waves.lean : waves.full;
    if (f.age_cohort && f.stream_waves > waves.cohort) f.stream_waves = waves.cohort;
    for (uint32_t i = 0; i < h.update_len; ++i) {
        const uint32_t op = ins_at(b + h.update_off, i).x & 0xffu;
        f.kills = f.kills || op == HNB_OP_M_KILL_SPHERE || op == HNB_OP_M_KILL_AABB;
    }
    if (f.has_ribbons && f.update_streams) f.ribbon = ribbon_facts(b, h, attrs);
    f.skip.eligible = f.update_streams && f.cull_lifetime && !f.kills && h.n_event_channels == 0 && !(h.flags & HNB_PROG_READS_PARENT);
    f.skip.dt_operand = f.cull_dt_operand;
    f.horizon_eligible = f.update_streams && f.cull_lifetime && !f.kills && !f.has_ribbons && !f.slot_order && opt.horizon;
    return f;
}

}  // namespace program
}  // namespace hnb
