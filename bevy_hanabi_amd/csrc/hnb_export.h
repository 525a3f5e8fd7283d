// The packed exports (hnb_effect_export, hnb_program_export, their _sorted forms - with an HnbExportSort or an HnbExportSortFiltered -,
// hnb_effect_export_filtered, hnb_effect_export_filtered_sorted, hnb_program_export_filtered; include/hanabi_amd.h "Packed output"), shared by the
// kernels' translation units (hnb_export.hip, hnb_export_sort.hip, hnb_export_filter.hip, hnb_export_cull.hip, hnb_export_filter_prog.hip,
// hnb_export_cull_prog.hip: a code object each) and the runtime that loads and launches them (hanabi_amd.hip): the kernels' argument blocks, the
// sort's pass and (instance, slot) arithmetic, the scratch layouts, the kernels by name (ExportKernel) and the launches of a call
// (export_launch_plan). Plain C++ below the argument blocks: a host compiler takes it, so the tests check the layouts and the plan without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/hanabi_amd.h"
#include "hnb_sort_key.h"

namespace hnb {

constexpr uint32_t kExportBlock = 256;         // lanes per workgroup: one list row per lane and pass
constexpr uint32_t kExportMaxStride = 256;     // bytes per record
constexpr uint32_t kExportIdField = 0x100u;    // ExportFieldArg::ncomp_flags: the field is HNB_ATTR_ID (slot_base + slot, no plane)

struct ExportFieldArg {
    uint64_t plane_off;      // bytes from an instance's slab base
    uint32_t dst_dw;         // dwords from the record's start
    uint32_t ncomp_flags;    // bits 0..2: components of 4 bytes; kExportIdField
};

struct ExportArgs {
    const uint64_t* slabs;          // [n_instances] slab base addresses
    const HnbDeviceMeta* meta;      // [n_instances] rows after the frames enqueued so far
    const uint32_t* offsets;        // program form: [n_instances + 1] first record of every instance (k_export_offsets); NULL: one instance, record 0
    const uint32_t* slot_bases;     // program form with an ID field: [n_instances]; NULL: slot_base below
    uint32_t* out_count;            // effect form: [0] = records written, [1] = alive rows found (the program form's are written by k_export_offsets); may be NULL
    uint32_t* dst;                  // 16-byte aligned
    uint64_t dst_capacity;          // records
    uint64_t alive_off[2];          // bytes from the slab base
    uint64_t pad_mask;              // bit d: dword d of a record is covered by no field (written as zero)
    uint32_t capacity, stride_dw, n_fields, tile_rows, slot_base;
    uint32_t order_pitch;           // sorted export: slots between the two value buffers below
    ExportFieldArg fields[HNB_EXPORT_MAX_FIELDS];
    const uint32_t* order;          // sorted export (k_export_sort_rows_*): the value buffers [2][order_pitch] of the sort, row r of the result = record r;
    const uint32_t* order_state;    //   the sort's ExportSortState words say which of the two holds the result. NULL for k_export_rows_*: the list is read
    uint32_t n_inst, slot_bits;     // sorted program export, program scope (k_export_sort_rows_all_*): order[r] = export_sort_pack(instance, slot, slot_bits)
    uint32_t total_cap;             //   ... and n_inst * capacity, the bound of the concatenated row space
};

// The four instantiations of k_export_rows by the LDS image they declare: records of up to 32 / 64 / 128 bytes in tiles of 256 rows, up to 256 bytes in
// tiles of 128 rows. At most 32 KiB per workgroup.
constexpr uint32_t kExportVariants = 4;
inline uint32_t export_variant(uint32_t stride_bytes) { return stride_bytes <= 32u ? 0u : stride_bytes <= 64u ? 1u : stride_bytes <= 128u ? 2u : 3u; }
inline uint32_t export_tile_rows(uint32_t variant) { return variant == 3u ? 128u : 256u; }


// ---- sorted export (hnb_effect_export_sorted, hnb_program_export_sorted; kernels: hnb_export_sort.hip, a second code object) ----
// A least-significant-digit radix sort of (key, slot) pairs, 8 bits per pass, tiles of 4096 rows, digit offsets on two levels (per tile, and per
// group of 32 tiles) as in hnb_sort.hip.h: no workgroup waits for another.
constexpr uint32_t kExportSortTile = 4096;     // rows per workgroup
constexpr uint32_t kExportSortGroup = 32;      // tiles per group of the two-level digit offsets
constexpr uint32_t kExportSortPasses = 4;      // 32-bit keys

struct ExportSortState {        // zeroed in front of the keys kernel
    uint32_t or_keys;           // OR of every key
    uint32_t or_not_keys;       // OR of every complemented key: a bit set in both differs between two keys
    uint32_t pad[2];
};

struct ExportSortArgs {
    const uint64_t* slab;           // [1] the instance's slab base address
    const HnbDeviceMeta* meta;      // [1] its row after the frames enqueued so far
    uint32_t* keys;                 // [2][pitch] ping-pong
    uint32_t* vals;                 // [2][pitch] slots, ping-pong
    uint32_t* hist;                 // [4 digits][tiles][256]: per-tile digit counts
    uint32_t* gsum;                 // [2][4 digits][groups][256]: digit counts per group of tiles; set 0 from the keys kernel (rows in list order), set 1 from
                                    //   k_export_sort_hist (rows as the earlier passes left them); zeroed in front of the keys kernel
    ExportSortState* state;
    uint64_t alive_off[2];          // bytes from the slab base
    uint64_t plane_off;             // the key source: the POSITION plane (DEPTH, DISTANCE) or the scalar attribute's
    uint32_t capacity, pitch, tiles, groups;
    uint32_t key;                   // HNB_SORT_KEY_*
    uint32_t is_f32;                // HNB_SORT_KEY_ATTR: the plane holds f32
    uint32_t descending;
    float v[3];
    // sorted program export (hnb_program_export_sorted). Instance scope: keys, vals, hist, gsum and state hold one section per instance, instance k's
    // at k times the size the members above describe; slab and meta are the program's tables. Program scope: one row space of all instances, pitch /
    // tiles / groups are those of n_inst * capacity rows.
    uint32_t n_inst, slot_bits;     // program scope: vals hold export_sort_pack(instance, slot, slot_bits)
    const uint32_t* offsets;        // program scope: [n_inst + 1] first row of every instance in the concatenated space (k_export_offsets), [n_inst] = rows in all
    uint32_t total_cap;             // program scope: n_inst * capacity
};

struct ExportSortPass { bool active; uint32_t ran, src; };
// Pass p (0..3) of the sort: whether it runs at all (its digit differs between two keys), how many passes ran before it, and which ping-pong
// buffer it reads; p = 4 gives the buffer that holds the result.
HNB_SORT_KEY_FN ExportSortPass export_sort_pass(uint32_t varying, uint32_t pass) {
    ExportSortPass r;
    r.ran = 0;
    for (uint32_t q = 0; q < pass; ++q) r.ran += ((varying >> (8u * q)) & 0xffu) ? 1u : 0u;
    r.active = pass < kExportSortPasses && ((varying >> (8u * (pass & 3u))) & 0xffu) != 0u;
    r.src = r.ran & 1u;
    return r;
}

// Program scope of the sorted program export: one 32-bit value names (instance, slot). slot_bits = ceil(log2(capacity)); the instance sits above
// them, so the values are ordered like the pairs. A program fits when n_inst << slot_bits <= 2^32.
HNB_SORT_KEY_FN uint32_t export_sort_slot_bits(uint32_t capacity) {
    uint32_t b = 0;
    while (b < 32u && (1ull << b) < (uint64_t)capacity) ++b;
    return b;
}
HNB_SORT_KEY_FN bool export_sort_pack_fits(uint64_t n_inst, uint32_t capacity) {
    const uint32_t b = export_sort_slot_bits(capacity);
    return n_inst <= (1ull << (32u - b));
}
HNB_SORT_KEY_FN uint32_t export_sort_pack(uint32_t instance, uint32_t slot, uint32_t slot_bits) { return slot_bits >= 32u ? slot : (instance << slot_bits) | slot; }
HNB_SORT_KEY_FN uint32_t export_sort_unpack_instance(uint32_t v, uint32_t slot_bits) { return slot_bits >= 32u ? 0u : v >> slot_bits; }
HNB_SORT_KEY_FN uint32_t export_sort_unpack_slot(uint32_t v, uint32_t slot_bits) { return slot_bits >= 32u ? v : v & ((1u << slot_bits) - 1u); }

HNB_SORT_KEY_FN const uint32_t* export_order_of(const ExportArgs& a) {
    const uint32_t varying = a.order_state[0] & a.order_state[1];
    return a.order + (size_t)export_sort_pass(varying, kExportSortPasses).src * a.order_pitch;
}
// ... of instance k in the instance scope of the sorted program export: its section of the value buffers, by its own state words
HNB_SORT_KEY_FN const uint32_t* export_order_of_instance(const ExportArgs& a, uint32_t k) {
    const uint32_t* st = a.order_state + (size_t)k * (sizeof(ExportSortState) / 4u);
    return a.order + ((size_t)k * 2u + export_sort_pass(st[0] & st[1], kExportSortPasses).src) * a.order_pitch;
}


// ---- filtered export (hnb_effect_export_filtered; kernels: hnb_export_filter.hip, a third code object) ----
// A stable compaction of the alive list by a predicate, over tiles of the sort's size: mark (one bit per row, one count per tile), an exclusive scan of
// the tile counts by one workgroup, compact (order[offset + rank] = slot). The gather then reads ExportArgs::order (one buffer, order_pitch unused) and
// takes its row count from ExportArgs::order_state[0], the kept total. No workgroup waits for another.
constexpr uint32_t kExportFilterTile = kExportSortTile;                  // rows per workgroup
constexpr uint32_t kExportFilterTileWords = kExportFilterTile / 64u;     // 64-bit mask words per tile: one per wave and round

struct ExportFilterArgs {
    const uint64_t* slab;           // [1] the instance's slab base address
    const HnbDeviceMeta* meta;      // [1] its row after the frames enqueued so far
    uint32_t* order;                // [capacity] slots of the kept rows, in list order
    uint64_t* mask;                 // [tiles][kExportFilterTileWords] bit r % 64 of word r / 64: list row r is kept
    uint32_t* tile_count;           // [tiles] kept rows of a tile (k_export_filter_mark)
    uint32_t* tile_offset;          // [tiles] kept rows of the tiles in front of it (k_export_filter_scan)
    uint32_t* state;                // [0] = kept rows in all
    uint64_t alive_off[2];          // bytes from the slab base
    uint64_t plane_off;             // the predicate's source: the POSITION plane (PLANES, SPHERE) or the scalar attribute's
    uint32_t capacity, tiles;
    uint32_t kind;                  // HNB_FILTER_*
    uint32_t n_planes, is_f32, invert, lo_bits, hi_bits;
    float P[HNB_FILTER_MAX_PLANES][4];
};

// The scratch of an effect's filtered exports, one allocation; every section starts on a 256-byte boundary. 4 bytes per slot of capacity (order) and,
// per tile of 4096 slots, 512 bytes of mask and two words.
struct ExportFilterScratch { uint32_t tiles; uint64_t order_off, order_bytes, mask_off, mask_bytes, count_off, count_bytes, offset_off, offset_bytes, state_off, state_bytes, total; };
HNB_SORT_KEY_FN ExportFilterScratch export_filter_scratch_layout(uint32_t capacity) {
    ExportFilterScratch l;
    l.tiles = (uint32_t)(((uint64_t)capacity + kExportFilterTile - 1u) / kExportFilterTile);
    l.order_off = 0;
    l.order_bytes = (uint64_t)capacity * 4u;
    l.mask_off = (l.order_off + l.order_bytes + 255u) & ~(uint64_t)255u;
    l.mask_bytes = (uint64_t)l.tiles * kExportFilterTileWords * 8u;
    l.count_off = (l.mask_off + l.mask_bytes + 255u) & ~(uint64_t)255u;
    l.count_bytes = (uint64_t)l.tiles * 4u;
    l.offset_off = (l.count_off + l.count_bytes + 255u) & ~(uint64_t)255u;
    l.offset_bytes = (uint64_t)l.tiles * 4u;
    l.state_off = (l.offset_off + l.offset_bytes + 255u) & ~(uint64_t)255u;
    l.state_bytes = 16u;
    l.total = l.state_off + 256u;
    return l;
}

// The scratch of a sorted export, one allocation; every section starts on a 256-byte boundary. `sections` sections of `rows` rows in every buffer:
// u32 keys[sections][2][pitch], u32 vals likewise (16 bytes per row), then - all of it zeroed in front of every multi-tile sort - an ExportSortState and
// u32 gsum[2][4][groups][256] per section, and last u32 hist[4][tiles][256] per section, which the kernels write before they read it. Instance scope:
// one section of `capacity` rows per instance (an effect's own sort is n_inst = 1). Program scope: one section of n_inst * capacity rows.
// rows == 0: more than 0xFFFFFF00 rows in a section, which 32 bits of pitch do not hold.
struct ExportSortScratch { uint32_t sections, rows, pitch, tiles, groups; uint64_t vals_off, state_off, gsum_off, hist_off, zero_bytes, total; };
HNB_SORT_KEY_FN ExportSortScratch export_sort_scratch_layout(uint32_t n_inst, uint32_t capacity, uint32_t scope) {
    ExportSortScratch l = {};
    const uint64_t rows = scope == HNB_SORT_SCOPE_PROGRAM ? (uint64_t)n_inst * capacity : capacity;
    if (rows > 0xFFFFFF00ull) return l;
    l.sections = scope == HNB_SORT_SCOPE_PROGRAM ? 1u : n_inst;
    l.rows = (uint32_t)rows;
    l.pitch = (l.rows + 63u) & ~63u;
    l.tiles = (uint32_t)((rows + kExportSortTile - 1u) / kExportSortTile);       // (in 64 bits: the last 4095 row counts would wrap)
    l.groups = (l.tiles + kExportSortGroup - 1u) / kExportSortGroup;
    l.vals_off = (uint64_t)l.sections * l.pitch * 8u;
    l.state_off = l.vals_off * 2u;
    l.gsum_off = l.state_off + (((uint64_t)l.sections * sizeof(ExportSortState) + 255u) & ~(uint64_t)255u);
    l.hist_off = l.gsum_off + (uint64_t)l.sections * 2u * kExportSortPasses * l.groups * 1024u;
    l.zero_bytes = l.hist_off - l.state_off;
    l.total = l.hist_off + (uint64_t)l.sections * kExportSortPasses * l.tiles * 1024u;
    return l;
}


// ---- filtered, then sorted (hnb_effect_export_filtered_sorted; kernels: hnb_export_cull.hip, a fourth code object, and those of units 2 and 3) ----
// The filter's compaction feeds the sort: k_export_cull_keys takes its rows from the filter's order[] and their count from its state word, the sort's
// later kernels and the kRowsOrdered gather take the same count as the alive_count of a 32-byte row with HnbDeviceMeta's layout that lies where the
// filter's state word does (f.state == (uint32_t*)s.meta; its other words are zeroed with the allocation and never written). Effects of one tile:
// k_export_cull_tile does all of it in one workgroup.
struct ExportCullArgs {
    ExportFilterArgs f;             // as the filtered export binds it (meta: the effect's row), in the call's own scratch
    ExportSortArgs s;               // as the sorted export binds it, except meta: the row that holds the kept count
};

// The scratch of an effect's filtered-then-sorted exports, one allocation: export_filter_scratch_layout, then (at sort_off, a 256-byte boundary)
// export_sort_scratch_layout of one instance. 20 bytes per slot of capacity and, above 4096 slots, about 5.6 more for the digit tables and the mask.
// sort.rows == 0: more than 0xFFFFFF00 slots, refused as the sorted export refuses them.
struct ExportCullScratch { ExportFilterScratch filter; ExportSortScratch sort; uint64_t sort_off, total; };
HNB_SORT_KEY_FN ExportCullScratch export_cull_scratch_layout(uint32_t capacity) {
    ExportCullScratch l;
    l.filter = export_filter_scratch_layout(capacity);
    l.sort = export_sort_scratch_layout(1u, capacity, HNB_SORT_SCOPE_INSTANCE);
    l.sort_off = (l.filter.total + 255u) & ~(uint64_t)255u;
    l.total = l.sort_off + l.sort.total;
    return l;
}


// ---- filtered export, program form (hnb_program_export_filtered; kernels: hnb_export_filter_prog.hip, a fifth code object, and k_export_offsets) ----
// The filtered export's compaction once per instance, the instance being blockIdx.y: every scratch section of the effect form exists per instance,
// and the state word of instance k is word 0 of kept[k], a 32-byte row with HnbDeviceMeta's layout whose other words are zeroed with the allocation
// and never written. k_export_offsets, bound to those rows, scans the kept counts; the kRowsFilteredInstance gather takes count and first record
// from the same rows and from offsets[]. No workgroup waits for another.
struct ExportFilterRow {            // what of an HnbExportFilter may differ between the instances of one call: a device row per instance
    float P[HNB_FILTER_MAX_PLANES][4];
    uint32_t n_planes, invert, lo_bits, hi_bits;
    uint32_t pad[4];
};
static_assert(sizeof(ExportFilterRow) == 128, "a filter row is 128 bytes");

struct ExportFilterProgArgs {
    ExportFilterArgs f;             // slab, meta: the program's tables [n_inst]; order, mask, tile_count, tile_offset: instance 0's section, instance k's lies k
                                    //   sections behind it; state: kept[0]; n_planes, invert, lo_bits, hi_bits, P: the one filter of a call that shares it
    const ExportFilterRow* filters; // [n_inst] a filter per instance; NULL: every instance takes f's
    uint32_t n_inst;
    uint32_t order_pitch;           // slots between two instances' sections of order[]
};

// The scratch of a program's filtered exports, one allocation; every section starts on a 256-byte boundary. Per instance: 4 bytes per slot of
// capacity (order), per tile of 4096 slots 512 bytes of mask and two words, a 32-byte kept row and a 128-byte filter row.
struct ExportFilterProgScratch {
    uint32_t n_inst, tiles, pitch;  // tiles of ONE instance; pitch: slots of one instance's section of order[]
    uint64_t order_off, order_bytes, mask_off, mask_bytes, count_off, count_bytes, offset_off, offset_bytes, kept_off, kept_bytes, filter_off, filter_bytes, total;
};
HNB_SORT_KEY_FN ExportFilterProgScratch export_filter_prog_scratch_layout(uint32_t n_inst, uint32_t capacity) {
    ExportFilterProgScratch l;
    const uint64_t n = n_inst, align = 255u;
    l.n_inst = n_inst;
    l.tiles = (uint32_t)(((uint64_t)capacity + kExportFilterTile - 1u) / kExportFilterTile);
    l.pitch = capacity;
    l.order_off = 0;
    l.order_bytes = n * l.pitch * 4u;
    l.mask_off = (l.order_off + l.order_bytes + align) & ~align;
    l.mask_bytes = n * l.tiles * kExportFilterTileWords * 8u;
    l.count_off = (l.mask_off + l.mask_bytes + align) & ~align;
    l.count_bytes = n * l.tiles * 4u;
    l.offset_off = (l.count_off + l.count_bytes + align) & ~align;
    l.offset_bytes = n * l.tiles * 4u;
    l.kept_off = (l.offset_off + l.offset_bytes + align) & ~align;
    l.kept_bytes = n * sizeof(HnbDeviceMeta);
    l.filter_off = (l.kept_off + l.kept_bytes + align) & ~align;
    l.filter_bytes = n * sizeof(ExportFilterRow);
    l.total = (l.filter_off + l.filter_bytes + align) & ~align;
    return l;
}


// ---- filtered, then sorted, program form (hnb_program_export_sorted with an HnbExportSortFiltered; kernels: hnb_export_cull_prog.hip, a sixth code
// object of the exports, and those of units 1, 2 and 5) ----
// The filtered program export's compaction feeds the sorted program export's instance scope, as the effect form's feeds an effect's sort: the sort
// and the gather take instance k's row count from kept[k], the rows k_export_offsets scans. Instances of one tile: k_export_cull_tile_inst does
// everything in front of that scan in one workgroup per instance.
static_assert(sizeof(HnbExportSortFiltered) == 48, "HnbExportSortFiltered layout");

struct ExportCullProgArgs {
    ExportFilterProgArgs p;         // as the filtered program export binds it (f.meta: the program's rows), in this form's own scratch
    ExportSortArgs s;               // as the sorted program export binds its instance scope, except meta: the kept rows (p.f.state)
};

// The scratch of a program's filtered-then-sorted exports, one allocation: export_filter_prog_scratch_layout, then (at sort_off, a 256-byte
// boundary) export_sort_scratch_layout of the instance scope. sort.rows == 0: more than 0xFFFFFF00 slots, refused as the sorted export refuses them.
struct ExportCullProgScratch { ExportFilterProgScratch filter; ExportSortScratch sort; uint64_t sort_off, total; };
HNB_SORT_KEY_FN ExportCullProgScratch export_cull_prog_scratch_layout(uint32_t n_inst, uint32_t capacity) {
    ExportCullProgScratch l;
    l.filter = export_filter_prog_scratch_layout(n_inst, capacity);
    l.sort = export_sort_scratch_layout(n_inst, capacity, HNB_SORT_SCOPE_INSTANCE);
    l.sort_off = (l.filter.total + 255u) & ~(uint64_t)255u;
    l.total = l.sort_off + l.sort.total;
    return l;
}


// ---- the host path of every form: which kernels there are, and which of them a call launches ----
// The kernels of the code objects, in the order of their units: the index of a kernel's handle in the context. kExpKernelCount sizes the handle
// array, kExportUnitCount the module array. A later unit is numbered behind the earlier ones, whose values stay.
enum ExportUnit : uint32_t { kUnitExport, kUnitExportSort, kUnitExportFilter, kUnitExportCull, kUnitExportFilterProg, kUnitExportCullProg, kExportUnitCount };
enum ExportKernel : uint32_t {
    kExpRows0, kExpRows1, kExpRows2, kExpRows3, kExpOffsets,                                                    // hnb_export.hip
    kExpSortRows0, kExpSortRows1, kExpSortRows2, kExpSortRows3, kExpSortTile, kExpSortKeys, kExpSortHist, kExpSortScatter,   // hnb_export_sort.hip: one effect,
    kExpSortRowsInst0, kExpSortRowsInst1, kExpSortRowsInst2, kExpSortRowsInst3, kExpSortTileInst, kExpSortKeysInst, kExpSortHistInst, kExpSortScatterInst,   // (tiles, instances),
    kExpSortRowsAll0, kExpSortRowsAll1, kExpSortRowsAll2, kExpSortRowsAll3, kExpSortFill, kExpSortHistAll, kExpSortScatterAll,   // all instances' rows as one space
    kExpFilterRows0, kExpFilterRows1, kExpFilterRows2, kExpFilterRows3, kExpFilterTile, kExpFilterMark, kExpFilterScan, kExpFilterCompact,   // hnb_export_filter.hip
    kExpCullTile, kExpCullKeys,                                                                                 // hnb_export_cull.hip
    kExpFilterRowsInst0, kExpFilterRowsInst1, kExpFilterRowsInst2, kExpFilterRowsInst3,                         // hnb_export_filter_prog.hip: (tiles, instances)
    kExpFilterTileInst, kExpFilterMarkInst, kExpFilterScanInst, kExpFilterCompactInst,
    kExpCullTileInst, kExpCullKeysInst,                                                                         // hnb_export_cull_prog.hip: (tiles, instances)
    kExpKernelCount
};

enum ExportForm : uint32_t { kExportPlain, kExportSorted, kExportFiltered, kExportFilteredSorted };
// What a launch passes: an argument block by value (the sort's hist and scatter kernels take the pass behind it), or k_export_offsets' five words
enum ExportArgBlock : uint32_t { kExportArgsRows, kExportArgsSort, kExportArgsSortPass, kExportArgsFilter, kExportArgsOffsets, kExportArgsCull, kExportArgsFilterProg, kExportArgsCullProg };
struct ExportLaunch { uint32_t kernel, grid_x, grid_y, args, pass; };   // (workgroups of kExportBlock lanes)
constexpr uint32_t kExportPlanMax = 13, kExportNoMemset = ~0u;
struct ExportPlan {
    uint32_t n;                         // launches, in stream order
    uint32_t memset_before;             // a multi-tile sort: bytes [zero_off, zero_off + zero_bytes) of the call's scratch are zeroed in front of launch
    uint64_t zero_off, zero_bytes;      //   `memset_before` (the sort's state words and group sums); kExportNoMemset: nothing is
    ExportLaunch launch[kExportPlanMax];
};

// The gather of a form, by the LDS image of its records (export_variant)
HNB_SORT_KEY_FN uint32_t export_rows_kernel(uint32_t form, bool program, uint32_t scope, uint32_t variant) {
    const uint32_t first = form == kExportFiltered ? (program ? kExpFilterRowsInst0 : kExpFilterRows0) : form == kExportPlain ? kExpRows0 : !program ? kExpSortRows0 :
                           form == kExportSorted && scope == HNB_SORT_SCOPE_PROGRAM ? kExpSortRowsAll0 : kExpSortRowsInst0;
    return first + variant;
}

// The launches of one export, in order. `program`: all n_inst instances of a program (plain or sorted in `scope`), else one effect (n_inst and scope
// are not read). A sorted form's rows must fit (export_sort_scratch_layout(...).rows != 0). kExportFilteredSorted of a program: instance scope. The
// filtered program forms scan KEPT counts, so their k_export_offsets runs behind the instances' compaction counts, not in front. Decides;
// hanabi_amd.hip run_export_plan executes.
HNB_SORT_KEY_FN ExportPlan export_launch_plan(uint32_t form, bool program, uint32_t scope, uint32_t n_inst, uint32_t capacity, uint32_t stride_bytes) {
    ExportPlan pl = {};
    pl.memset_before = kExportNoMemset;
    const uint32_t n = program ? n_inst : 1u;
    const bool all = program && form == kExportSorted && scope == HNB_SORT_SCOPE_PROGRAM;
    const uint32_t tiles = (uint32_t)(((uint64_t)capacity + kExportSortTile - 1u) / kExportSortTile);   // of one instance (the filter's tiles are the sort's)
    const uint32_t rows = all ? n * capacity : capacity, gy = all ? 1u : n;        // of the gather's row space, and how many of them
    const uint32_t variant = export_variant(stride_bytes), tile_rows = export_tile_rows(variant);
    const auto add = [&pl](uint32_t kernel, uint32_t gx, uint32_t gy, uint32_t args, uint32_t pass = 0u) { pl.launch[pl.n++] = ExportLaunch{kernel, gx, gy, args, pass}; };
    if (program && (form == kExportPlain || form == kExportSorted)) add(kExpOffsets, 1u, 1u, kExportArgsOffsets);   // over the alive counts
    if (form == kExportSorted) {
        const ExportSortScratch l = export_sort_scratch_layout(n, capacity, all ? HNB_SORT_SCOPE_PROGRAM : HNB_SORT_SCOPE_INSTANCE);
        const uint32_t tile = program ? kExpSortTileInst : kExpSortTile, keys = all ? kExpSortFill : program ? kExpSortKeysInst : kExpSortKeys;
        const uint32_t hist = all ? kExpSortHistAll : program ? kExpSortHistInst : kExpSortHist, scatter = all ? kExpSortScatterAll : program ? kExpSortScatterInst : kExpSortScatter;
        if (!all && l.tiles <= 1u) add(tile, 1u, n, kExportArgsSort);              // every instance's whole sort by one workgroup
        else {
            pl.memset_before = pl.n; pl.zero_off = l.state_off; pl.zero_bytes = l.zero_bytes;
            add(keys, tiles, n, kExportArgsSort);                                  // (the keys kernels count pass 0's digits; k_export_sort_fill does not)
            for (uint32_t pass = 0; pass < kExportSortPasses; ++pass) {
                if (pass || all) add(hist, l.tiles, gy, kExportArgsSortPass, pass);
                add(scatter, l.tiles, gy, kExportArgsSortPass, pass);
            }
        }
    } else if (form == kExportFiltered && program) {
        if (tiles <= 1u) add(kExpFilterTileInst, 1u, n, kExportArgsFilterProg);    // every instance's mark, count and compact by one workgroup
        else {
            add(kExpFilterMarkInst, tiles, n, kExportArgsFilterProg);
            add(kExpFilterScanInst, 1u, n, kExportArgsFilterProg);
        }
        add(kExpOffsets, 1u, 1u, kExportArgsOffsets);                              // over the kept counts
        if (tiles > 1u) add(kExpFilterCompactInst, tiles, n, kExportArgsFilterProg);
    } else if (form == kExportFiltered) {
        if (tiles <= 1u) add(kExpFilterTile, 1u, 1u, kExportArgsFilter);           // mark, count and compact by one workgroup
        else {
            add(kExpFilterMark, tiles, 1u, kExportArgsFilter);
            add(kExpFilterScan, 1u, 1u, kExportArgsFilter);
            add(kExpFilterCompact, tiles, 1u, kExportArgsFilter);
        }
    } else if (form == kExportFilteredSorted) {                                    // the program form: the effect form's launches per instance, and the scan of the kept counts
        const uint32_t filter_args = program ? kExportArgsFilterProg : kExportArgsFilter, cull_args = program ? kExportArgsCullProg : kExportArgsCull;
        const uint32_t mark = program ? kExpFilterMarkInst : kExpFilterMark, scan = program ? kExpFilterScanInst : kExpFilterScan, compact = program ? kExpFilterCompactInst : kExpFilterCompact;
        const uint32_t tile = program ? kExpCullTileInst : kExpCullTile, keys = program ? kExpCullKeysInst : kExpCullKeys;
        const uint32_t hist = program ? kExpSortHistInst : kExpSortHist, scatter = program ? kExpSortScatterInst : kExpSortScatter;
        if (tiles <= 1u) {
            add(tile, 1u, n, cull_args);                                           // mark, compact into (key, slot) pairs and every pass by one workgroup
            if (program) add(kExpOffsets, 1u, 1u, kExportArgsOffsets);             // over the kept counts
        } else {
            add(mark, tiles, n, filter_args);
            add(scan, 1u, n, filter_args);
            if (program) add(kExpOffsets, 1u, 1u, kExportArgsOffsets);             // where the filtered program export has it: only the gather needs it
            add(compact, tiles, n, filter_args);
            const ExportSortScratch l = export_sort_scratch_layout(n, capacity, HNB_SORT_SCOPE_INSTANCE);   // (the sort section of either form's scratch)
            const uint64_t sort_off = program ? export_cull_prog_scratch_layout(n, capacity).sort_off : export_cull_scratch_layout(capacity).sort_off;
            pl.memset_before = pl.n; pl.zero_off = sort_off + l.state_off; pl.zero_bytes = l.zero_bytes;
            add(keys, tiles, n, cull_args);                                        // the kept rows' keys, and pass 0's digit counts
            for (uint32_t pass = 0; pass < kExportSortPasses; ++pass) {
                if (pass) add(hist, tiles, n, kExportArgsSortPass, pass);
                add(scatter, tiles, n, kExportArgsSortPass, pass);
            }
        }
    }
    add(export_rows_kernel(form, program, scope, variant), (rows + tile_rows - 1u) / tile_rows, gy, kExportArgsRows);
    return pl;
}

}  // namespace hnb
