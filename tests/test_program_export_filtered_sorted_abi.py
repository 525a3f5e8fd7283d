"""The filtered, then sorted program export (an HnbExportSortFiltered through hnb_program_export_sorted, include/hanabi_amd.h "Packed output")
without a GPU: the 48-byte descriptor in C99 and in ctypes, no new entry point; its two kernels in a code object of their own with no scratch and
no spills, next to six older ones whose kernels are what they were; the form's launch plan and scratch layout (hnb_export.h) from a stand-alone
host program under the address and undefined-behaviour sanitizers, held against the design's table; NULL arguments fail loudly."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import runtime
from test_export_filtered_abi import CSRC, _rows, _standalone, sort_layout
from test_export_sorted_abi import A, LLVM, ROOT

NEW_KERNELS = ["k_export_cull_keys_inst", "k_export_cull_tile_inst"]
V = (32, 64, 128, 256)
OLDER = {       # the six older code objects and their kernels
    "export": [f"k_export_rows_{v}" for v in V] + ["k_export_offsets"],
    "export_sort": [f"k_export_sort_rows{s}_{v}" for s in ("", "_inst", "_all") for v in V]
                   + [f"k_export_sort_{k}{s}" for k in ("tile", "keys", "hist", "scatter") for s in ("", "_inst")] + ["k_export_sort_fill", "k_export_sort_hist_all", "k_export_sort_scatter_all"],
    "export_filter": [f"k_export_filter_rows_{v}" for v in V] + [f"k_export_filter_{k}" for k in ("tile", "mark", "scan", "compact")],
    "export_cull": ["k_export_cull_tile", "k_export_cull_keys"],
    "export_filter_prog": [f"k_export_filter_rows_inst_{v}" for v in V] + [f"k_export_filter_{k}_inst" for k in ("tile", "mark", "scan", "compact")],
    "bounds": ["k_bounds_tile", "k_bounds_finish", "k_bounds_union", "k_bounds_small"],
}


# ---- the descriptor -------------------------------------------------------------------------------------------------------------------------------
def test_descriptor_has_the_headers_size_and_offsets_in_c99_and_ctypes(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd.h"
    int main(void) {
        HnbExportSortFiltered sf = {{0}};
        const HnbExportSort* as_sort = (const HnbExportSort*)&sf;     /* how a caller passes it */
        sf.sort.struct_size = (uint32_t)sizeof sf;
        printf("%zu %zu %zu %zu %zu %u %zu\n", sizeof(HnbExportSortFiltered), offsetof(HnbExportSortFiltered, sort), offsetof(HnbExportSortFiltered, filters),
               offsetof(HnbExportSortFiltered, n_filters), offsetof(HnbExportSortFiltered, reserved2), as_sort->struct_size, sizeof(HnbExportSort));
        return 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    assert got == [48, 0, 32, 40, 44, 48, 32]
    S = runtime.ExportSortFiltered
    assert [C.sizeof(S), S.sort.offset, S.filters.offset, S.n_filters.offset, S.reserved2.offset] == got[:5]
    assert C.sizeof(runtime.ExportSort) == 32 and C.sizeof(runtime.ExportFilter) == 128      # the classes the descriptor is made of keep their sizes
    sf, arr = runtime.export_sort_filtered(dict(key="depth", v=(1, 2, 3), descending=True), [dict(kind="sphere", sphere=(0, 0, 0, 1))] * 3)
    assert (sf.sort.struct_size, sf.sort.key, sf.sort.descending, list(sf.sort.v), sf.n_filters, sf.reserved2) == (48, 0, 1, [1.0, 2.0, 3.0], 3, 0)
    assert sf.filters == C.addressof(arr) and len(arr) == 3 and arr[2].struct_size == 128
    assert callable(runtime.Program.export_filtered_sorted)
    assert list(inspect.signature(runtime.Program.export_filtered_sorted).parameters) == ["self", "fields", "dst_ptr", "stride", "capacity_records", "count_ptr", "offsets_ptr", "filter",
                                                                                          "sort"]


def test_header_declares_61_functions_and_integration_mirrors_the_struct():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header))
    assert len(declared) == 61 and declared == set(runtime.ABI_SYMBOLS)  # the feature is a descriptor, not an entry point
    assert "typedef struct HnbExportSortFiltered" in header
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert declared <= set(re.findall(r"pub fn (hnb_[a-z0-9_]+)\(", txt)) and "pub fn hnb_program_export_filtered_sorted" not in txt
    m = re.search(r"#\[repr\(C\)\]\s*pub struct HnbExportSortFiltered \{(.*?)\}", txt, flags=re.S)
    assert m, "INTEGRATION.md mirrors the struct"
    members = [" ".join(line.split("//")[0].split()).rstrip(",") for line in m.group(1).splitlines() if line.split("//")[0].strip()]
    assert members == ["pub sort: HnbExportSort", "pub filters: *const HnbExportFilter", "pub n_filters: u32", "pub reserved2: u32"]


def test_calls_fail_loudly_on_null_arguments_and_without_a_device():
    lib = runtime.load_library()
    d = runtime.export_desc([(A.POSITION.id, 0)], 0x1000, 16, 1)
    sf, arr = runtime.export_sort_filtered(dict(key="depth", v=(0, 0, 1)), [dict(kind="sphere", sphere=(0, 0, 0, 1))])
    s = C.cast(C.byref(sf), C.POINTER(runtime.ExportSort))
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for args in ((None, C.byref(d), s), (fake, None, s), (fake, C.byref(d), None), (None, None, None)):
        for scope in (0, 1):
            assert lib.hnb_program_export_sorted(*args, scope, None) == -1 and b"NULL" in lib.hnb_last_error()
        assert lib.hnb_effect_export_sorted(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no program to export from, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code objects -----------------------------------------------------------------------------------------------------------------------------
def test_seventh_code_object_is_gfx950_embedded_and_holds_two_kernels_without_scratch_or_spills():
    co = hb.export_cull_prog_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_export_cull_prog.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(NEW_KERNELS), sorted(rows)
    for name, r in rows.items():
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert 0 < r["group_segment_fixed_size"] <= 8 * 1024, f"{name}: {r['group_segment_fixed_size']} B of LDS per workgroup"
    assert rows["k_export_cull_keys_inst"]["vgpr_count"] <= 64           # eight waves per SIMD stay possible
    effect = _rows(hb.export_cull_code_path())                           # the effect form's bodies: the same LDS
    assert rows["k_export_cull_keys_inst"]["group_segment_fixed_size"] == effect["k_export_cull_keys"]["group_segment_fixed_size"]
    assert rows["k_export_cull_tile_inst"]["group_segment_fixed_size"] == effect["k_export_cull_tile"]["group_segment_fixed_size"]
    assert rows["k_export_cull_tile_inst"]["kernarg_segment_size"] == rows["k_export_cull_keys_inst"]["kernarg_segment_size"] == effect["k_export_cull_keys"]["kernarg_segment_size"] + 16
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_export_cull_prog_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_export_cull_prog.hip")).read()
    assert hb.build_export_cull_prog_code in hb.EXPORT_CODE_OBJECTS and len(hb.EXPORT_CODE_OBJECTS) == 6
    assert any(hb.build_export_cull_prog_code in getattr(hb, t) for t in re.findall(r"\b([A-Z_]+_CODE_OBJECTS)\b", inspect.getsource(hb.build_runtime)))


def test_the_six_older_code_objects_are_embedded_with_their_kernel_sets_unchanged():
    lib = open(hb.runtime_lib_path(), "rb").read()
    for unit, kernels in OLDER.items():
        co = getattr(hb, unit + "_code_path")()
        assert open(co, "rb").read() in lib, unit
        assert sorted(_rows(co)) == sorted(kernels), (unit, sorted(_rows(co)))


# ---- plan and scratch layout (csrc/hnb_export.h), as a stand-alone host program under the sanitizers -----------------------------------------------
def filter_prog_layout(n, cap):
    """export_filter_prog_scratch_layout restated: (tiles, pitch, [(offset, bytes)] of order, mask, counts, offsets, kept rows, filter rows, total)"""
    up = lambda x: (x + 255) & ~255
    tiles = -(-cap // 4096)
    sizes = [4 * n * cap, 512 * n * tiles, 4 * n * tiles, 4 * n * tiles, 32 * n, 128 * n]
    sections, off = [], 0
    for size in sizes:
        sections.append((off, size))
        off = up(off + size)
    return tiles, cap, sections, off


def plan_table(n, cap, stride):
    """The launches of a call as the issue's table states them: (kernel, grid x, grid y, argument block, pass)"""
    T = -(-cap // 4096)
    v = {32: 0, 64: 1, 128: 2, 256: 3}[stride]
    gather = (f"kExpSortRowsInst{v}", -(-cap // (128 if v == 3 else 256)), n, "rows", 0)
    if T <= 1:
        return [("kExpCullTileInst", 1, n, "cull+inst", 0), ("kExpOffsets", 1, 1, "offsets", 0), gather]
    plan = [("kExpFilterMarkInst", T, n, "filter+inst", 0), ("kExpFilterScanInst", 1, n, "filter+inst", 0), ("kExpOffsets", 1, 1, "offsets", 0),
            ("kExpFilterCompactInst", T, n, "filter+inst", 0), ("kExpCullKeysInst", T, n, "cull+inst", 0), ("kExpSortScatterInst", T, n, "sort+pass", 0)]
    for p in (1, 2, 3):
        plan += [("kExpSortHistInst", T, n, "sort+pass", p), ("kExpSortScatterInst", T, n, "sort+pass", p)]
    return plan + [gather]


def test_plan_and_scratch_layout_under_the_sanitizers_are_the_designs_table(tmp_path):
    names = (["kExpOffsets", "kExpFilterMarkInst", "kExpFilterScanInst", "kExpFilterCompactInst", "kExpSortHistInst", "kExpSortScatterInst", "kExpCullTileInst", "kExpCullKeysInst"]
             + [f"kExpSortRowsInst{v}" for v in range(4)])
    exe = _standalone(tmp_path, "cpl", r"""
    #include <cstdio>
    #include <cstdint>
    #include "hnb_export.h"
    using namespace hnb;
    static const char* kernel_name(uint32_t k) {
        switch (k) {
    """ + "\n".join(f'        case {k}: return "{k}";' for k in names) + r"""
        }
        return "?";
    }
    int main() {
        static_assert(kExportPlanMax == 13 && kExportArgsCullProg == 7, "the longest plan and the last argument block are this form's");
        static_assert(sizeof(ExportCullProgArgs) == sizeof(ExportFilterProgArgs) + sizeof(ExportSortArgs) && sizeof(HnbExportSortFiltered) == 48, "one block of each");
        static const char* const args[] = {"rows", "sort", "sort+pass", "filter", "offsets", "cull", "filter+inst", "cull+inst"};
        for (uint32_t variant = 0; variant < kExportVariants; ++variant)         // the gather of the filtered and sorted forms: an effect's, a program's per instance
            for (uint32_t scope = HNB_SORT_SCOPE_INSTANCE; scope <= HNB_SORT_SCOPE_PROGRAM; ++scope) {
                if (export_rows_kernel(kExportFilteredSorted, false, scope, variant) != kExpSortRows0 + variant) return 4;
                if (export_rows_kernel(kExportFilteredSorted, true, HNB_SORT_SCOPE_INSTANCE, variant) != kExpSortRowsInst0 + variant) return 5;
            }
        unsigned long long n, cap, stride;
        while (std::scanf("%llu %llu %llu", &n, &cap, &stride) == 3) {
            const ExportCullProgScratch l = export_cull_prog_scratch_layout((uint32_t)n, (uint32_t)cap);
            const unsigned long long v[] = {l.filter.tiles, l.filter.pitch, l.filter.order_off, l.filter.order_bytes, l.filter.mask_off, l.filter.mask_bytes, l.filter.count_off,
                                            l.filter.count_bytes, l.filter.offset_off, l.filter.offset_bytes, l.filter.kept_off, l.filter.kept_bytes, l.filter.filter_off,
                                            l.filter.filter_bytes, l.filter.total, l.sort_off, l.total, l.sort.sections, l.sort.rows, l.sort.pitch, l.sort.tiles, l.sort.groups,
                                            l.sort.vals_off, l.sort.state_off, l.sort.gsum_off, l.sort.hist_off, l.sort.zero_bytes, l.sort.total};
            std::printf("L");
            for (unsigned long long x : v) std::printf(" %llu", x);
            std::printf("\n");
            if (l.sort.rows == 0) { std::printf("P refused\n"); continue; }      // more than 0xFFFFFF00 slots: no plan is asked for
            const ExportPlan pl = export_launch_plan(kExportFilteredSorted, true, HNB_SORT_SCOPE_INSTANCE, (uint32_t)n, (uint32_t)cap, (uint32_t)stride);
            if (pl.n > kExportPlanMax) return 2;
            std::printf("P %u %d %llu %llu", pl.n, pl.memset_before == kExportNoMemset ? -1 : (int)pl.memset_before, (unsigned long long)pl.zero_off, (unsigned long long)pl.zero_bytes);
            for (uint32_t i = 0; i < pl.n; ++i) {
                const ExportLaunch& ln = pl.launch[i];
                if (ln.kernel >= kExpKernelCount || ln.args > kExportArgsCullProg) return 3;
                std::printf(" %s %u %u %s %u", kernel_name(ln.kernel), ln.grid_x, ln.grid_y, args[ln.args], ln.pass);
            }
            std::printf("\n");
        }
        return 0;
    }
    """)
    cases = [(n, cap, stride) for cap in (1, 4096, 4097, 10_000, 0xFFFFFF00, 0xFFFFFF01) for n in (1, 5, 65_535) for stride in (32, 256)]
    out = subprocess.run([exe], input="\n".join("%d %d %d" % c for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 2 * len(cases)
    for (n, cap, stride), lay, plan in zip(cases, out[0::2], out[1::2]):
        what = (n, cap, stride)
        w = [int(x) for x in lay.split()[1:]]
        tiles, pitch, sections, ftotal = filter_prog_layout(n, cap)
        assert w[0:2] == [tiles, pitch] and list(zip(w[2:14:2], w[3:14:2])) == sections and w[14] == ftotal, what      # export_filter_prog_scratch_layout(n, cap) ...
        sort_off, total = w[15], w[16]
        assert sort_off == ftotal and sort_off % 256 == 0, what         # ... followed, at a 256-byte boundary, ...
        assert tuple(w[17:]) == sort_layout(n, cap, 0), what            # ... by export_sort_scratch_layout(n, cap, INSTANCE)
        assert total == sort_off + w[-1], what
        if cap > 0xFFFFFF00:
            assert w[18] == 0 and plan == "P refused", what             # rows == 0: the call is refused, as the sorted export refuses it
            continue
        p = plan.split()
        count, memset, zero_off, zero_bytes = int(p[1]), int(p[2]), int(p[3]), int(p[4])
        got = [(p[i], int(p[i + 1]), int(p[i + 2]), p[i + 3], int(p[i + 4])) for i in range(5, len(p), 5)]
        assert count == len(got) and got == plan_table(n, cap, stride), (what, got)
        if cap <= 4096:
            assert count == 3 and memset == -1, what
        else:                                                            # thirteen launches, and one memset of the sort's state words and group sums in front of the keys kernel
            assert count == 13 and memset == 4 and got[memset][0] == "kExpCullKeysInst", what
            state_off, hist_off = w[23], w[25]
            assert zero_off == sort_off + state_off and zero_bytes == hist_off - state_off and zero_off + zero_bytes <= total, what
        assert all(gx >= 1 and 1 <= gy <= 65_535 for _, gx, gy, _, _ in got), what
