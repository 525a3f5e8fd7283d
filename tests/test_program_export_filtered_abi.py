"""The filtered program export (hnb_program_export_filtered, include/hanabi_amd.h "Packed output") without a GPU: header, ctypes mirror and
INTEGRATION.md agree on the prototype and the call fails loudly; its kernels live in a fifth code object with no scratch and no spills, the gathers
with the LDS of the effect form's; the launch plan of the new form is the design's table, with nothing of the earlier forms renumbered; the scratch
layout's sections are ordered, aligned, disjoint and inside the allocation, and for one instance they are the effect form's."""
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
from test_export_filtered_abi import CSRC, _rows, _standalone
from test_export_sorted_abi import A, LLVM, ROOT

# k_export_offsets, the call's ninth kernel, is the first code object's, unchanged: it is not in this one
PROG_KERNELS = (["k_export_filter_mark_inst", "k_export_filter_scan_inst", "k_export_filter_compact_inst", "k_export_filter_tile_inst"]
                + [f"k_export_filter_rows_inst_{v}" for v in (32, 64, 128, 256)])


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_integration_agree_on_the_prototype(tmp_path):
    src = r'''
    #include "hanabi_amd.h"
    int main(void) {
        int (*f)(HnbProgram*, const HnbExportDesc*, const HnbExportFilter*, uint32_t, uint32_t*) = hnb_program_export_filtered;
        return f == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    subprocess.check_call([str(tmp_path / "t")])
    assert "hnb_program_export_filtered" in runtime.ABI_SYMBOLS
    lib = runtime.load_library()
    assert hasattr(lib, "hnb_program_export_filtered")
    assert lib.hnb_program_export_filtered.argtypes == [C.c_void_p, C.POINTER(runtime.ExportDesc), C.POINTER(runtime.ExportFilter), C.c_uint32, C.c_void_p]
    assert callable(runtime.Program.export_filtered)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    m = re.search(r"int\s+hnb_program_export_filtered\s*\(([^)]*)\)\s*;", header)
    assert m, "the header declares the call"
    c_args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert c_args == ["HnbProgram* prog", "const HnbExportDesc* desc", "const HnbExportFilter* filters", "uint32_t n_filters", "uint32_t* out_offsets"]
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"pub fn hnb_program_export_filtered\(([^)]*)\) -> c_int;", txt)
    assert m, "INTEGRATION.md binds the call"
    assert [a.strip() for a in m.group(1).split(",")] == ["prog: *mut HnbProgram", "desc: *const HnbExportDesc", "filters: *const HnbExportFilter", "n_filters: u32",
                                                          "out_offsets: *mut u32"]
    assert "hnb_program_export_filtered(prog, &desc, filters, n_filters, out_offsets)" in txt      # ... and has a paragraph on it


def test_call_fails_loudly_on_null_arguments_and_without_a_device():
    lib = runtime.load_library()
    d = runtime.export_desc([(A.POSITION.id, 0)], 0x1000, 16, 1)
    f = runtime.export_filter("sphere", sphere=(0, 0, 0, 1))
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for args in ((None, C.byref(d), C.byref(f)), (fake, None, C.byref(f)), (fake, C.byref(d), None), (None, None, None)):
        for n in (0, 1, 2):
            assert lib.hnb_program_export_filtered(*args, n, None) == -1 and b"NULL" in lib.hnb_last_error()
    # (n_filters and mixed kinds are checked against the program's instances: tests/test_gpu_program_export_filtered.py)
    if not torch.cuda.is_available():   # no device: there is no program to export from, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code object ----------------------------------------------------------------------------------------------------------------------------
def test_fifth_code_object_is_built_carried_and_has_its_kernels_without_scratch_or_spills():
    co = hb.export_filter_prog_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_export_filter_prog.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(PROG_KERNELS), sorted(rows)
    for name, r in rows.items():
        assert 0 < r["group_segment_fixed_size"] <= 32 * 1024, f"{name}: {r['group_segment_fixed_size']} B of LDS per workgroup"
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
    effect_rows, first_rows = _rows(hb.export_filter_code_path()), _rows(hb.export_code_path())
    for v in (32, 64, 128, 256):         # the shared gather body: the same LDS image, the same argument block
        assert rows[f"k_export_filter_rows_inst_{v}"]["group_segment_fixed_size"] == effect_rows[f"k_export_filter_rows_{v}"]["group_segment_fixed_size"]
        assert rows[f"k_export_filter_rows_inst_{v}"]["kernarg_segment_size"] == first_rows[f"k_export_rows_{v}"]["kernarg_segment_size"]      # ExportArgs did not grow
    for k in ("mark", "scan", "compact", "tile"):      # the effect form's bodies: the same LDS; their block is an ExportFilterArgs and the instance words
        assert rows[f"k_export_filter_{k}_inst"]["group_segment_fixed_size"] == effect_rows[f"k_export_filter_{k}"]["group_segment_fixed_size"], k
        assert rows[f"k_export_filter_{k}_inst"]["kernarg_segment_size"] == effect_rows[f"k_export_filter_{k}"]["kernarg_segment_size"] + 16, k
    assert "k_export_offsets" in first_rows
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    for other in (hb.export_code_path(), hb.export_sort_code_path(), hb.export_filter_code_path(), hb.export_cull_code_path()):
        assert open(other, "rb").read() in lib                           # five embedded code objects
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_export_filter_prog_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_export_filter_prog.hip")).read()
    assert hb.build_export_filter_prog_code in hb.EXPORT_CODE_OBJECTS and len(hb.EXPORT_CODE_OBJECTS) == 6


# ---- the launch plan (csrc/hnb_export.h), as a stand-alone host program ---------------------------------------------------------------------------
def prog_plan_table(n, cap, stride):
    """The launches of the new form as the design states them"""
    T = -(-cap // 4096)
    v = {32: 0, 64: 1, 128: 2, 256: 3}[stride]
    G = -(-cap // (128 if v == 3 else 256))
    if T <= 1:
        return [("kExpFilterTileInst", 1, n, "filter+inst", 0), ("kExpOffsets", 1, 1, "offsets", 0), (f"kExpFilterRowsInst{v}", G, n, "rows", 0)]
    return [("kExpFilterMarkInst", T, n, "filter+inst", 0), ("kExpFilterScanInst", 1, n, "filter+inst", 0), ("kExpOffsets", 1, 1, "offsets", 0),
            ("kExpFilterCompactInst", T, n, "filter+inst", 0), (f"kExpFilterRowsInst{v}", G, n, "rows", 0)]


def test_launch_plan_of_the_new_form_is_the_designs_table_and_nothing_was_renumbered(tmp_path):
    names = ["kExpOffsets", "kExpFilterTileInst", "kExpFilterMarkInst", "kExpFilterScanInst", "kExpFilterCompactInst"] + [f"kExpFilterRowsInst{v}" for v in range(4)]
    exe = _standalone(tmp_path, "ppl", r"""
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
        // what the two existing plan tests pin
        static_assert(kExpCullTile == 36 && kExpCullKeys == 37 && kExpFilterRowsInst0 == 38, "the fourth unit's are numbered behind the 36 kernels of the first three");
        static_assert(kUnitExportCull == 3, "the fourth unit");
        static_assert(kExportPlain == 0 && kExportSorted == 1 && kExportFiltered == 2 && kExportFilteredSorted == 3, "forms");
        static_assert(kExportArgsRows == 0 && kExportArgsSort == 1 && kExportArgsSortPass == 2 && kExportArgsFilter == 3 && kExportArgsOffsets == 4 && kExportArgsCull == 5, "args[]");
        static_assert(sizeof(ExportCullArgs) == sizeof(ExportFilterArgs) + sizeof(ExportSortArgs), "one filter block and one sort block");
        // the fifth unit, behind them, and the sixth behind it
        static_assert(kUnitExportFilterProg == 4 && kUnitExportCullProg == 5 && kExportUnitCount == 6, "six units");
        static_assert(kExpFilterRowsInst0 == 38 && kExpFilterRowsInst1 == 39 && kExpFilterRowsInst2 == 40 && kExpFilterRowsInst3 == 41 && kExpFilterTileInst == 42 &&
                      kExpFilterMarkInst == 43 && kExpFilterScanInst == 44 && kExpFilterCompactInst == 45, "the fifth unit's kernels are numbered behind the fourth's");
        static_assert(kExpCullTileInst == 46 && kExpCullKeysInst == 47 && kExpKernelCount == 48, "the sixth unit's kernels are numbered behind the fifth's");
        static_assert(kExportArgsFilterProg == 6, "args[]");
        static_assert(sizeof(ExportFilterProgArgs) == sizeof(ExportFilterArgs) + 16 && sizeof(ExportFilterRow) == 128, "an ExportFilterArgs and the instance words");
        static const char* const args[] = {"rows", "sort", "sort+pass", "filter", "offsets", "cull", "filter+inst"};
        unsigned n, cap, stride;
        while (std::scanf("%u %u %u", &n, &cap, &stride) == 3) {
            const ExportPlan pl = export_launch_plan(kExportFiltered, true, HNB_SORT_SCOPE_INSTANCE, n, cap, stride);
            if (pl.n > kExportPlanMax) return 2;
            std::printf("%u %d", pl.n, pl.memset_before == kExportNoMemset ? -1 : (int)pl.memset_before);
            for (uint32_t i = 0; i < pl.n; ++i) std::printf(" %s %u %u %s %u", kernel_name(pl.launch[i].kernel), pl.launch[i].grid_x, pl.launch[i].grid_y, args[pl.launch[i].args], pl.launch[i].pass);
            std::printf("\n");
        }
        return 0;
    }
    """)
    cases = [(n, cap, stride) for cap in (300, 4096, 4097, 10_000) for n in (1, 5) for stride in (32, 256)]
    out = subprocess.run([exe], input="\n".join("%d %d %d" % c for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (n, cap, stride), line in zip(cases, out):
        w = line.split()
        count, memset = int(w[0]), int(w[1])
        got = [(w[i], int(w[i + 1]), int(w[i + 2]), w[i + 3], int(w[i + 4])) for i in range(2, len(w), 5)]
        assert count == len(got) and got == prog_plan_table(n, cap, stride), (n, cap, stride, got)
        assert count == (3 if cap <= 4096 else 5) and memset == -1, (n, cap, stride, count, memset)      # whatever the instance count; nothing is zeroed per call


# ---- the scratch layout ---------------------------------------------------------------------------------------------------------------------------
def test_scratch_layout_sections_are_ordered_aligned_disjoint_and_inside(tmp_path):
    exe = _standalone(tmp_path, "pfl", r"""
    #include <cstdio>
    #include <cstdint>
    #include "hnb_export.h"
    int main() {
        unsigned long long n, cap;
        while (std::scanf("%llu %llu", &n, &cap) == 2) {
            const hnb::ExportFilterProgScratch l = hnb::export_filter_prog_scratch_layout((uint32_t)n, (uint32_t)cap);
            const hnb::ExportFilterScratch e = hnb::export_filter_scratch_layout((uint32_t)cap);
            std::printf("%u %u %u", l.n_inst, l.tiles, l.pitch);
            const unsigned long long v[] = {l.order_off, l.order_bytes, l.mask_off, l.mask_bytes, l.count_off, l.count_bytes, l.offset_off, l.offset_bytes, l.kept_off, l.kept_bytes,
                                            l.filter_off, l.filter_bytes, l.total, e.order_bytes, e.mask_bytes, e.count_bytes, e.offset_bytes};
            for (unsigned long long x : v) std::printf(" %llu", x);
            std::printf("\n");
        }
        return 0;
    }
    """)
    caps = [1, 63, 64, 4096, 4097, 131_073, 16_777_216, (1 << 32) - 1]
    cases = [(n, cap) for n in (1, 5, 65535) for cap in caps]
    out = subprocess.run([exe], input="\n".join("%d %d" % c for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (n, cap), line in zip(cases, out):
        n_inst, tiles, pitch, *rest = [int(x) for x in line.split()]
        total, e_order, e_mask, e_count, e_offset = rest[12:]
        sections = list(zip(rest[0:12:2], rest[1:12:2]))                 # (offset, bytes): order, masks, tile counts, tile offsets, kept rows, filter table
        assert (n_inst, tiles) == (n, -(-cap // 4096)) and pitch >= cap, (n, cap, line)
        want = [4 * n * pitch, 512 * n * tiles, 4 * n * tiles, 4 * n * tiles, 32 * n, 128 * n]          # in 64 bits: 65535 instances of 2^32 - 1 slots are 2^50 bytes of order[]
        assert [size for _, size in sections] == want, (n, cap, sections, want)
        end = 0
        for off, size in sections:                                       # in this order, none starting before the one in front of it ends
            assert off >= end and off % 256 == 0 and size > 0, (n, cap, sections)
            end = off + size
        assert end <= total and total - end < 256, (n, cap, sections, total)
        assert total <= n * (4 * pitch + 520 * tiles + 160) + 7 * 256
        if n == 1:                                                       # one instance: the effect form's sections
            assert (sections[0][1], sections[1][1], sections[2][1], sections[3][1]) == (e_order, e_mask, e_count, e_offset), (cap, sections)
