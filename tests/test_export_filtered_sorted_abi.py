"""The filtered, then sorted export (hnb_effect_export_filtered_sorted, include/hanabi_amd.h "Packed output") without a GPU: the symbol is declared,
exported and bound and fails loudly on NULL arguments; its two kernels live in a fourth code object with no scratch and no spills; the third code
object is what it was before its helpers moved into a header; the launch plan of the new form is the design's table and the call's scratch layout
is the filter's followed by the sort's, every section aligned and inside the allocation."""
import ctypes as C
import json
import os
import subprocess

from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import runtime
from test_export_filtered_abi import FILTER_KERNELS, _rows, _standalone, sort_layout
from test_export_sorted_abi import A, LLVM, ROOT

CULL_KERNELS = ["k_export_cull_keys", "k_export_cull_tile"]


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_exported_and_bound(tmp_path):
    src = r'''
    #include "hanabi_amd.h"
    int main(void) {
        int (*f)(HnbEffect*, const HnbExportDesc*, const HnbExportFilter*, const HnbExportSort*) = hnb_effect_export_filtered_sorted;
        return f == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    subprocess.check_call([str(tmp_path / "t")])
    assert "hnb_effect_export_filtered_sorted" in runtime.ABI_SYMBOLS
    lib = runtime.load_library()
    assert hasattr(lib, "hnb_effect_export_filtered_sorted")
    assert lib.hnb_effect_export_filtered_sorted.argtypes == [C.c_void_p, C.POINTER(runtime.ExportDesc), C.POINTER(runtime.ExportFilter), C.POINTER(runtime.ExportSort)]
    assert callable(runtime.Effect.export_filtered_sorted)


def test_call_fails_loudly_on_every_null_argument():
    lib = runtime.load_library()
    d = runtime.export_desc([(A.POSITION.id, 0)], 0x1000, 16, 1)
    f = runtime.export_filter("sphere", sphere=(0, 0, 0, 1))
    s = runtime.export_sort("depth", v=(0, 0, 1))
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    good = [fake, C.byref(d), C.byref(f), C.byref(s)]
    for i in range(4):
        args = list(good)
        args[i] = None
        assert lib.hnb_effect_export_filtered_sorted(*args) == -1 and b"NULL" in lib.hnb_last_error(), i
    assert lib.hnb_effect_export_filtered_sorted(None, None, None, None) == -1 and b"NULL" in lib.hnb_last_error()


# ---- the code objects ---------------------------------------------------------------------------------------------------------------------------
def test_fourth_code_object_is_built_carried_and_has_two_kernels_without_scratch_or_spills():
    co = hb.export_cull_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_export_cull.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(CULL_KERNELS), sorted(rows)
    for name, r in rows.items():
        assert 0 < r["group_segment_fixed_size"] <= 32 * 1024, f"{name}: {r['group_segment_fixed_size']} B of LDS per workgroup"
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
    sort_rows, filter_rows = _rows(hb.export_sort_code_path()), _rows(hb.export_filter_code_path())
    # the keys kernel is the sorted export's with another row source; the tile kernel declares what the two tile kernels it joins declare
    assert rows["k_export_cull_keys"]["group_segment_fixed_size"] == sort_rows["k_export_sort_keys"]["group_segment_fixed_size"] == 4 * 256 * 4
    lds = rows["k_export_cull_tile"]["group_segment_fixed_size"]
    both = sort_rows["k_export_sort_tile"]["group_segment_fixed_size"] + filter_rows["k_export_filter_tile"]["group_segment_fixed_size"]
    assert both - 16 <= lds <= both + 16 and lds < 8 * 1024, (lds, both)
    # one argument block for both: an ExportFilterArgs and an ExportSortArgs, neither grown
    assert rows["k_export_cull_keys"]["kernarg_segment_size"] == rows["k_export_cull_tile"]["kernarg_segment_size"]
    assert rows["k_export_cull_keys"]["kernarg_segment_size"] == filter_rows["k_export_filter_tile"]["kernarg_segment_size"] + sort_rows["k_export_sort_tile"]["kernarg_segment_size"]
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    for other in (hb.export_code_path(), hb.export_sort_code_path(), hb.export_filter_code_path()):
        assert open(other, "rb").read() in lib                           # four embedded code objects
    import inspect
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_export_cull_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "bevy_hanabi_amd", "csrc", "hnb_export_cull.hip")).read()
    assert hb.build_export_cull_code in hb.EXPORT_CODE_OBJECTS


def test_third_code_object_keeps_its_kernels_and_resource_rows():
    """tests/golden/export_filter_code_object_rows.json: the rows of hnb_export_filter.hsaco as they were while mark_tile, tile_prefix, keeps_slot and
    filter_source lived in hnb_export_filter.hip itself."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "export_filter_code_object_rows.json")))["hnb_export_filter"]
    rows = _rows(hb.export_filter_code_path())
    assert sorted(rows) == sorted(golden) == sorted(FILTER_KERNELS)
    for name, want in golden.items():
        assert rows[name] == want, (name, rows[name], want)


# ---- the launch plan and the scratch layout (csrc/hnb_export.h), as stand-alone host programs ----------------------------------------------------
def cull_plan_table(cap, stride):
    """The launches of the new form as the design states them"""
    T = -(-cap // 4096)
    v = {32: 0, 64: 1, 128: 2, 256: 3}[stride]
    G = -(-cap // (128 if v == 3 else 256))
    if T <= 1:
        return [("kExpCullTile", 1, 1, "cull", 0), (f"kExpSortRows{v}", G, 1, "rows", 0)], None
    L = [("kExpFilterMark", T, 1, "filter", 0), ("kExpFilterScan", 1, 1, "filter", 0), ("kExpFilterCompact", T, 1, "filter", 0),
         ("kExpCullKeys", T, 1, "cull", 0), ("kExpSortScatter", T, 1, "sort+pass", 0)]
    for p in (1, 2, 3):
        L += [("kExpSortHist", T, 1, "sort+pass", p), ("kExpSortScatter", T, 1, "sort+pass", p)]
    L.append((f"kExpSortRows{v}", G, 1, "rows", 0))
    return L, 3


def filter_total(cap):
    """export_filter_scratch_layout(cap).total restated"""
    tiles, off = -(-cap // 4096), 0
    for size in (4 * cap, tiles * 512, tiles * 4, tiles * 4):
        off = (off + size + 255) & ~255
    return off + 256


def test_launch_plan_of_the_new_form_is_the_designs_table(tmp_path):
    names = ["kExpCullTile", "kExpCullKeys", "kExpFilterMark", "kExpFilterScan", "kExpFilterCompact", "kExpSortHist", "kExpSortScatter"] + [f"kExpSortRows{v}" for v in range(4)]
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
        static_assert(kExpCullTile == 36 && kExpCullKeys == 37 && kExpFilterRowsInst0 == 38, "the fourth unit's are numbered behind the 36 kernels of the first three");
        static_assert(kUnitExportCull == 3, "the fourth unit");
        static_assert(kExportPlain == 0 && kExportSorted == 1 && kExportFiltered == 2 && kExportFilteredSorted == 3, "forms");
        static const char* const args[] = {"rows", "sort", "sort+pass", "filter", "offsets", "cull"};
        static_assert(kExportArgsRows == 0 && kExportArgsSort == 1 && kExportArgsSortPass == 2 && kExportArgsFilter == 3 && kExportArgsOffsets == 4 && kExportArgsCull == 5, "args[]");
        static_assert(sizeof(ExportCullArgs) == sizeof(ExportFilterArgs) + sizeof(ExportSortArgs), "one filter block and one sort block");
        unsigned cap, stride;
        while (std::scanf("%u %u", &cap, &stride) == 2) {
            const ExportPlan pl = export_launch_plan(kExportFilteredSorted, false, HNB_SORT_SCOPE_INSTANCE, 1, cap, stride);
            if (pl.n > kExportPlanMax) return 2;
            std::printf("%u %d %llu %llu", pl.n, pl.memset_before == kExportNoMemset ? -1 : (int)pl.memset_before, (unsigned long long)pl.zero_off, (unsigned long long)pl.zero_bytes);
            for (uint32_t i = 0; i < pl.n; ++i) std::printf(" %s %u %u %s %u", kernel_name(pl.launch[i].kernel), pl.launch[i].grid_x, pl.launch[i].grid_y, args[pl.launch[i].args], pl.launch[i].pass);
            std::printf("\n");
        }
        return 0;
    }
    """)
    cases = [(cap, stride) for cap in (300, 4096, 4097, 10_000) for stride in (32, 256)]
    out = subprocess.run([exe], input="\n".join("%d %d" % c for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (cap, stride), line in zip(cases, out):
        w = line.split()
        count, memset, zero_off, zero_bytes = int(w[0]), int(w[1]), int(w[2]), int(w[3])
        got = [(w[i], int(w[i + 1]), int(w[i + 2]), w[i + 3], int(w[i + 4])) for i in range(4, len(w), 5)]
        want, want_memset = cull_plan_table(cap, stride)
        assert count == len(got) <= 12 and got == want, (cap, stride, got, want)
        assert count == (2 if cap <= 4096 else 12)
        assert memset == (-1 if want_memset is None else want_memset), (cap, stride, memset)
        if want_memset is not None:                                      # the state words and group sums of the sort section, which lies behind the filter's
            assert got[memset][0] == "kExpCullKeys"
            l = sort_layout(1, cap, 0)
            assert (zero_off, zero_bytes) == (filter_total(cap) + l[6], l[9]), (cap, stride, zero_off, zero_bytes, l)


def test_scratch_layout_is_the_filters_then_the_sorts_aligned_and_inside(tmp_path):
    exe = _standalone(tmp_path, "cl", r"""
    #include <cstdio>
    #include <cstdint>
    #include "hnb_export.h"
    int main() {
        unsigned long long cap;
        while (std::scanf("%llu", &cap) == 1) {
            const hnb::ExportCullScratch l = hnb::export_cull_scratch_layout((uint32_t)cap);
            const hnb::ExportFilterScratch f = hnb::export_filter_scratch_layout((uint32_t)cap);
            const hnb::ExportSortScratch s = hnb::export_sort_scratch_layout(1u, (uint32_t)cap, HNB_SORT_SCOPE_INSTANCE);
            const bool same = l.filter.total == f.total && l.filter.order_off == f.order_off && l.filter.mask_off == f.mask_off && l.filter.count_off == f.count_off &&
                              l.filter.offset_off == f.offset_off && l.filter.state_off == f.state_off && l.filter.tiles == f.tiles && l.sort.rows == s.rows &&
                              l.sort.pitch == s.pitch && l.sort.vals_off == s.vals_off && l.sort.state_off == s.state_off && l.sort.gsum_off == s.gsum_off &&
                              l.sort.hist_off == s.hist_off && l.sort.zero_bytes == s.zero_bytes && l.sort.total == s.total;
            std::printf("%d %u %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (int)same, l.sort.rows, (unsigned long long)l.filter.order_off,
                        (unsigned long long)l.filter.mask_off, (unsigned long long)l.filter.count_off, (unsigned long long)l.filter.offset_off, (unsigned long long)l.filter.state_off,
                        (unsigned long long)l.filter.total, (unsigned long long)l.sort_off, (unsigned long long)l.sort.vals_off, (unsigned long long)l.sort.state_off,
                        (unsigned long long)l.sort.gsum_off, (unsigned long long)l.sort.hist_off, (unsigned long long)l.sort.total, (unsigned long long)l.total);
        }
        return 0;
    }
    """)
    caps = [1, 63, 64, 300, 4095, 4096, 4097, 10_000, 131_072, 131_073, 135_245, 16_777_216, 0xFFFFFF00, 0xFFFFFF01, (1 << 32) - 1]
    out = subprocess.run([exe], input="\n".join(str(c) for c in caps), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(caps)
    for cap, line in zip(caps, out):
        same, rows, order, mask, count, offset, state, ftotal, sort_off, vals, sstate, gsum, hist, stotal, total = [int(x) for x in line.split()]
        assert same == 1, cap                                            # the two layouts it is made of, unchanged
        if cap > 0xFFFFFF00:
            assert rows == 0, cap                                        # refused, as the sorted export refuses it
            continue
        assert rows == cap
        tiles = -(-cap // 4096)
        groups = -(-tiles // 32)
        pitch = (cap + 63) & ~63
        # (offset, bytes) in the order of the allocation: the filter's order, mask, tile counts, tile offsets and the 32-byte row that holds the kept
        # count; the sort's keys, vals, state, gsum, hist
        sects = [(order, 4 * cap), (mask, 512 * tiles), (count, 4 * tiles), (offset, 4 * tiles), (state, 32),
                 (sort_off, 8 * pitch), (sort_off + vals, 8 * pitch), (sort_off + sstate, 16), (sort_off + gsum, 8192 * groups), (sort_off + hist, 4096 * tiles)]
        end = 0
        for off, size in sects:
            assert off >= end and off % 256 == 0 and size > 0, (cap, sects)
            end = off + size
        assert state + 32 <= ftotal <= sort_off and sort_off % 256 == 0
        assert end == sort_off + stotal == total, (cap, sects, total)
        assert total <= 20 * pitch + 8192 * groups + (4096 + 520) * tiles + 8 * 256      # 20 bytes per slot, the digit tables, the mask and tile words, the alignment
