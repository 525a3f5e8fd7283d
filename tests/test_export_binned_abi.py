"""The binned export (hnb_effect_export_binned, include/hanabi_amd_binned.h) without a GPU: header, ctypes mirror and INTEGRATION.md agree
on HnbExportBins and the prototype, and hanabi_amd.h declares what it declared; the cell function of csrc/hnb_bin_cell.h, compiled as a
stand-alone host program under the address and undefined-behaviour sanitizers, gives the cells of a numpy restatement on cell edges, signed
zeros, infinities, NaNs and a grid of exactly 2^24 cells; the form's launch plan (csrc/hnb_export_bin.h) from the same kind of program is the
design's table and leaves every other form's plan alone; the three kernels live in a code object of their own with no scratch and no spills;
NULL arguments fail loudly."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import runtime
from test_export_filtered_abi import CSRC, INSTANCE, _rows, _standalone, plan_table, sort_layout
from test_export_sorted_abi import A, LLVM, ROOT

BIN_KERNELS = ["k_export_bin_keys", "k_export_bin_tile", "k_export_bin_starts"]
F32 = np.float32


# ---- the semantics, restated in numpy -----------------------------------------------------------------------------------------------------------------
def np_cells(p, dims, origin, inv_cell):
    """p: [n, 3] binary32 positions -> [n] uint32 cells, the header's formulas operation by operation in binary32: per axis t = (p - origin) * inv_cell,
    inside iff t >= 0 and t < (float)dims (a NaN compares false), i = trunc(t) behind that test; (i2 * d1 + i1) * d0 + i0, or n_cells outside."""
    p = np.asarray(p, F32).reshape(-1, 3)
    dims = [int(d) for d in dims]
    origin, inv_cell = np.asarray(origin, F32), np.asarray(inv_cell, F32)
    n_cells = dims[0] * dims[1] * dims[2]
    inside = np.ones(len(p), bool)
    idx = []
    with np.errstate(all="ignore"):
        for c in range(3):
            d = p[:, c] - origin[c]
            t = d * inv_cell[c]
            assert d.dtype == F32 and t.dtype == F32
            ok = (t >= F32(0)) & (t < F32(dims[c]))
            idx.append(np.where(ok, t, F32(0)).astype(np.uint32).astype(np.uint64))     # converted only where the range test passed
            inside &= ok
    cell = (idx[2] * np.uint64(dims[1]) + idx[1]) * np.uint64(dims[0]) + idx[0]
    return np.where(inside, cell, np.uint64(n_cells)).astype(np.uint32)


def np_table(sorted_cells, n_cells):
    """cell_start[c] = the rows whose cell is smaller than c, c = 0 .. n_cells + 1"""
    return np.searchsorted(np.asarray(sorted_cells, np.uint32), np.arange(n_cells + 2, dtype=np.uint32), "left").astype(np.uint32)


def test_the_restatement_itself_on_a_case_worked_by_hand():
    dims, origin, inv = (4, 2, 3), (1.0, -1.0, 0.0), (2.0, 1.0, 0.5)      # cells of 0.5 x 1 x 2 from (1, -1, 0): x in [1, 3), y in [-1, 1), z in [0, 6)
    p = [(1.0, -1.0, 0.0), (1.49, -0.5, 1.9), (1.5, 0.0, 2.0), (2.99, 0.99, 5.99), (3.0, 0.0, 0.0), (0.99, 0.0, 0.0), (2.0, np.nan, 1.0), (2.0, 0.0, np.inf),
         (2.0, 0.0, -0.0), (-np.inf, 0.0, 1.0)]
    want = [0, 0, (1 * 2 + 1) * 4 + 1, (2 * 2 + 1) * 4 + 3, 24, 24, 24, 24, (0 * 2 + 1) * 4 + 2, 24]
    assert list(np_cells(p, dims, origin, inv)) == want
    assert list(np_table(sorted(want), 24)) == [0] + [2] * 6 + [3] * 7 + [4] * 10 + [5, 10]      # entry c: the rows below cell c; [24]: first outside; [25]: all


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_header_and_integration_agree_on_the_struct_and_the_prototype(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd_binned.h"
    int main(void) {
        int (*f)(HnbEffect*, const HnbExportDesc*, const HnbExportBins*) = hnb_effect_export_binned;
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %u\n", sizeof(HnbExportBins), offsetof(HnbExportBins, struct_size), offsetof(HnbExportBins, flags), offsetof(HnbExportBins, dims),
               offsetof(HnbExportBins, reserved), offsetof(HnbExportBins, origin), offsetof(HnbExportBins, inv_cell), offsetof(HnbExportBins, cell_start), HNB_BIN_MAX_CELLS);
        return f == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    S = runtime.ExportBins
    assert got == [56, 0, 4, 8, 20, 24, 36, 48, 1 << 24]
    assert [C.sizeof(S), S.struct_size.offset, S.flags.offset, S.dims.offset, S.reserved.offset, S.origin.offset, S.inv_cell.offset, S.cell_start.offset] == got[:8]
    assert runtime.BIN_MAX_CELLS == got[8]
    g = runtime.export_bins((8, 4, 2), (1, 2, 3), (0.5, 0.25, 4), 0x1000)
    assert (g.struct_size, g.flags, list(g.dims), g.reserved, list(g.origin), list(g.inv_cell), g.cell_start) == (56, 0, [8, 4, 2], 0, [1.0, 2.0, 3.0], [0.5, 0.25, 4.0], 0x1000)
    lib = runtime.load_library()
    assert runtime.ABI_BINNED_SYMBOLS == ["hnb_effect_export_binned"] and hasattr(lib, "hnb_effect_export_binned")
    assert lib.hnb_effect_export_binned.argtypes == [C.c_void_p, C.POINTER(runtime.ExportDesc), C.POINTER(runtime.ExportBins)]
    assert list(inspect.signature(runtime.Effect.export_binned).parameters) == ["self", "fields", "dst_ptr", "stride", "capacity_records", "count_ptr", "dims", "origin", "inv_cell",
                                                                                "cell_start_ptr"]
    full = open(os.path.join(ROOT, "include", "hanabi_amd_binned.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    m = re.search(r"int\s+hnb_effect_export_binned\s*\(([^)]*)\)\s*;", header)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["HnbEffect* fx", "const HnbExportDesc* desc", "const HnbExportBins* bins"]
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header)) == set(runtime.ABI_BINNED_SYMBOLS)        # the companion header: this one entry point
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", main)) == set(runtime.ABI_SYMBOLS) and "hnb_effect_export_binned" not in runtime.ABI_SYMBOLS
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"\bfn hnb_effect_export_binned\(([^)]*)\) -> c_int;", txt)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["fx: *mut HnbEffect", "desc: *const HnbExportDesc", "bins: *const HnbExportBins"]
    m = re.search(r"#\[repr\(C\)\]\s*pub struct HnbExportBins \{(.*?)\}", txt, flags=re.S)
    assert m, "INTEGRATION.md mirrors the struct"
    members = [" ".join(line.split("//")[0].split()).rstrip(",") for line in m.group(1).splitlines() if line.split("//")[0].strip()]
    assert members == ["pub struct_size: u32", "pub flags: u32", "pub dims: [u32; 3]", "pub reserved: u32", "pub origin: [f32; 3]", "pub inv_cell: [f32; 3]", "pub cell_start: *mut u32"]
    for word in ("a program form", "a filter in front of the binning", "any transform"):       # what is out of scope is said where a caller reads it
        assert word in full, word


def test_call_fails_loudly_on_null_arguments_and_without_a_device():
    """Up to the device check: the NULL refusals come before anything is dereferenced, loaded or enqueued. The refusals of a descriptor's members
    need an effect, and an effect a device: tests/test_gpu_export_binned.py holds them."""
    lib = runtime.load_library()
    d = runtime.export_desc([(A.POSITION.id, 0)], 0x1000, 16, 1)
    g = runtime.export_bins((1, 1, 1), (0, 0, 0), (1, 1, 1), 0x1000)
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for args in ((None, C.byref(d), C.byref(g)), (fake, None, C.byref(g)), (fake, C.byref(d), None), (None, None, None)):
        assert lib.hnb_effect_export_binned(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to export from, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the cell function (csrc/hnb_bin_cell.h), as a stand-alone host program under the sanitizers ---------------------------------------------------------
CELL_SRC = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "hnb_bin_cell.h"
using namespace hnb;
static float f(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }
// input: "d0 d1 d2 o0 o1 o2 i0 i1 i2 n" (floats as hex bits), then n rows "x y z" of hex bits; output: the grid's cell count, then the cell of every row
int main() {
    unsigned d[3], o[3], iv[3], n;
    while (std::scanf("%u %u %u %x %x %x %x %x %x %u", &d[0], &d[1], &d[2], &o[0], &o[1], &o[2], &iv[0], &iv[1], &iv[2], &n) == 10) {
        BinGrid g;
        for (int c = 0; c < 3; ++c) { g.dims[c] = d[c]; g.origin[c] = f(o[c]); g.inv_cell[c] = f(iv[c]); }
        g.n_cells = bin_cell_count(g.dims);
        std::printf("%u", g.n_cells);
        for (unsigned i = 0; i < n; ++i) {
            unsigned p[3];
            if (std::scanf("%x %x %x", &p[0], &p[1], &p[2]) != 3) return 1;
            std::printf(" %u", bin_cell_of(g, f(p[0]), f(p[1]), f(p[2])));
        }
        std::printf("\n");
    }
    return 0;
}
"""


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def _ulp(x, k):
    """x moved k binary32 steps (x finite and not 0)"""
    b = np.asarray(x, F32).view(np.int32)
    return (b + np.where(b < 0, -k, k).astype(np.int32)).view(F32)


def edge_positions(dims, origin, inv_cell, rng):
    """Rows that sit on what the cell function can get wrong: per axis every cell edge origin + k / inv_cell exactly and one step either side (all of
    them for small grids, a sample and both ends for large ones), -0 and +0, the infinities, NaNs of both signs, the largest finite values, t just
    below and exactly at dims[c]; the other two axes in the middle of the grid, or somewhere."""
    origin, inv_cell = np.asarray(origin, F32), np.asarray(inv_cell, F32)
    mid = np.array([origin[c] + (F32(dims[c]) * F32(0.5)) / inv_cell[c] for c in range(3)], F32)
    rows = []
    for c in range(3):
        ks = np.arange(dims[c] + 1) if dims[c] <= 64 else np.unique(np.concatenate([[0, 1, 2, dims[c] - 1, dims[c]], rng.integers(0, dims[c] + 1, 40)]))
        edges = (origin[c] + ks.astype(F32) / inv_cell[c]).astype(F32)
        top = (origin[c] + F32(dims[c]) / inv_cell[c]).astype(F32)
        vals = [edges, _ulp(np.where(edges == 0, F32(1e-30), edges), 1), _ulp(np.where(edges == 0, F32(1e-30), edges), -1), [top, _ulp(top, -1), _ulp(top, 1)],
                [F32(0.0), F32(-0.0), np.inf, -np.inf, np.nan, -np.nan, F32(3.4028235e38), F32(-3.4028235e38), F32(1e-45), F32(-1e-45), origin[c]]]
        for v in np.concatenate([np.asarray(x, F32).reshape(-1) for x in vals]):
            p = mid.copy()
            p[c] = v
            rows.append(p)
    rows += list(rng.uniform(-1.5, 1.5, (200, 3)).astype(F32) * (F32(dims[0]) / inv_cell[0]) + mid)      # ... and a cloud over and around the grid
    return np.array(rows, F32)


GRIDS = [((1, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),                    # dims of 1: one cell and the outside bin
         ((1, 1, 1), (-3.0, -3.0, -3.0), (1 / 6, 1 / 6, 1 / 6)),
         ((8, 8, 8), (-1.0, -1.0, -1.0), (4.0, 4.0, 4.0)),
         ((5, 1, 7), (0.1, -0.0, 1e-3), (1 / 0.3, 0.7, 3.0)),             # edges that are no binary fractions: origin + k / inv_cell rounds
         ((17, 5, 3), (-2.5, 0.25, 10.0), (3.0, 1.5, 0.125)),             # 255 cells
         ((256, 256, 256), (-1.0, -2.0, -3.0), (128.0, 64.0, 100.0)),     # exactly 2^24 cells
         ((1 << 24, 1, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),             # ... along one axis: t up to 2^24, the largest index a binary32 still counts
         ((64, 64, 32), (-40.0, -40.0, -40.0), (0.8, 0.8, 0.4))]


def test_cell_function_under_the_sanitizers_is_the_numpy_restatement(tmp_path):
    exe = _standalone(tmp_path, "cell", CELL_SRC)
    rng = np.random.default_rng(24)
    lines, want = [], []
    for dims, origin, inv in GRIDS:
        p = edge_positions(dims, origin, inv, rng)
        lines.append("%d %d %d " % dims + " ".join(f"{int(b):x}" for b in np.concatenate([_bits(origin), _bits(inv)])) + f" {len(p)}")
        lines += [" ".join(f"{int(b):x}" for b in _bits(row)) for row in p]
        want.append((dims, np_cells(p, dims, origin, inv)))
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()      # (a sanitizer report ends the program with an error)
    assert len(out) == len(GRIDS)
    seen_outside = seen_last = 0
    for line, (dims, cells) in zip(out, want):
        n_cells = dims[0] * dims[1] * dims[2]
        got = np.array([int(x) for x in line.split()], np.uint32)
        assert got[0] == n_cells
        np.testing.assert_array_equal(got[1:], cells, err_msg=str(dims))
        assert cells.max() <= n_cells
        seen_outside += int((cells == n_cells).sum())
        seen_last += int((cells == n_cells - 1).sum())
    assert seen_outside > 100 and seen_last > 8                                    # both sides of the upper edge occurred
    # -0 at the origin is inside, in cell 0 of its axis; t exactly at dims is outside, one step below it inside the last cell
    assert list(np_cells([(-0.0, 0.0, 0.0), (8.0, 0.0, 0.0), (_ulp(F32(8.0), -1), 0.0, 0.0)], (8, 1, 1), (0, 0, 0), (1, 1, 1))) == [0, 8, 7]
    # the cell counts the runtime refuses: a dimension of 0, a product above 2^24 (taken in 64 bits: 65536^3 is 0 modulo 2^32)
    refused = [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1 << 24, 2, 1), (4097, 4096, 1), (65536, 65536, 65536), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (1 << 31, 2, 1)]
    lines = ["%d %d %d 0 0 0 3f800000 3f800000 3f800000 0" % d for d in refused + [(4096, 4096, 1), (1, 1, 1)]]
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [0] * len(refused) + [1 << 24, 1]


# ---- the launch plan (csrc/hnb_export.h), as a stand-alone host program under the sanitizers ----------------------------------------------------------
def binned_plan_table(cap, stride, n_cells):
    """The launches of a binned export as the issue lists them: (tile | memset + keys + the hist / scatter passes) + starts + gather"""
    T = -(-cap // 4096)
    v = {32: 0, 64: 1, 128: 2, 256: 3}[stride]
    L, memset = [], None
    if T <= 1:
        L.append(("kBinKTile", 1, 1, "bin", 0))
    else:
        memset = 0
        L += [("kBinKKeys", T, 1, "bin", 0), ("kExpSortScatter", T, 1, "sort+pass", 0)]
        for p in (1, 2, 3):
            L += [("kExpSortHist", T, 1, "sort+pass", p), ("kExpSortScatter", T, 1, "sort+pass", p)]
    L.append(("kBinKStarts", -(-(n_cells + 2) // 256), 1, "bin", 0))
    L.append((f"kExpSortRows{v}", -(-cap // (128 if v == 3 else 256)), 1, "rows", 0))
    return L, memset


def test_plan_of_the_binned_form_is_the_listed_one_and_every_other_forms_plan_is_unchanged(tmp_path):
    kernels = (["kExpOffsets"] + [f"kExp{f}Rows{s}{v}" for f, s in (("", ""), ("Sort", ""), ("Sort", "Inst"), ("Sort", "All"), ("Filter", "")) for v in range(4)]
               + [f"kExpSort{k}{s}" for s in ("", "Inst") for k in ("Tile", "Keys", "Hist", "Scatter")] + ["kExpSortFill", "kExpSortHistAll", "kExpSortScatterAll"]
               + [f"kExpFilter{k}" for k in ("Tile", "Mark", "Scan", "Compact")])
    exe = _standalone(tmp_path, "bpl", r"""
    #include <cstdio>
    #include <cstdint>
    #include "hnb_export_bin.h"
    using namespace hnb;
    static const char* kernel_name(uint32_t k) {
        switch (k) {
        case kExportBinKernelBase + kBinKTile: return "kBinKTile";
        case kExportBinKernelBase + kBinKKeys: return "kBinKKeys";
        case kExportBinKernelBase + kBinKStarts: return "kBinKStarts";
    """ + "\n".join(f'        case {k}: return "{k}";' for k in kernels) + r"""
        }
        return "?";
    }
    int main() {
        // numbered apart: the units, kernels and argument blocks of hnb_export.h are what they were
        static_assert(kExpCullKeysInst == 47 && kExpKernelCount == 48 && kExportUnitCount == 6 && kExportArgsCullProg == 7 && kExportPlanMax == 13, "hnb_export.h");
        static_assert(kBinKTile == 0 && kBinKKeys == 1 && kBinKStarts == 2 && kExportBinKernelCount == 3 && kExportBinKernelBase == 0x100 && kExportArgsBin == 8, "hnb_export_bin.h");
        static_assert(sizeof(ExportBinArgs) == sizeof(ExportSortArgs) + sizeof(BinGrid) + 8 && sizeof(BinGrid) == 40, "a sort block, the grid and the table");
        static const char* const args[] = {"rows", "sort", "sort+pass", "filter", "offsets", "cull", "filter+inst", "cull+inst", "bin"};
        unsigned form, program, scope, n, cap, stride, n_cells;
        while (std::scanf("%u %u %u %u %u %u %u", &form, &program, &scope, &n, &cap, &stride, &n_cells) == 7) {
            const ExportPlan pl = form == 4 ? export_bin_launch_plan(cap, stride, n_cells) : export_launch_plan(form, program != 0, scope, n, cap, stride);
            if (pl.n > kExportPlanMax) return 2;
            std::printf("%u %d %llu %llu", pl.n, pl.memset_before == kExportNoMemset ? -1 : (int)pl.memset_before, (unsigned long long)pl.zero_off, (unsigned long long)pl.zero_bytes);
            for (uint32_t i = 0; i < pl.n; ++i) {
                const uint32_t k = pl.launch[i].kernel;
                if ((k >= kExpKernelCount && (k < kExportBinKernelBase || k >= kExportBinKernelBase + kExportBinKernelCount)) || pl.launch[i].args > kExportArgsBin) return 3;
                std::printf(" %s %u %u %s %u", kernel_name(pl.launch[i].kernel), pl.launch[i].grid_x, pl.launch[i].grid_y, args[pl.launch[i].args], pl.launch[i].pass);
            }
            std::printf("\n");
        }
        return 0;
    }
    """)

    def run(cases):
        out = subprocess.run([exe], input="\n".join("%d %d %d %d %d %d %d" % c for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        res = []
        for line in out:
            w = line.split()
            res.append((int(w[0]), int(w[1]), int(w[2]), int(w[3]), [(w[i], int(w[i + 1]), int(w[i + 2]), w[i + 3], int(w[i + 4])) for i in range(4, len(w), 5)]))
        return res

    caps = (300, 4096, 4097, 135_245)
    cases = [(4, 0, INSTANCE, 1, cap, stride, n_cells) for cap in caps for stride in (32, 256) for n_cells in (1, 254, 255, 512, 65_536, 1 << 24)]
    for case, (count, memset, zero_off, zero_bytes, got) in zip(cases, run(cases)):
        _, _, _, _, cap, stride, n_cells = case
        want, want_memset = binned_plan_table(cap, stride, n_cells)
        assert count == len(got) <= 11 and got == want, (case, got, want)
        assert count == (3 if cap <= 4096 else 10), case
        assert memset == (-1 if want_memset is None else want_memset), case
        if want_memset is not None:                                      # the state words and group sums of export_sort_scratch_layout(1, capacity, INSTANCE)
            l = sort_layout(1, cap, INSTANCE)
            assert (zero_off, zero_bytes) == (l[6], l[9]), (case, zero_off, zero_bytes, l)
        starts = [g for g in got if g[0] == "kBinKStarts"]
        assert len(starts) == 1 and (starts[0][1] - 1) * 256 < n_cells + 2 <= starts[0][1] * 256        # sized from n_cells: one lane per entry
        assert all(gx == (-(-cap // 4096) if k != "kBinKTile" else 1) for k, gx, _, _, _ in got[:-2])  # ... and every other grid from the capacity
    # every existing form: the table tests/test_export_filtered_abi.py holds
    forms = {"plain": 0, "sorted": 1, "filtered": 2}
    old = [(form, program, scope, n, cap, stride) for form, program, scope in (("plain", 0, 0), ("plain", 1, 0), ("sorted", 0, 0), ("sorted", 1, 0), ("sorted", 1, 1), ("filtered", 0, 0))
           for cap in caps for n in (1, 5) for stride in (32, 256)]
    for case, (count, memset, _, _, got) in zip(old, run([(forms[c[0]],) + c[1:] + (0,) for c in old])):
        want, want_memset = plan_table(*case)
        assert got == want and memset == (-1 if want_memset is None else want_memset), (case, got)


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------
def test_code_object_is_gfx950_embedded_and_holds_three_kernels_without_scratch_or_spills():
    co = hb.export_bin_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_export_bin.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(BIN_KERNELS), sorted(rows)
    for name, r in rows.items():
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)                           # eight waves per SIMD stay possible
    kernarg = {r["kernarg_segment_size"] for r in rows.values()}
    sort_rows = _rows(hb.export_sort_code_path())
    assert kernarg == {sort_rows["k_export_sort_keys"]["kernarg_segment_size"] + 48}          # one ExportBinArgs by value: a sort block, the grid, the table
    # LDS as the sources declare: the keys kernel's four 256-bin histograms, the one-workgroup sort's bases, wave counters and OR words (the sorted
    # export's own kernels declare the same), none in the table kernel
    lds = {n: r["group_segment_fixed_size"] for n, r in rows.items()}
    assert lds == {"k_export_bin_keys": 4 * 256 * 4, "k_export_bin_tile": 256 * 4 + 4 * 256 * 4 + 2 * 4 * 4, "k_export_bin_starts": 0}
    assert lds["k_export_bin_keys"] == sort_rows["k_export_sort_keys"]["group_segment_fixed_size"] and lds["k_export_bin_tile"] == sort_rows["k_export_sort_tile"]["group_segment_fixed_size"]
    src = open(os.path.join(CSRC, "hnb_export_bin.hip")).read()
    assert len(re.findall(r'extern "C" __global__ void __launch_bounds__\(256\) k_export_bin_', src)) == len(re.findall(r"__global__", src)) == 3
    assert "#pragma clang fp contract(off)" in src and "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_bin_cell.h")).read()
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_export_bin_code)
    assert hb.BINNED_CODE_OBJECTS == (hb.build_export_bin_code,) and hb.build_export_bin_code not in hb.EXPORT_CODE_OBJECTS + hb.QUERY_CODE_OBJECTS
    assert "BINNED_CODE_OBJECTS" in inspect.getsource(hb.build_runtime)
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    for other in (hb.export_code_path(), hb.export_sort_code_path(), hb.export_filter_code_path(), hb.export_cull_code_path(), hb.export_filter_prog_code_path(),
                  hb.export_cull_prog_code_path()):
        assert open(other, "rb").read() in lib and not set(_rows(other)) & set(BIN_KERNELS)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_export_bin_code.inc" in ignored and "*.hsaco" in ignored
