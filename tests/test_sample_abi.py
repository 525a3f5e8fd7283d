"""The sample (hnb_effect_sample, include/hanabi_amd_sample.h) without a GPU: header, ctypes mirrors and INTEGRATION.md agree on the structures and the
prototype, and the call fails loudly; the plain C++ of csrc/hnb_sample.h - the sampling rule the kernels call, the check of a description and the
launch plan - compiled as a stand-alone host program under the address and undefined-behaviour sanitizers gives what the restatements in numpy /
Python give, bit for bit; the two kernels live in a code object of their own with no scratch and no spills. The restatements here (np_sample,
np_store, sample_plan) are what tests/test_gpu_sample.py expects."""
import ctypes as C
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import runtime
from test_export_binned_abi import np_cells
from test_export_filtered_abi import CSRC, _rows
from test_export_sorted_abi import A, LLVM, ROOT

SAMPLE_KERNELS = ["k_sample_nearest", "k_sample_trilinear"]
NEAREST, TRILINEAR, SET, ADD = 0, 1, 0, 1
TILE = 4096
F32, U32 = np.float32, np.uint32


# ---- the semantics, restated in numpy: binary32 arrays, one operation per statement ---------------------------------------------------------------
def np_axis(t, dim):
    """t: [n] binary32, inside [0, dim) -> (lo, hi [n] int64: the two cell centres' indices, clamped; w [n] binary32; clamped [n] bool)"""
    u = t - F32(0.5)
    fl = np.floor(u)
    w = u - fl
    assert u.dtype == F32 and fl.dtype == F32 and w.dtype == F32
    j = fl.astype(np.int64)
    return np.maximum(j, 0), np.minimum(j + 1, dim - 1), w, (j < 0) | (j + 1 > dim - 1)


def np_lerp(lo, hi, w):
    d = hi - lo
    m = w * d
    assert d.dtype == F32 and m.dtype == F32
    return lo + m


def np_sample(pos, field, dims, origin, inv_cell, mode):
    """pos: [n, 3] binary32; field: [n_cells, k] binary32 -> (inside [n] bool: sampled, else the outside bin; s [n, k] binary32, 0 where outside;
    clamped [n] bool: inside with a corner clamped on some axis - of the trilinear stencil, whatever the mode)"""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    dims = [int(d) for d in dims]
    origin, inv_cell = np.asarray(origin, F32), np.asarray(inv_cell, F32)
    field = np.asarray(field, F32).reshape(dims[0] * dims[1] * dims[2], -1)
    cells = np_cells(pos, dims, origin, inv_cell).astype(np.int64)
    inside = cells != len(field)
    p = pos[inside]
    s = np.zeros((len(pos), field.shape[1]), F32)
    clamped = np.zeros(len(pos), bool)
    with np.errstate(all="ignore"):
        ax = []
        for c in range(3):
            d = p[:, c] - origin[c]
            t = d * inv_cell[c]
            ax.append(np_axis(t, dims[c]))
        clamped[inside] = ax[0][3] | ax[1][3] | ax[2][3]
        if mode == NEAREST:
            s[inside] = field[cells[inside]]
        else:
            (lo0, hi0, w0, _), (lo1, hi1, w1, _), (lo2, hi2, w2, _) = ax
            F = lambda x, y, z: field[(z * dims[1] + y) * dims[0] + x]
            w0, w1, w2 = w0[:, None], w1[:, None], w2[:, None]
            a00 = np_lerp(F(lo0, lo1, lo2), F(hi0, lo1, lo2), w0)
            a10 = np_lerp(F(lo0, hi1, lo2), F(hi0, hi1, lo2), w0)
            a01 = np_lerp(F(lo0, lo1, hi2), F(hi0, lo1, hi2), w0)
            a11 = np_lerp(F(lo0, hi1, hi2), F(hi0, hi1, hi2), w0)
            b0 = np_lerp(a00, a10, w1)
            b1 = np_lerp(a01, a11, w1)
            s[inside] = np_lerp(b0, b1, w2)
    return inside, s, clamped


def np_store(op, v, s, scale):
    """v, s: binary32 arrays -> v' = s * scale (SET) or v + s * scale (ADD), each operation rounded to binary32; denormals are kept"""
    with np.errstate(all="ignore"):
        r = np.asarray(s, F32) * F32(scale)
        out = np.asarray(v, F32) + r if op == ADD else r
    assert out.dtype == F32
    return out


def same_bits_or_both_nan(got_bits, want_bits):
    """[n] bool: the bits agree, or the expectation is a NaN and so is the result (which NaN is unspecified)"""
    got, want = np.asarray(got_bits, U32), np.asarray(want_bits, U32)
    return (got == want) | (np.isnan(want.view(F32)) & np.isnan(got.view(F32)))


def sample_plan(mode, capacity):
    """sample_launch_plan restated -> (kernel, grid_x, grid_y, clear_stats_bytes): a workgroup per tile of 4096 slots, the kernel by the mode"""
    return (SAMPLE_KERNELS[mode], max(1, -(-capacity // TILE)), 1, 16)


def test_the_restatement_itself_on_cases_worked_by_hand():
    f = np.arange(8, dtype=F32).reshape(8, 1) * F32(10)                   # 2 x 2 x 2: the value of cell (x, y, z) is 10 (x + 2 y + 4 z)
    pos = np.array([(0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (1.5, 0.5, 0.5), (0.0, 0.0, 0.0), (1.99, 0.75, 1.0), (2.0, 0, 0), (np.nan, 0, 0), (-0.0, 0.5, 0.5)], F32)
    inside, s, clamped = np_sample(pos, f, (2, 2, 2), (0, 0, 0), (1, 1, 1), TRILINEAR)
    assert list(inside) == [True] * 5 + [False, False, True] and list(clamped) == [False, False, True, True, True, False, False, True]
    # a cell centre is its cell; the middle is the mean of all eight; past the last centre the edge is held
    assert s[:4, 0].tolist() == [0.0, 35.0, 10.0, 0.0] and s[7, 0] == 0.0
    assert s[4, 0] == F32(10) + (F32(0.25) * F32(20) + F32(0.5) * F32(40))       # x clamped to cell 1, y a quarter of the way, z half way
    inside, s, _ = np_sample(pos, f, (2, 2, 2), (0, 0, 0), (1, 1, 1), NEAREST)
    assert s[:5, 0].tolist() == [0.0, 70.0, 10.0, 0.0, 50.0] and not s[5:7].any()
    # 1 x 1 x 1: every corner is cell 0, so s = F + w (F - F) = F for a finite F; an infinite F gives inf - inf
    for value, want_nan in ((F32(-3.25), False), (F32(1e-42), False), (F32(np.inf), True)):
        _, s, c = np_sample([(0.3, 0.9, 0.0)], [[value]], (1, 1, 1), (0, 0, 0), (1, 1, 1), TRILINEAR)
        assert c[0] and (np.isnan(s[0, 0]) if want_nan else s[0, 0].view(U32) == value.view(U32))
    assert np_store(ADD, [F32(1.0)], [F32(2.0)], -0.25)[0] == F32(0.5) and np_store(SET, [F32(1.0)], [F32(2.0)], -0.25)[0] == F32(-0.5)
    assert np_store(SET, [F32(0)], [F32(3.0)], 2.0 ** -140).view(U32)[0] == 3 << 9                  # 3 * 2^-140 = 3 * 2^9 * 2^-149: a denormal, kept
    assert sample_plan(TRILINEAR, 16_777_216) == ("k_sample_trilinear", 4096, 1, 16) and sample_plan(NEAREST, 4097)[:2] == ("k_sample_nearest", 2)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------
MEMBERS = ["struct_size", "flags", "dims", "n_channels", "origin", "inv_cell", "mode", "scale", "channels", "field", "out_stats"]
CH_MEMBERS = ["attr", "comp", "op", "reserved"]


def test_ctypes_mirrors_header_and_integration_agree_on_the_structs_and_the_prototype(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd_sample.h"
    int main(void) {
        int (*fe)(HnbEffect*, const HnbSampleDesc*) = hnb_effect_sample;
        printf("%zu", sizeof(HnbSampleDesc));
    ''' + "\n".join(f'        printf(" %zu", offsetof(HnbSampleDesc, {m}));' for m in MEMBERS) + r'''
        printf(" %zu", sizeof(HnbSampleChannel));
    ''' + "\n".join(f'        printf(" %zu", offsetof(HnbSampleChannel, {m}));' for m in CH_MEMBERS) + r'''
        printf(" %u %u %u %u %u\n", HNB_SAMPLE_MAX_CHANNELS, HNB_SAMPLE_NEAREST, HNB_SAMPLE_TRILINEAR, HNB_SAMPLE_SET, HNB_SAMPLE_ADD);
        return fe == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    D, Ch = runtime.SampleDesc, runtime.SampleChannel
    assert got == [136, 0, 4, 8, 20, 24, 36, 48, 52, 56, 120, 128, 16, 0, 4, 8, 12, 4, 0, 1, 0, 1]
    assert [C.sizeof(D)] + [getattr(D, m).offset for m in MEMBERS] == got[:12]
    assert [C.sizeof(Ch)] + [getattr(Ch, m).offset for m in CH_MEMBERS] == got[12:17]
    assert (runtime.SAMPLE_MAX_CHANNELS, runtime.SAMPLE_NEAREST, runtime.SAMPLE_TRILINEAR, runtime.SAMPLE_SET, runtime.SAMPLE_ADD) == tuple(got[17:])
    d = runtime.sample_desc((4, 5, 6), (1, 2, 3), (0.5, 0.25, 2), 0x1000, [(A.VELOCITY.id, 2, ADD), (A.LIFETIME.id, 0, SET)], NEAREST, -0.25, 0x3000)
    assert (d.struct_size, d.flags, list(d.dims), d.n_channels, list(d.origin), list(d.inv_cell), d.mode, d.scale, d.field, d.out_stats) == (136, 0, [4, 5, 6], 2, [1, 2, 3], [0.5, 0.25, 2],
                                                                                                                                       0, -0.25, 0x1000, 0x3000)
    assert [(c.attr, c.comp, c.op, c.reserved) for c in d.channels] == [(A.VELOCITY.id, 2, 1, 0), (A.LIFETIME.id, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    d = runtime.sample_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 0x1000, [(A.VELOCITY.id, 0, ADD)])
    assert (d.mode, d.scale, d.n_channels, d.out_stats) == (1, 1.0, 1, None)
    lib = runtime.load_library()
    assert runtime.ABI_SAMPLE_SYMBOLS == ["hnb_effect_sample"]
    full = open(os.path.join(ROOT, "include", "hanabi_amd_sample.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(lib, "hnb_effect_sample") and lib.hnb_effect_sample.argtypes == [C.c_void_p, C.POINTER(runtime.SampleDesc)]
    m = re.search(r"int\s+hnb_effect_sample\s*\(([^)]*)\)\s*;", header)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["HnbEffect* fx", "const HnbSampleDesc* desc"]
    m = re.search(r"\bfn hnb_effect_sample\(([^)]*)\) -> c_int;", txt)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["fx: *mut HnbEffect", "desc: *const HnbSampleDesc"]
    assert list(inspect.signature(runtime.Effect.sample).parameters) == ["self", "dims", "origin", "inv_cell", "field_ptr", "channels", "mode", "scale", "stats_ptr"]
    assert not hasattr(runtime.Program, "sample")                          # (no program form: the header says why)
    # every header declares exactly its own symbols: hanabi_amd.h and its 61 are as they were, and the companion lists do not overlap
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header)) == set(runtime.ABI_SAMPLE_SYMBOLS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", main)) == set(runtime.ABI_SYMBOLS) and len(runtime.ABI_SYMBOLS) == 61
    for other in (runtime.ABI_SYMBOLS, runtime.ABI_BINNED_SYMBOLS, runtime.ABI_IMPORT_SYMBOLS, runtime.ABI_DEPOSIT_SYMBOLS):
        assert not set(runtime.ABI_SAMPLE_SYMBOLS) & set(other)
    assert '#include "hanabi_amd.h"' in full and '#include "hanabi_amd_binned.h"' in full
    bound = set(re.findall(r"pub fn (hnb_[a-z0-9_]+)\(", txt))
    assert not set(runtime.ABI_SAMPLE_SYMBOLS) & bound                    # (the `pub fn` set mirrors hanabi_amd.h and the host header: the sample sits in a module of its own)
    m = re.search(r"#\[repr\(C\)\]\s*pub struct HnbSampleDesc \{(.*?)\}", txt, flags=re.S)
    assert m, "INTEGRATION.md mirrors the struct"
    rust = [" ".join(line.split("//")[0].split()).rstrip(",") for line in m.group(1).splitlines() if line.split("//")[0].strip()]
    assert rust == ["pub struct_size: u32", "pub flags: u32", "pub dims: [u32; 3]", "pub n_channels: u32", "pub origin: [f32; 3]", "pub inv_cell: [f32; 3]", "pub mode: u32", "pub scale: f32",
                    "pub channels: [HnbSampleChannel; 4]", "pub field: *const f32", "pub out_stats: *mut u32"]
    m = re.search(r"#\[repr\(C\)\]\s*pub struct HnbSampleChannel \{(.*?)\}", txt, flags=re.S)
    assert m and [" ".join(line.split("//")[0].split()).rstrip(",") for line in m.group(1).splitlines() if line.split("//")[0].strip()] == [f"pub {n}: u32" for n in CH_MEMBERS]
    for word in ("OUTSIDE BIN", "u = t[c] - 0.5f", "lo[c] = max(j, 0)", "inf - inf", "which NaN is unspecified", "Out of scope: a program form", "f16 / bf16 fields", "per-channel scales",
                 "AGE", "the last row is never read"):
        assert word in full, word


def test_call_fails_loudly_on_null_arguments_and_without_a_device():
    """Up to the device check: the NULL refusals come before anything is dereferenced, loaded or enqueued. The refusals of a description's members
    need an effect, and an effect a device: the stand-alone program below holds them, and tests/test_gpu_sample.py on a live effect."""
    lib = runtime.load_library()
    d = runtime.sample_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 0x1000, [(A.VELOCITY.id, 0, ADD)])
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for args in ((None, C.byref(d)), (fake, None), (None, None)):
        assert lib.hnb_effect_sample(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to sample into, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------
def test_code_object_is_built_carried_and_has_its_two_kernels_without_scratch_or_spills():
    co = hb.sample_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_sample.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(SAMPLE_KERNELS), sorted(rows)
    for name, r in rows.items():
        assert r["group_segment_fixed_size"] == 0, f"{name}: {r['group_segment_fixed_size']} B of LDS per workgroup (the field is not staged)"
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["kernarg_segment_size"] == 168, (name, r)                # one SampleArgs by value
        assert r["vgpr_count"] <= 128, (name, r)                          # four waves per SIMD stay possible
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_sample_code)
    for h in ("hnb_sample.h", "hnb_bin_cell.h", "hnb_sort_key.h"):
        assert f'"{h}"' in inspect.getsource(hb.build_sample_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_sample.hip")).read()
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_sample.h")).read()
    assert hb.SAMPLE_CODE_OBJECTS == (hb.build_sample_code,)
    assert hb.EXPORT_CODE_OBJECTS == (hb.build_export_code, hb.build_export_sort_code, hb.build_export_filter_code, hb.build_export_cull_code, hb.build_export_filter_prog_code,
                                      hb.build_export_cull_prog_code)
    assert (hb.BINNED_CODE_OBJECTS, hb.IMPORT_CODE_OBJECTS, hb.QUERY_CODE_OBJECTS, hb.DEPOSIT_CODE_OBJECTS) == ((hb.build_export_bin_code,), (hb.build_import_code,), (hb.build_bounds_code,),
                                                                                                                (hb.build_deposit_code,))
    assert "SAMPLE_CODE_OBJECTS" in inspect.getsource(hb.build_runtime) and "hanabi_amd_sample.h" in inspect.getsource(hb.build_runtime)
    assert "hanabi_amd_sample.h" in inspect.getsource(hb._build_code_object)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_sample_code.inc" in ignored and "*.hsaco" in ignored
    for other in (hb.bounds_code_path(), hb.export_bin_code_path(), hb.import_code_path(), hb.deposit_code_path()):
        assert not set(_rows(other)) & set(SAMPLE_KERNELS)


# ---- csrc/hnb_sample.h as a stand-alone host program under the sanitizers ---------------------------------------------------------------------------
ERRORS = ["Ok", "ErrStructSize", "ErrFlags", "ErrMode", "ErrDims", "ErrOrigin", "ErrInvCell", "ErrChannelCount", "ErrAttr", "ErrComp", "ErrOp", "ErrChannelReserved", "ErrDuplicate",
          "ErrUnusedChannel", "ErrScale", "ErrField", "ErrStats", "ErrNoPosition"]
E = {n: i for i, n in enumerate(ERRORS)}
# what the check is given: (attr, ncomp, is_f32); layout 1 has no POSITION
LAYOUT = [(A.POSITION.id, 3, 1), (A.VELOCITY.id, 3, 1), (A.AGE.id, 1, 1), (A.LIFETIME.id, 1, 1), (A.COLOR.id, 1, 0), (A.HDR_COLOR.id, 4, 1), (A.SIZE2.id, 2, 1)]

HOST_SRC = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "hnb_sample.h"
using namespace hnb;
""" + "\n".join(f"static_assert(kSample{n} == {i}, \"SampleDescError\");" for i, n in enumerate(ERRORS)) + r"""
static_assert(kSampleDescErrorCount == """ + str(len(ERRORS)) + r""", "SampleDescError");
static_assert(sizeof(HnbSampleDesc) == 136 && sizeof(SampleArgs) == 168 && kSampleKNearest == 0 && kSampleKTrilinear == 1 && kSampleKernelCount == 2, "hnb_sample.h");
static_assert(kSampleTile == """ + str(TILE) + r""" && kSampleBlock == 256, "hnb_sample.h");
static const SampleLayoutAttr kLayout[] = {""" + ", ".join("{%d, %d, %d}" % l for l in LAYOUT) + r"""};
static float f_of(unsigned b) { float f; std::memcpy(&f, &b, 4); return f; }
static unsigned b_of(float f) { unsigned b; std::memcpy(&b, &f, 4); return b; }
int main() {
    char what[16];
    BinGrid g = {};
    std::vector<float> field;                 // exactly n_cells values on the heap: a corner row at or past n_cells is an error the sanitizer reports
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "names")) {
            for (uint32_t i = 0; i < kSampleKernelCount; ++i) std::printf("%u:%s ", kSampleKernelNames[i].kernel, kSampleKernelNames[i].name);
            std::printf("\n");
        } else if (!std::strcmp(what, "plan")) {
            unsigned mode, cap;
            if (std::scanf("%u %u", &mode, &cap) != 2) return 1;
            const SamplePlan pl = sample_launch_plan(mode, cap);
            if (pl.tiles != pl.grid_x) return 5;
            std::printf("%s %u %u %llu\n", pl.kernel < kSampleKernelCount ? kSampleKernelNames[pl.kernel].name : "?", pl.grid_x, pl.grid_y, (unsigned long long)pl.clear_stats_bytes);
        } else if (!std::strcmp(what, "grid")) {
            unsigned ob[3], ib[3];
            if (std::scanf("%u %u %u %x %x %x %x %x %x", &g.dims[0], &g.dims[1], &g.dims[2], &ob[0], &ob[1], &ob[2], &ib[0], &ib[1], &ib[2]) != 9) return 1;
            for (int c = 0; c < 3; ++c) { g.origin[c] = f_of(ob[c]); g.inv_cell[c] = f_of(ib[c]); }
            g.n_cells = bin_cell_count(g.dims);
            field.assign(g.n_cells, 0.0f);
            field.shrink_to_fit();
            for (uint32_t i = 0; i < g.n_cells; ++i) {
                unsigned b;
                if (std::scanf("%x", &b) != 1) return 1;
                field[i] = f_of(b);
            }
            std::printf("%u\n", g.n_cells);
        } else if (!std::strcmp(what, "s")) {     // one particle through the kernels' own functions, in the kernels' order
            unsigned mode, op, sb, pb[3], vb;
            if (std::scanf("%u %u %x %x %x %x %x", &mode, &op, &sb, &pb[0], &pb[1], &pb[2], &vb) != 7) return 1;
            const float x = f_of(pb[0]), y = f_of(pb[1]), z = f_of(pb[2]);
            const uint32_t cell = bin_cell_of(g, x, y, z);
            if (cell == g.n_cells) { std::printf("0 %x\n", vb); continue; }
            float s;
            if (mode == HNB_SAMPLE_NEAREST) s = field.at(cell);
            else {
                const SampleAxis ax = sample_axis(sample_axis_t(x, g.origin[0], g.inv_cell[0]), g.dims[0]);
                const SampleAxis ay = sample_axis(sample_axis_t(y, g.origin[1], g.inv_cell[1]), g.dims[1]);
                const SampleAxis az = sample_axis(sample_axis_t(z, g.origin[2], g.inv_cell[2]), g.dims[2]);
                uint32_t rows[8];
                sample_corner_rows(g.dims, ax, ay, az, rows);
                float c[8];
                for (int i = 0; i < 8; ++i) c[i] = field.at(rows[i]);
                s = sample_blend(c, ax.w, ay.w, az.w);
            }
            std::printf("1 %x\n", b_of(sample_store(op, f_of(vb), s, f_of(sb))));
        } else if (!std::strcmp(what, "desc")) {
            HnbSampleDesc d;
            std::memset(&d, 0, sizeof d);
            unsigned long long fld, stats; unsigned layout_first, ob[3], ib[3], sb;
            if (std::scanf("%u %u %u %u %u %u %u %x %x %x %x %x %x %u %x %llx %llx", &layout_first, &d.struct_size, &d.flags, &d.dims[0], &d.dims[1], &d.dims[2], &d.n_channels, &ob[0], &ob[1],
                           &ob[2], &ib[0], &ib[1], &ib[2], &d.mode, &sb, &fld, &stats) != 17) return 1;
            std::memcpy(d.origin, ob, 12); std::memcpy(d.inv_cell, ib, 12); d.scale = f_of(sb);
            d.field = (const float*)(uintptr_t)fld; d.out_stats = (uint32_t*)(uintptr_t)stats;
            for (unsigned k = 0; k < HNB_SAMPLE_MAX_CHANNELS; ++k)
                if (std::scanf("%u %u %u %u", &d.channels[k].attr, &d.channels[k].comp, &d.channels[k].op, &d.channels[k].reserved) != 4) return 1;
            if (layout_first > 1) return 1;
            const SampleCheck c = sample_check_desc(d, kLayout + layout_first, (uint32_t)(sizeof kLayout / sizeof *kLayout) - layout_first);
            if (c.error >= kSampleDescErrorCount || !sample_error_text(c.error)[1]) return 3;
            std::printf("%u %u %u %u", c.error, c.channel, c.n_cells, c.position_index);
            for (uint32_t k = 0; k < d.n_channels && k < HNB_SAMPLE_MAX_CHANNELS; ++k) std::printf(" %u", c.layout_index[k]);
            std::printf("\n");
        } else return 4;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """g++ alone, with the address and undefined-behaviour sanitizers and no contraction: the header is plain C++ on the host. The program has its
    own main and is run directly."""
    tmp = tmp_path_factory.mktemp("sample_host")
    (tmp / "smp.cpp").write_text(HOST_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), str(tmp / "smp.cpp"), "-o", str(tmp / "smp")])
    return str(tmp / "smp")


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()      # (a sanitizer report ends the program with an error)
    assert len(out) == len(lines)
    return out


def _f32(x):
    return int(np.array([x], F32).view(U32)[0])


def _desc_line(layout_first=0, struct_size=136, flags=0, dims=(4, 4, 4), n_channels=2, origin=(0.0, 0.0, 0.0), inv_cell=(1.0, 1.0, 1.0), mode=1, scale=1.0, field=0x1000, stats=0x3000,
               channels=((A.VELOCITY.id, 1, 1, 0), (A.HDR_COLOR.id, 3, 0, 0))):
    ch = list(channels) + [(0, 0, 0, 0)] * (4 - len(channels))
    return ("desc %d %d %d %d %d %d %d " % (layout_first, struct_size, flags, *dims, n_channels) + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell))
            + " %d %x %x %x " % (mode, _f32(scale), field, stats) + " ".join("%d %d %d %d" % c for c in ch))


def test_description_check_refuses_what_the_header_lists(host_exe):
    ask = lambda **kw: [int(x) for x in _ask(host_exe, [_desc_line(**kw)])[0].split()]
    assert ask() == [E["Ok"], 0, 64, 0, 1, 5]                                            # n_cells, POSITION's entry, the channels' entries
    assert ask(mode=0, stats=0, scale=-0.25)[0] == E["Ok"] and ask(scale=2.0 ** -140)[0] == E["Ok"] and ask(scale=0.0)[0] == E["Ok"]
    assert ask(dims=(1 << 24, 1, 1))[:3] == [E["Ok"], 0, 1 << 24]
    assert ask(n_channels=4, channels=((A.POSITION.id, 2, 0, 0), (A.VELOCITY.id, 0, 1, 0), (A.SIZE2.id, 1, 1, 0), (A.LIFETIME.id, 0, 0, 0))) == [E["Ok"], 0, 64, 0, 0, 1, 6, 3]
    assert ask(n_channels=3, channels=((A.VELOCITY.id, 0, 1, 0), (A.VELOCITY.id, 1, 1, 0), (A.VELOCITY.id, 2, 1, 0)))[0] == E["Ok"]      # one attribute, three components
    for size in (0, 132, 140):
        assert ask(struct_size=size)[0] == E["ErrStructSize"]
    for flags in (1, 2, 0x80000000):
        assert ask(flags=flags)[0] == E["ErrFlags"]
    for mode in (2, 3, 0xFFFFFFFF):
        assert ask(mode=mode)[0] == E["ErrMode"]
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), ((1 << 24) + 1, 1, 1), (4096, 4096, 2), (65536, 65536, 65536)):
        assert ask(dims=dims)[0] == E["ErrDims"], dims
    for axis in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            o = [0.0] * 3; o[axis] = bad
            assert ask(origin=o)[:2] == [E["ErrOrigin"], axis]
        for bad in (np.nan, np.inf, 0.0, -0.0, -1.0):
            i = [1.0] * 3; i[axis] = bad
            assert ask(inv_cell=i)[:2] == [E["ErrInvCell"], axis]
    assert ask(n_channels=5)[0] == E["ErrChannelCount"] and ask(n_channels=0, channels=())[0] == E["ErrChannelCount"]
    good = (A.VELOCITY.id, 1, 1, 0)
    for attr in (A.AGE.id, A.COLOR.id, A.SIZE3.id, A.ID.id, A.PARTICLE_COUNTER.id, 39, 9999):     # AGE; packed u32; not in the layout; not stored; no attribute
        assert ask(channels=(good, (attr, 0, 0, 0)))[:2] == [E["ErrAttr"], 1], attr
    for attr, comp in ((A.LIFETIME.id, 1), (A.POSITION.id, 3), (A.HDR_COLOR.id, 4), (A.SIZE2.id, 2), (A.LIFETIME.id, 0xFFFFFFFF)):
        assert ask(channels=((attr, comp, 0, 0), good))[:2] == [E["ErrComp"], 0]
    for op in (2, 3, 0xFFFFFFFF):
        assert ask(channels=(good, (A.LIFETIME.id, 0, op, 0)))[:2] == [E["ErrOp"], 1]
    assert ask(channels=(good, (A.LIFETIME.id, 0, 0, 1)))[:2] == [E["ErrChannelReserved"], 1]
    assert ask(channels=(good, (A.VELOCITY.id, 1, 0, 0)))[:2] == [E["ErrDuplicate"], 1]                                       # the same (attr, comp), whatever the op
    assert ask(n_channels=3, channels=((A.POSITION.id, 0, 0, 0), good, (A.POSITION.id, 0, 1, 0)))[:2] == [E["ErrDuplicate"], 2]
    for k, entry in ((2, (A.LIFETIME.id, 0, 0, 0)), (3, (0, 1, 0, 0)), (2, (0, 0, 1, 0)), (3, (0, 0, 0, 1))):
        ch = [good, (A.LIFETIME.id, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]; ch[k] = entry
        assert ask(channels=ch)[:2] == [E["ErrUnusedChannel"], k]
    assert ask(n_channels=1, channels=(good, (A.LIFETIME.id, 0, 0, 0)))[:2] == [E["ErrUnusedChannel"], 1]
    for bad in (np.nan, np.inf, -np.inf):
        assert ask(scale=bad)[0] == E["ErrScale"]
    for field in (0, 0x1004, 0x1008):
        assert ask(field=field)[0] == E["ErrField"]
    assert ask(stats=0x3004)[0] == E["ErrStats"] and ask(stats=0x3008)[0] == E["ErrStats"]
    assert ask(layout_first=1)[0] == E["ErrNoPosition"]


def test_launch_plan_is_its_restatement_over_every_capacity_edge(host_exe):
    assert _ask(host_exe, ["names"])[0].split() == [f"{i}:{n}" for i, n in enumerate(SAMPLE_KERNELS)]
    caps = [1, 2, 3, 4, 255, 256, 300, 4095, 4096, 4097, 8192, 3 * 4096 + 5, 300_007, 16_777_216, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 4096, 2 ** 32 - 4095, 2 ** 32 - 1]
    cases = [(mode, cap) for mode in (NEAREST, TRILINEAR) for cap in caps]
    for (mode, cap), line in zip(cases, _ask(host_exe, ["plan %d %d" % c for c in cases])):
        w = line.split()
        got = (w[0],) + tuple(int(x) for x in w[1:])
        assert got == sample_plan(mode, cap), (mode, cap, got)
        assert (got[1] - 1) * TILE < cap <= got[1] * TILE and got[2] == 1   # every slot belongs to one workgroup, and every workgroup has a slot
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## Sample" in design and design.index("## Deposit") < design.index("## Sample") < design.index("## Measurement (row d)")
    for word in ("`k_sample_nearest`", "`k_sample_trilinear`", "ceil(capacity / 4096)", "LDS"):
        assert word in design, word


# ---- the rule, through the kernels' own functions -----------------------------------------------------------------------------------------------------
RULE_GRIDS = [(1, 1, 1), (2, 1, 7), (5, 4, 3), (64, 64, 64)]
SCALES = [1.0, -0.25, 2.0 ** -140]


def axis_values(dim):
    """t along one axis of `dim` cells (origin 0, edge 1: t = p): -0, faces, centres, the values either side of 0.5 and dim - 0.5, the grid's two ends
    and their neighbours, a denormal, and what lands outside"""
    up, down = (lambda x: np.nextafter(F32(x), F32(np.inf))), (lambda x: np.nextafter(F32(x), F32(-np.inf)))
    v = [F32(-0.0), F32(0.0), F32(1e-45), F32(1e-30), F32(0.25), down(0.5), F32(0.5), up(0.5), down(dim - 0.5), F32(dim - 0.5), up(dim - 0.5), down(dim), F32(dim), up(dim),
         F32(-1e-45), F32(-1e-30), F32(np.nan), F32(np.inf), F32(-np.inf)]
    cells = sorted({0, 1, dim // 2, dim - 2, dim - 1} & set(range(dim)))
    for i in cells:
        v += [F32(i), F32(i + 0.5), down(i + 0.5), up(i + 0.5), F32(i + 0.75)]
        if i:
            v.append(down(i))
    return np.unique(np.array(v, F32).view(U32)).view(F32)


def rule_fields(dims, rng):
    """two fields of one channel: finite with denormals of both signs and zeros; the same with infinities and NaNs planted"""
    n = dims[0] * dims[1] * dims[2]
    f = rng.normal(0, 3, n).astype(F32)
    special = np.array([1e-40, -1e-45, 1e-38, -0.0, 0.0, 3e38, -3e38], F32)
    idx = rng.permutation(n)
    f[idx[: min(n, len(special))]] = special[: min(n, len(special))]
    g = f.copy()
    bad = np.array([np.inf, -np.inf, np.nan], F32)
    idx = rng.permutation(n)
    g[idx[: min(n, 3)]] = bad[: min(n, 3)]
    if n > 64:
        g[idx[3: n // 50]] = np.resize(bad, n // 50 - 3)
    return [f, g]


@pytest.mark.parametrize("dims", RULE_GRIDS, ids=["x".join(map(str, d)) for d in RULE_GRIDS])
def test_rule_under_the_sanitizers_is_the_numpy_restatement_bit_for_bit(host_exe, dims):
    rng = np.random.default_rng(dims[0] * 100 + dims[2])
    lat = [axis_values(d) for d in dims]
    # the lattice: every pair of axes at every edge value with the third at a few, then random points in and a little around an odd box
    picks = [l[rng.permutation(len(l))[:6]] for l in lat]
    pts = []
    for c in range(3):
        axes = [picks[0], picks[1], picks[2]]
        axes[c] = lat[c]
        axes[(c + 1) % 3] = lat[(c + 1) % 3]
        pts += list(itertools.product(*axes))
    lattice = np.unique(np.array(pts, F32).view(U32).reshape(-1, 3), axis=0).view(F32)
    if len(lattice) > 2500:
        lattice = lattice[rng.permutation(len(lattice))[:2500]]
    unit = (dims, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), lattice)
    origin = np.array([-1.5, 0.3, -7.25], F32)
    size = np.array([3.1, 0.7, 11.0], F32)
    inv_cell = (np.array(dims, F32) / size).astype(F32)
    cloud = (origin + size * rng.uniform(-0.05, 1.05, (1500, 3))).astype(F32)
    odd = (dims, origin, inv_cell, cloud)
    total = sampled = clamped_n = nan_n = denormal_n = 0
    for dims_, o, iv, pos in (unit, odd):
        for field in rule_fields(dims, rng):
            lines = ["grid %d %d %d " % tuple(dims) + " ".join("%x" % _f32(x) for x in tuple(o) + tuple(iv)) + " " + " ".join("%x" % b for b in field.view(U32))]
            want = []
            v = rng.normal(0, 2, len(pos)).astype(F32)
            v[::7] = F32(1e-41); v[3::11] = F32(-0.0)
            for mode in (NEAREST, TRILINEAR):
                inside, s, clamped = np_sample(pos, field[:, None], dims, o, iv, mode)
                for op in (SET, ADD):
                    for scale in SCALES:
                        out = np.where(inside, np_store(op, v, s[:, 0], scale), v).view(U32)
                        lines += ["s %d %d %x %x %x %x %x" % (mode, op, _f32(scale), *[int(b) for b in p], int(vb)) for p, vb in zip(pos.view(U32), v.view(U32))]
                        want.append((inside, out))
                        r = out.view(F32)[inside]
                        nan_n += int(np.isnan(r).sum())
                        denormal_n += int(((r != 0) & (np.abs(r) < F32(1.1754944e-38))).sum())
                sampled += int(inside.sum()); clamped_n += int(clamped.sum()); total += len(pos)
            got = _ask(host_exe, lines)
            assert int(got[0]) == dims[0] * dims[1] * dims[2]
            got = np.array([[int(x, 16) for x in g.split()] for g in got[1:]], np.uint64)
            want_in = np.concatenate([w[0] for w in want])
            want_bits = np.concatenate([w[1] for w in want])
            np.testing.assert_array_equal(got[:, 0].astype(bool), want_in, err_msg=f"{dims}: inside")
            ok = same_bits_or_both_nan(got[:, 1].astype(U32), want_bits)
            bad = np.flatnonzero(~ok)
            assert not len(bad), (dims, len(bad), [(lines[1 + i], hex(int(got[i, 1])), hex(int(want_bits[i]))) for i in bad[:6]])
    # the sweep holds what it is meant to: particles in and out, clamped corners, NaN results and denormal results
    assert 0 < sampled < total and clamped_n > 0 and nan_n > 0 and denormal_n > 0, (sampled, total, clamped_n, nan_n, denormal_n)
    if dims == (1, 1, 1):                                                  # every corner is cell 0: a finite field comes through as field[0] * scale, exactly
        f = F32(-2.75)
        line = ["grid 1 1 1 0 0 0 %x %x %x %x" % (_f32(1.0), _f32(1.0), _f32(1.0), _f32(f)), "s 1 0 %x %x %x %x 0" % (_f32(-0.25), _f32(0.3), _f32(0.99), _f32(0.0))]
        assert _ask(host_exe, line)[1] == "1 %x" % _f32(f * F32(-0.25))
