"""The program form of the sample (hnb_program_sample, include/hanabi_amd_sample_program.h) without a GPU: header, ctypes mirror and INTEGRATION.md
agree on the structure and the prototype, and the call fails loudly; the plain C++ of csrc/hnb_sample_program.h - the check of the outer description,
the launch plan, the reset ranges and the 64-bit field offset - compiled as a stand-alone host program under the address and undefined-behaviour
sanitizers gives what the restatements in Python give; the three kernels live in a code object of their own with no scratch, no spills and at most 64
bytes of fixed LDS. The restatements of the rule itself are tests/test_sample_abi.py's, which tests/test_gpu_sample_program.py applies per instance."""
import ctypes as C
import inspect
import itertools
import os
import re
import subprocess

import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import runtime
from test_export_filtered_abi import CSRC, _rows
from test_export_sorted_abi import A, LLVM, ROOT
from test_sample_abi import E as INNER, LAYOUT, NEAREST, SAMPLE_KERNELS, TILE, TRILINEAR, _f32, sample_plan

PROG_KERNELS = ["k_sample_prog_nearest", "k_sample_prog_trilinear", "k_sample_prog_reset"]
MAX_INSTANCES = 65535
MAX_CELLS = 1 << 24                              # HNB_BIN_MAX_CELLS
ARGS_BYTES = 216                                 # sizeof(SampleProgArgs)
MEMBERS = ["struct_size", "flags", "sample", "field_instance_stride", "out_instance_stats", "reserved"]


def reset_ranges(chunks, horizons):
    """sample_program_reset_ranges restated: what reset_plane_proofs(fx, false) clears of one slab -> (lmin_bytes, horizon_bytes)"""
    return 4 * chunks, (256 + 24 * chunks) if horizons else 0


def program_sample_plan(mode, n_inst, capacity, lmin_bytes, horizon_bytes):
    """sample_program_launch_plan restated -> (kernel, grid_x, grid_y, reset_grid_x, reset_grid_y, lmin_words, horizon_words, clear_stats_bytes,
    clear_instance_stats_bytes): the effect form's tiles times the instances; a reset lane per 4-byte word, 256 lanes per workgroup"""
    _, tiles, _, clear = sample_plan(mode, capacity)
    words = lmin_bytes // 4 + horizon_bytes // 4
    return (PROG_KERNELS[mode], tiles, n_inst, max(1, -(-words // 256)), n_inst, lmin_bytes // 4, horizon_bytes // 4, clear, 16 * n_inst)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_header_and_integration_agree_on_the_struct_and_the_prototype(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd_sample_program.h"
    int main(void) {
        int (*fp)(HnbProgram*, const HnbProgramSampleDesc*) = hnb_program_sample;
        int (*fe)(HnbEffect*, const HnbSampleDesc*) = hnb_effect_sample;          /* the program form's header brings the effect form's along */
        printf("%zu", sizeof(HnbProgramSampleDesc));
    ''' + "\n".join(f'        printf(" %zu", offsetof(HnbProgramSampleDesc, {m}));' for m in MEMBERS) + r'''
        printf(" %u %zu\n", HNB_PROGRAM_SAMPLE_MAX_INSTANCES, sizeof(HnbSampleDesc));
        return fp == 0 || fe == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    D = runtime.ProgramSampleDesc
    assert got == [168, 0, 4, 8, 144, 152, 160, MAX_INSTANCES, 136]
    assert [C.sizeof(D)] + [getattr(D, m).offset for m in MEMBERS] == got[:7] and runtime.PROGRAM_SAMPLE_MAX_INSTANCES == MAX_INSTANCES
    assert [n for n, _ in D._fields_] == MEMBERS and dict(D._fields_)["sample"] is runtime.SampleDesc
    d = runtime.program_sample_desc((4, 5, 6), (1, 2, 3), (0.5, 0.25, 2), 0x1000, [(A.VELOCITY.id, 2, 1), (A.LIFETIME.id, 0, 0)], NEAREST, -0.25, 0x3000, 240, 0x5000)
    assert (d.struct_size, d.flags, d.field_instance_stride, d.out_instance_stats, d.reserved) == (168, 0, 240, 0x5000, 0)
    s = d.sample
    assert (s.struct_size, s.flags, list(s.dims), s.n_channels, s.mode, s.scale, s.field, s.out_stats) == (136, 0, [4, 5, 6], 2, 0, -0.25, 0x1000, 0x3000)
    d = runtime.program_sample_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 0x1000, [(A.VELOCITY.id, 0, 1)])
    assert (d.sample.mode, d.sample.scale, d.sample.out_stats, d.field_instance_stride, d.out_instance_stats) == (1, 1.0, None, 0, None)
    lib = runtime.load_library()
    assert runtime.ABI_SAMPLE_PROGRAM_SYMBOLS == ["hnb_program_sample"]
    assert hasattr(lib, "hnb_program_sample") and lib.hnb_program_sample.argtypes == [C.c_void_p, C.POINTER(runtime.ProgramSampleDesc)]
    full = open(os.path.join(ROOT, "include", "hanabi_amd_sample_program.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"int\s+hnb_program_sample\s*\(([^)]*)\)\s*;", header)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["HnbProgram* prog", "const HnbProgramSampleDesc* desc"]
    m = re.search(r"\bfn hnb_program_sample\(([^)]*)\) -> c_int;", txt)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["prog: *mut HnbProgram", "desc: *const HnbProgramSampleDesc"]
    # the binding's method takes Effect.sample's arguments and the two the program form adds
    params = list(inspect.signature(runtime.Program.sample_all).parameters)
    assert params == list(inspect.signature(runtime.Effect.sample).parameters) + ["field_instance_stride", "instance_stats_ptr"]
    # every header declares exactly its own symbols: hanabi_amd.h and its 61 are as they were, the sample's header its one, and the seven lists do not overlap
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header)) == set(runtime.ABI_SAMPLE_PROGRAM_SYMBOLS)
    for h, own in (("hanabi_amd.h", runtime.ABI_SYMBOLS), ("hanabi_amd_sample.h", runtime.ABI_SAMPLE_SYMBOLS), ("hanabi_amd_splat.h", runtime.ABI_SPLAT_SYMBOLS)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", text)) == set(own), h
    assert len(runtime.ABI_SYMBOLS) == 61
    lists = [runtime.ABI_SYMBOLS, runtime.ABI_BINNED_SYMBOLS, runtime.ABI_IMPORT_SYMBOLS, runtime.ABI_DEPOSIT_SYMBOLS, runtime.ABI_SAMPLE_SYMBOLS, runtime.ABI_SPLAT_SYMBOLS,
             runtime.ABI_SAMPLE_PROGRAM_SYMBOLS]
    for a, b in itertools.combinations(lists, 2):
        assert not set(a) & set(b)
    assert '#include "hanabi_amd_sample.h"' in full and re.search(r"#define\s+HNB_PROGRAM_SAMPLE_MAX_INSTANCES\s+65535u", header)
    bound = set(re.findall(r"pub fn (hnb_[a-z0-9_]+)\(", txt))
    assert not set(runtime.ABI_SAMPLE_PROGRAM_SYMBOLS) & bound            # (the `pub fn` set mirrors hanabi_amd.h and the host header: the call sits in a module of its own)
    assert "pub mod sample_program" in txt
    m = re.search(r"#\[repr\(C\)\]\s*pub struct HnbProgramSampleDesc \{(.*?)\}", txt, flags=re.S)
    assert m, "INTEGRATION.md mirrors the struct"
    rust = [" ".join(line.split("//")[0].split()).rstrip(",") for line in m.group(1).splitlines() if line.split("//")[0].strip()]
    assert rust == ["pub struct_size: u32", "pub flags: u32", "pub sample: HnbSampleDesc", "pub field_instance_stride: u64", "pub out_instance_stats: *mut u32", "pub reserved: u64"]
    # the contract is stated by reference: the rule's arithmetic stays in the effect form's header, which still names the program form as out of its scope
    for word in ("hanabi_amd_sample.h", "bit for bit", "OUTSIDE BIN", "field_instance_stride == 0", "taken in 64 bits", "modulo 2^32", "does not depend on the instance count",
                 "per-instance grids or transforms", "AGE destinations", "an instance of 256 slots still takes a workgroup of its own"):
        assert word in full, word
    for word in ("u = t[c] - 0.5f", "lo[c] = max(j, 0)", "a00", "floorf"):
        assert word not in full, word
    assert "Out of scope: a program form" in open(os.path.join(ROOT, "include", "hanabi_amd_sample.h")).read()


def test_call_fails_loudly_on_null_arguments_and_without_a_device():
    """Up to the device check: the NULL refusals come before anything is dereferenced, loaded or enqueued. The refusals of a description's members
    need a program, and a program a device: the stand-alone program below holds them, and tests/test_gpu_sample_program.py on a live program."""
    lib = runtime.load_library()
    d = runtime.program_sample_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 0x1000, [(A.VELOCITY.id, 0, 1)])
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for args in ((None, C.byref(d)), (fake, None), (None, None)):
        assert lib.hnb_program_sample(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no program to sample into, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------
def test_code_object_is_built_carried_and_has_its_three_kernels_without_scratch_or_spills():
    co = hb.sample_prog_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_sample_prog.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(PROG_KERNELS), sorted(rows)
    for name, r in rows.items():
        assert r["group_segment_fixed_size"] <= 64, f"{name}: {r['group_segment_fixed_size']} B of fixed LDS per workgroup (the stats of four waves, nothing else)"
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["kernarg_segment_size"] == ARGS_BYTES, (name, r)        # one SampleProgArgs by value
        assert r["vgpr_count"] <= 128, (name, r)                          # four waves per SIMD stay possible
    assert rows["k_sample_prog_reset"]["group_segment_fixed_size"] == 0
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_sample_prog_code)
    for h in ("hnb_sample_program.h", "hnb_sample.h", "hnb_sample.hip.h", "hnb_bin_cell.h", "hnb_sort_key.h"):
        assert f'"{h}"' in inspect.getsource(hb.build_sample_prog_code)
    assert '"hnb_sample.hip.h"' in inspect.getsource(hb.build_sample_code)         # the effect form's unit is rebuilt when the shared text changes
    for f in ("hnb_sample_prog.hip", "hnb_sample.hip.h"):
        assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, f)).read()
    for f in ("hnb_sample_prog.hip", "hnb_sample.hip"):                    # both units take the tile from the one shared text
        text = open(os.path.join(CSRC, f)).read()
        assert '#include "hnb_sample.hip.h"' in text and "sample_tile_by_channels<MODE>" in text and "load_row" not in text
    assert hb.SAMPLE_PROGRAM_CODE_OBJECTS == (hb.build_sample_prog_code,) and hb.SAMPLE_CODE_OBJECTS == (hb.build_sample_code,)
    assert "SAMPLE_PROGRAM_CODE_OBJECTS" in inspect.getsource(hb.build_runtime) and "hanabi_amd_sample_program.h" in inspect.getsource(hb.build_runtime)
    assert "hanabi_amd_sample_program.h" in inspect.getsource(hb._build_code_object)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_sample_prog_code.inc" in ignored and "*.hsaco" in ignored
    others = (hb.export_code_path(), hb.export_sort_code_path(), hb.export_filter_code_path(), hb.export_cull_code_path(), hb.export_filter_prog_code_path(),
              hb.export_cull_prog_code_path(), hb.bounds_code_path(), hb.export_bin_code_path(), hb.import_code_path(), hb.deposit_code_path(), hb.sample_code_path(),
              hb.splat_code_path())
    for other in others:
        assert not set(_rows(other)) & set(PROG_KERNELS), other
    assert sorted(_rows(hb.sample_code_path())) == sorted(SAMPLE_KERNELS)  # the effect form's unit keeps exactly its two


# ---- csrc/hnb_sample_program.h as a stand-alone host program under the sanitizers -------------------------------------------------------------------
ERRORS = ["Ok", "ErrStructSize", "ErrFlags", "ErrReserved", "ErrInner", "ErrStride", "ErrInstanceStats", "ErrInstances"]
E = {n: i for i, n in enumerate(ERRORS)}

HOST_SRC = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "hnb_sample_program.h"
using namespace hnb;
""" + "\n".join(f"static_assert(kSampleProg{n} == {i}, \"SampleProgDescError\");" for i, n in enumerate(ERRORS)) + r"""
static_assert(kSampleProgDescErrorCount == """ + str(len(ERRORS)) + r""", "SampleProgDescError");
static_assert(sizeof(HnbProgramSampleDesc) == 168 && sizeof(SampleProgArgs) == """ + str(ARGS_BYTES) + r""" && kSampleProgKernelCount == 3 && kSampleProgLdsWords * 4 <= 64, "hnb_sample_program.h");
static_assert(kSampleProgKNearest == HNB_SAMPLE_NEAREST && kSampleProgKTrilinear == HNB_SAMPLE_TRILINEAR && kSampleProgKReset == 2, "a mode is its kernel's index");
static_assert(kSampleProgMaxInstances == """ + str(MAX_INSTANCES) + r""" && kSampleProgResetBlock == 256, "hnb_sample_program.h");
static const SampleLayoutAttr kLayout[] = {""" + ", ".join("{%d, %d, %d}" % l for l in LAYOUT) + r"""};
static float f_of(unsigned b) { float f; std::memcpy(&f, &b, 4); return f; }
int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "names")) {
            for (uint32_t i = 0; i < kSampleProgKernelCount; ++i) std::printf("%u:%s ", kSampleProgKernelNames[i].kernel, kSampleProgKernelNames[i].name);
            std::printf("\n");
        } else if (!std::strcmp(what, "plan")) {
            unsigned mode, n_inst, cap, chunks, hz;
            if (std::scanf("%u %u %u %u %u", &mode, &n_inst, &cap, &chunks, &hz) != 5) return 1;
            const SampleProgResetRanges rr = sample_program_reset_ranges(chunks, hz != 0);
            const SampleProgPlan pl = sample_program_launch_plan(mode, n_inst, cap, rr.lmin_bytes, rr.horizon_bytes);
            if (pl.tiles != pl.grid_x || pl.kernel >= kSampleProgKReset) return 5;
            std::printf("%llu %llu %s %u %u %u %u %u %u %llu %llu\n", (unsigned long long)rr.lmin_bytes, (unsigned long long)rr.horizon_bytes, kSampleProgKernelNames[pl.kernel].name,
                        pl.grid_x, pl.grid_y, pl.reset_grid_x, pl.reset_grid_y, pl.lmin_words, pl.horizon_words, (unsigned long long)pl.clear_stats_bytes,
                        (unsigned long long)pl.clear_instance_stats_bytes);
        } else if (!std::strcmp(what, "offset")) {
            unsigned i; unsigned long long stride;
            if (std::scanf("%u %llu", &i, &stride) != 2) return 1;
            std::printf("%llu\n", (unsigned long long)sample_program_field_offset(i, stride));
        } else if (!std::strcmp(what, "desc")) {
            HnbProgramSampleDesc o;
            std::memset(&o, 0, sizeof o);
            HnbSampleDesc& d = o.sample;
            unsigned long long stride, inst_stats, reserved, fld, stats; unsigned n_inst, layout_first, ob[3], ib[3], sb;
            if (std::scanf("%u %u %u %llu %llx %llu", &n_inst, &o.struct_size, &o.flags, &stride, &inst_stats, &reserved) != 6) return 1;
            o.field_instance_stride = stride; o.out_instance_stats = (uint32_t*)(uintptr_t)inst_stats; o.reserved = reserved;
            if (std::scanf("%u %u %u %u %u %u %u %x %x %x %x %x %x %u %x %llx %llx", &layout_first, &d.struct_size, &d.flags, &d.dims[0], &d.dims[1], &d.dims[2], &d.n_channels, &ob[0], &ob[1],
                           &ob[2], &ib[0], &ib[1], &ib[2], &d.mode, &sb, &fld, &stats) != 17) return 1;
            std::memcpy(d.origin, ob, 12); std::memcpy(d.inv_cell, ib, 12); d.scale = f_of(sb);
            d.field = (const float*)(uintptr_t)fld; d.out_stats = (uint32_t*)(uintptr_t)stats;
            for (unsigned k = 0; k < HNB_SAMPLE_MAX_CHANNELS; ++k)
                if (std::scanf("%u %u %u %u", &d.channels[k].attr, &d.channels[k].comp, &d.channels[k].op, &d.channels[k].reserved) != 4) return 1;
            if (layout_first > 1) return 1;
            const SampleProgCheck c = sample_program_check_desc(o, kLayout + layout_first, (uint32_t)(sizeof kLayout / sizeof *kLayout) - layout_first, n_inst);
            if (c.error >= kSampleProgDescErrorCount || !sample_program_error_text(c.error)[1]) return 3;
            if ((c.error == kSampleProgErrInner) != (c.inner.error != kSampleOk)) return 6;      // the inner refusals are delegated, and reported as the inner check reports them
            std::printf("%u %u %u %u\n", c.error, c.inner.error, c.inner.channel, c.inner.n_cells);
        } else return 4;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """g++ alone, with the address and undefined-behaviour sanitizers and no contraction: the header is plain C++ on the host. The program has its
    own main and is run directly."""
    tmp = tmp_path_factory.mktemp("sample_program_host")
    (tmp / "smp.cpp").write_text(HOST_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), str(tmp / "smp.cpp"), "-o", str(tmp / "smp")])
    return str(tmp / "smp")


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()      # (a sanitizer report ends the program with an error)
    assert len(out) == len(lines)
    return out


def _desc_line(n_inst=5, outer_size=168, outer_flags=0, stride=0, inst_stats=0x5000, reserved=0, layout_first=0, struct_size=136, flags=0, dims=(4, 4, 4), n_channels=2,
               origin=(0.0, 0.0, 0.0), inv_cell=(1.0, 1.0, 1.0), mode=1, scale=1.0, field=0x1000, stats=0x3000, channels=((A.VELOCITY.id, 1, 1, 0), (A.HDR_COLOR.id, 3, 0, 0))):
    ch = list(channels) + [(0, 0, 0, 0)] * (4 - len(channels))
    return ("desc %d %d %d %d %x %d " % (n_inst, outer_size, outer_flags, stride, inst_stats, reserved) + "%d %d %d %d %d %d %d " % (layout_first, struct_size, flags, *dims, n_channels)
            + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell)) + " %d %x %x %x " % (mode, _f32(scale), field, stats) + " ".join("%d %d %d %d" % c for c in ch))


def test_description_check_refuses_what_the_header_lists_in_its_order(host_exe):
    ask = lambda **kw: [int(x) for x in _ask(host_exe, [_desc_line(**kw)])[0].split()]
    assert ask() == [E["Ok"], 0, 0, 64]
    assert ask(stride=128)[0] == E["Ok"] and ask(stride=132)[0] == E["Ok"] and ask(stride=1 << 40)[0] == E["Ok"]      # n_cells * n_channels = 128: exactly, padded, far apart
    assert ask(inst_stats=0, stats=0)[0] == E["Ok"] and ask(n_inst=1)[0] == E["Ok"] and ask(n_inst=MAX_INSTANCES)[0] == E["Ok"]
    assert ask(dims=(MAX_CELLS, 1, 1), n_channels=4, channels=((A.POSITION.id, 2, 0, 0), (A.VELOCITY.id, 0, 1, 0), (A.SIZE2.id, 1, 1, 0), (A.LIFETIME.id, 0, 0, 0)),
               stride=4 * MAX_CELLS) == [E["Ok"], 0, 0, MAX_CELLS]
    # every outer refusal ...
    for size in (0, 136, 164, 172):
        assert ask(outer_size=size)[0] == E["ErrStructSize"]
    for flags in (1, 2, 0x80000000):
        assert ask(outer_flags=flags)[0] == E["ErrFlags"]
    for reserved in (1, 1 << 32, (1 << 64) - 1):
        assert ask(reserved=reserved)[0] == E["ErrReserved"]
    for stride in (1, 2, 3, 4, 64, 124, 127, 129, 130, 131, (1 << 40) + 2):       # not a multiple of 4, or below the 128 words of an instance's field
        assert ask(stride=stride)[0] == E["ErrStride"], stride
    assert ask(dims=(MAX_CELLS, 1, 1), stride=2 * MAX_CELLS - 4)[0] == E["ErrStride"] and ask(dims=(MAX_CELLS, 1, 1), stride=2 * MAX_CELLS)[0] == E["Ok"]
    for p in (0x5004, 0x5008, 0x500C, 0x5001):
        assert ask(inst_stats=p)[0] == E["ErrInstanceStats"]
    for n in (0, MAX_INSTANCES + 1, 1 << 20, (1 << 32) - 1):
        assert ask(n_inst=n)[0] == E["ErrInstances"]
    # ... in the order the header lists them: each one with every later one planted behind it
    later = [("outer_size", 164), ("outer_flags", 1), ("reserved", 1), ("flags", 1), ("stride", 2), ("inst_stats", 0x5004), ("n_inst", 0)]
    first = ["ErrStructSize", "ErrFlags", "ErrReserved", "ErrInner", "ErrStride", "ErrInstanceStats", "ErrInstances"]
    for i in range(len(later)):
        assert ask(**dict(later[i:]))[0] == E[first[i]], first[i]
    # every inner refusal, reached through the outer check and reported with the inner check's number and channel
    inner = lambda **kw: ask(**kw)[:3]
    good = (A.VELOCITY.id, 1, 1, 0)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(struct_size=132), "ErrStructSize", 0), (dict(struct_size=168), "ErrStructSize", 0), (dict(flags=1), "ErrFlags", 0), (dict(mode=2), "ErrMode", 0),
             (dict(dims=(0, 4, 4)), "ErrDims", 0), (dict(dims=(4096, 4096, 2)), "ErrDims", 0), (dict(origin=(0.0, nan, 0.0)), "ErrOrigin", 1), (dict(inv_cell=(1.0, 1.0, 0.0)), "ErrInvCell", 2),
             (dict(inv_cell=(inf, 1.0, 1.0)), "ErrInvCell", 0), (dict(n_channels=0, channels=()), "ErrChannelCount", 0), (dict(n_channels=5), "ErrChannelCount", 0),
             (dict(channels=(good, (A.AGE.id, 0, 0, 0))), "ErrAttr", 1), (dict(channels=(good, (A.COLOR.id, 0, 0, 0))), "ErrAttr", 1), (dict(channels=((A.LIFETIME.id, 1, 0, 0), good)), "ErrComp", 0),
             (dict(channels=(good, (A.LIFETIME.id, 0, 2, 0))), "ErrOp", 1), (dict(channels=(good, (A.LIFETIME.id, 0, 0, 1))), "ErrChannelReserved", 1),
             (dict(channels=(good, (A.VELOCITY.id, 1, 0, 0))), "ErrDuplicate", 1), (dict(channels=(good, (A.LIFETIME.id, 0, 0, 0), (0, 0, 1, 0))), "ErrUnusedChannel", 2),
             (dict(scale=nan), "ErrScale", 0), (dict(scale=-inf), "ErrScale", 0), (dict(field=0), "ErrField", 0), (dict(field=0x1008), "ErrField", 0), (dict(stats=0x3004), "ErrStats", 0),
             (dict(layout_first=1), "ErrNoPosition", 0)]
    assert {name for _, name, _ in cases} == set(INNER) - {"Ok"}          # every refusal sample_check_desc has
    for kw, name, channel in cases:
        assert inner(**kw) == [E["ErrInner"], INNER[name], channel], (kw, name)
        assert inner(stride=2, inst_stats=0x5004, n_inst=0, **kw)[:2] == [E["ErrInner"], INNER[name]]      # ... before the outer refusals behind it


def test_launch_plan_and_reset_ranges_are_their_restatements_over_every_edge(host_exe):
    assert _ask(host_exe, ["names"])[0].split() == [f"{i}:{n}" for i, n in enumerate(PROG_KERNELS)]
    assert not set(PROG_KERNELS) & set(SAMPLE_KERNELS)
    caps = [1, 2, 3, 4, 255, 256, 300, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 5, 65_536, 300_007, 16_777_216, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 4096, 2 ** 32 - 4095, 2 ** 32 - 1]
    cases = [(mode, n, cap, chunks, hz) for mode in (NEAREST, TRILINEAR) for n in (1, 2, MAX_INSTANCES) for cap in caps for chunks, hz in ((1, 0), (2, 1), (4097, 1))]
    cases += [(TRILINEAR, 512, 65_536, chunks, hz) for chunks in (1, 2, 4097) for hz in (0, 1)]
    for (mode, n, cap, chunks, hz), line in zip(cases, _ask(host_exe, ["plan %d %d %d %d %d" % c for c in cases])):
        w = line.split()
        lmin, horizon = reset_ranges(chunks, hz)
        assert (int(w[0]), int(w[1])) == (lmin, horizon), (chunks, hz, w[:2])
        got = (w[2],) + tuple(int(x) for x in w[3:])
        assert got == program_sample_plan(mode, n, cap, lmin, horizon), (mode, n, cap, chunks, hz, got)
        assert (got[1] - 1) * TILE < cap <= got[1] * TILE and got[2] == got[4] == n <= MAX_INSTANCES       # every slot of every instance belongs to one workgroup
        words = got[5] + got[6]
        assert (got[3] - 1) * 256 < words <= got[3] * 256                 # every word of both ranges belongs to one lane, and every workgroup has a word
    # what reset_plane_proofs(fx, false) clears, worked by hand: 4 bytes per chunk; 256 bytes and 24 per chunk when the horizons are kept
    assert reset_ranges(1, False) == (4, 0) and reset_ranges(2, True) == (8, 304) and reset_ranges(4097, True) == (16388, 98584) and reset_ranges(4097, False) == (16388, 0)
    assert program_sample_plan(TRILINEAR, 512, 65_536, 64, 640) == ("k_sample_prog_trilinear", 16, 512, 1, 512, 16, 160, 16, 8192)
    assert program_sample_plan(NEAREST, 3, 4097, *reset_ranges(4097, True))[3] == -(-(4097 + 64 + 6 * 4097) // 256)
    src = open(os.path.join(CSRC, "hanabi_amd.hip")).read()               # the ranges restate these two lines of reset_plane_proofs
    assert "p->dev.horizon_off, 0, 256 + (size_t)p->dev.chunks_per_inst * 24, st)" in src and "p->dev.lmin_off, 0, (size_t)p->dev.chunks_per_inst * 4, st)" in src
    # 65,536 instances are refused by the check, not planned
    assert int(_ask(host_exe, [_desc_line(n_inst=65_536)])[0].split()[0]) == E["ErrInstances"]


def test_field_offset_of_an_instance_is_taken_in_64_bits(host_exe):
    cases = [(0, 0), (1, 0), (65_534, 0), (1, 128), (65_534, 4 * MAX_CELLS), (65_534, 4 * MAX_CELLS + 4), (2, 1 << 40), (65_534, 1 << 32)]
    got = [int(x) for x in _ask(host_exe, ["offset %d %d" % c for c in cases])]
    assert got == [i * s for i, s in cases]
    assert got[4] == 65_534 << 26 and got[4] >= 1 << 41                    # far past 2^32 elements: a product in 32 bits would wrap
    text = open(os.path.join(CSRC, "hnb_sample_prog.hip")).read()
    assert "a.field + sample_program_field_offset(i, a.field_stride)" in text   # the kernels take the instance's field through this function


def test_design_names_the_kernels_and_the_effect_forms_scope_no_longer_excludes_it():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    first = design.index("## Sample (`hnb_effect_sample`)")
    assert first < design.index("## Splat") < design.index("## Sample, program form (`hnb_program_sample`)") < design.index("## Measurement (row d)")
    for word in ["`" + k + "`" for k in PROG_KERNELS] + ["(tiles, n_inst)", "one barrier", "reset_plane_proofs"]:
        assert word in design, word
    sample = design[first: design.index("## Splat")]
    scope = [l for l in sample.splitlines() if "Out of scope" in l or "out of scope" in l]
    assert scope and not any("a program form" in l for l in scope)
