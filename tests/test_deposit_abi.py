"""The deposit (hnb_effect_deposit / hnb_program_deposit, include/hanabi_amd_deposit.h) without a GPU: header, ctypes mirrors and INTEGRATION.md agree
on the structures and the prototypes, and the calls fail loudly; the plain C++ of csrc/hnb_deposit.h - the quantisation of a stored f32, the check of
a description and the launch plan - compiled as a stand-alone host program under the address and undefined-behaviour sanitizers gives what the
restatements in numpy / Python give, bit for bit; the two kernels live in a code object of their own with no scratch and no spills. The
restatements here (np_quantise, np_deposit, deposit_plan) are what tests/test_gpu_deposit.py expects and chooses its shapes by."""
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
from test_export_binned_abi import np_cells
from test_export_filtered_abi import CSRC, EDGE_BITS, _rows, _standalone
from test_export_sorted_abi import A, LLVM, ROOT

DEPOSIT_KERNELS = ["k_deposit_lds", "k_deposit_global"]
LDS_BUDGET, SPAN_BYTES, TILE = 48 * 1024, 2048, 4096
BIN_MAX_CELLS = 1 << 24
F32 = np.float32


# ---- the semantics, restated in numpy ---------------------------------------------------------------------------------------------------------------
def np_quantise(bits, frac_bits):
    """bits: stored f32 words -> (ok [n] bool, q [n] int64; 0 where rejected). binary64 holds v * 2^s exactly (24 significant bits, exponents
    -149 + 0 .. 127 + 32), so the product does not round and rint is the round-half-even of the exact value."""
    with np.errstate(all="ignore"):
        v = np.asarray(bits, np.uint32).view(F32).astype(np.float64)
        d = v * 2.0 ** int(frac_bits)
        ok = np.isfinite(d) & (np.abs(d) < 2.0 ** 62)
        q = np.rint(np.where(ok, d, 0.0)).astype(np.int64)
    return ok, q


def np_deposit(pos, alive, dims, origin, inv_cell, sources=(), fracs=()):
    """pos: [slots, 3] f32, alive: [slots] bool, sources: per channel the [slots] stored words of its component, fracs: its frac_bits
    -> (count [n_cells + 1] uint32, sums [n_cells + 1, k] int64 (modulo 2^64), stats [4] uint32)"""
    alive = np.asarray(alive, bool)
    n_cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    cells = np_cells(np.asarray(pos, F32)[alive], dims, origin, inv_cell).astype(np.int64)
    count = np.bincount(cells, minlength=n_cells + 1).astype(np.uint64)
    sums = np.zeros((n_cells + 1, len(sources)), np.uint64)
    rejected = 0
    for k, (src, s) in enumerate(zip(sources, fracs)):
        ok, q = np_quantise(np.asarray(src, np.uint32)[alive], s)
        np.add.at(sums[:, k], cells[ok], q[ok].view(np.uint64))           # unsigned adds wrap: the two's-complement sum modulo 2^64
        rejected += int((~ok).sum())
    stats = np.array([len(cells), int((cells == n_cells).sum()), rejected, 0], np.uint64)
    return (count & 0xFFFFFFFF).astype(np.uint32), sums.view(np.int64), (stats & 0xFFFFFFFF).astype(np.uint32)


def table_bytes(n_cells, n_channels):
    return (n_cells + 1) * (4 + 8 * n_channels)


def deposit_plan(program, n_inst, capacity, n_cells, n_channels):
    """deposit_launch_plan restated -> (kernel, grid_x, grid_y, span, lds_bytes, clear_count_bytes, clear_sums_bytes, clear_stats_bytes). DESIGN.md
    "Deposit": a table within the LDS budget is accumulated by a workgroup per span of ceil(table / 2048) tiles, a larger one per tile in memory."""
    table = table_bytes(n_cells, n_channels)
    tiles = max(1, -(-capacity // TILE))
    inst = n_inst if program else 1
    clear = ((n_cells + 1) * 4, (n_cells + 1) * 8 * n_channels, 16)
    if table <= LDS_BUDGET:
        span = -(-table // SPAN_BYTES)
        return ("k_deposit_lds", -(-tiles // span), inst, span, table) + clear
    return ("k_deposit_global", tiles, inst, 1, 0) + clear


def last_lds_cells(n_channels):
    """the largest n_cells whose table is still within the budget"""
    return LDS_BUDGET // (4 + 8 * n_channels) - 1


def test_the_restatement_itself_on_a_case_worked_by_hand():
    f = lambda *x: np.array(x, F32).view(np.uint32)
    # frac_bits 1: halves. 0.25 -> 0.5 ties to 0; 0.75 -> 1.5 ties to 2; 1.25 -> 2.5 ties to 2; -1.25 -> -2; 3.0 -> 6; -0.0 -> 0
    ok, q = np_quantise(f(0.25, 0.75, 1.25, -1.25, 3.0, -0.0, np.nan, np.inf, -np.inf), 1)
    assert list(ok) == [True] * 6 + [False] * 3 and list(q) == [0, 2, 2, -2, 6, 0, 0, 0, 0]
    ok, q = np_quantise(f(2.0 ** 61, 2.0 ** 62, -(2.0 ** 62), 2.0 ** 62 * (1 - 2.0 ** -24)), 0)           # the bound is exclusive on both sides
    assert list(ok) == [True, False, False, True] and list(q[[0, 3]]) == [2 ** 61, 2 ** 62 - 2 ** 38]
    ok, q = np_quantise(f(2.0 ** 29, 2.0 ** 30), 32)
    assert list(ok) == [True, False] and q[0] == 2 ** 61
    assert list(np_quantise(np.array([1, 0x80000001], np.uint32), 32)[1]) == [0, 0]                         # denormals: 2^-149 * 2^32 rounds to 0
    # two cells of edge 1 along x from 0, and the outside bin; slot 2 is dead; slot 3's source is a NaN: counted, not summed, rejected
    pos = np.array([(0.5, 0, 0), (1.5, 0, 0), (0.5, 0, 0), (1.0, 0, 0), (2.0, 0, 0), (np.nan, 0, 0)], F32)
    alive = [True, True, False, True, True, True]
    src = f(1.5, -2.5, 100.0, np.nan, 0.5, -7.0)
    count, sums, stats = np_deposit(pos, alive, (2, 1, 1), (0, 0, 0), (1, 1, 1), [src, src], [0, 2])
    assert list(count) == [1, 2, 2] and sums.tolist() == [[2, 6], [-2, -10], [-7, -26]] and list(stats) == [5, 2, 2, 0]      # 1.5 -> 2, -2.5 -> -2, 0.5 -> 0: ties to even
    # four values whose sum wraps past 2^63: the sum is modulo 2^64
    big = f(2.0 ** 61, 2.0 ** 61, 2.0 ** 61, 2.0 ** 61)
    _, sums, _ = np_deposit(np.zeros((4, 3), F32), [True] * 4, (1, 1, 1), (-1, -1, -1), (0.5, 0.5, 0.5), [big], [0])
    assert sums.tolist() == [[-2 ** 63], [0]]
    assert deposit_plan(False, 1, 16_777_216, 512, 1) == ("k_deposit_lds", 1024, 1, 4, 6156, 2052, 4104, 16)
    assert deposit_plan(True, 7, 300, 64 ** 3, 1)[:5] == ("k_deposit_global", 1, 7, 1, 0)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------
MEMBERS = ["struct_size", "flags", "dims", "n_channels", "origin", "inv_cell", "channels", "count", "sums", "out_stats"]
CH_MEMBERS = ["attr", "comp", "frac_bits", "reserved"]


def test_ctypes_mirrors_header_and_integration_agree_on_the_structs_and_the_prototypes(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd_deposit.h"
    int main(void) {
        int (*fe)(HnbEffect*, const HnbDepositDesc*) = hnb_effect_deposit;
        int (*fp)(HnbProgram*, const HnbDepositDesc*) = hnb_program_deposit;
        printf("%zu", sizeof(HnbDepositDesc));
    ''' + "\n".join(f'        printf(" %zu", offsetof(HnbDepositDesc, {m}));' for m in MEMBERS) + r'''
        printf(" %zu", sizeof(HnbDepositChannel));
    ''' + "\n".join(f'        printf(" %zu", offsetof(HnbDepositChannel, {m}));' for m in CH_MEMBERS) + r'''
        printf(" %u %u\n", HNB_DEPOSIT_MAX_CHANNELS, HNB_DEPOSIT_ACCUMULATE);
        return fe == 0 || fp == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    D, Ch = runtime.DepositDesc, runtime.DepositChannel
    assert got == [136, 0, 4, 8, 20, 24, 36, 48, 112, 120, 128, 16, 0, 4, 8, 12, 4, 1]
    assert [C.sizeof(D)] + [getattr(D, m).offset for m in MEMBERS] == got[:11]
    assert [C.sizeof(Ch)] + [getattr(Ch, m).offset for m in CH_MEMBERS] == got[11:16]
    assert (runtime.DEPOSIT_MAX_CHANNELS, runtime.DEPOSIT_ACCUMULATE) == tuple(got[16:])
    d = runtime.deposit_desc((4, 5, 6), (1, 2, 3), (0.5, 0.25, 2), 0x1000, [(A.AGE.id, 0, 16), (A.VELOCITY.id, 2, 8)], 0x2000, 0x3000, accumulate=True)
    assert (d.struct_size, d.flags, list(d.dims), d.n_channels, list(d.origin), list(d.inv_cell), d.count, d.sums, d.out_stats) == (136, 1, [4, 5, 6], 2, [1, 2, 3], [0.5, 0.25, 2], 0x1000,
                                                                                                                                  0x2000, 0x3000)
    assert [(c.attr, c.comp, c.frac_bits, c.reserved) for c in d.channels] == [(A.AGE.id, 0, 16, 0), (A.VELOCITY.id, 2, 8, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    d = runtime.deposit_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 0x1000)
    assert (d.flags, d.n_channels, d.sums, d.out_stats) == (0, 0, None, None)
    lib = runtime.load_library()
    assert runtime.ABI_DEPOSIT_SYMBOLS == ["hnb_effect_deposit", "hnb_program_deposit"]
    full = open(os.path.join(ROOT, "include", "hanabi_amd_deposit.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, handle, rust in (("hnb_effect_deposit", "HnbEffect* fx", "fx: *mut HnbEffect"), ("hnb_program_deposit", "HnbProgram* prog", "prog: *mut HnbProgram")):
        assert hasattr(lib, name) and getattr(lib, name).argtypes == [C.c_void_p, C.POINTER(runtime.DepositDesc)]
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == [handle, "const HnbDepositDesc* desc"], name
        m = re.search(r"\bfn " + name + r"\(([^)]*)\) -> c_int;", txt)
        assert m and [a.strip() for a in m.group(1).split(",")] == [rust, "desc: *const HnbDepositDesc"], name
    params = ["self", "dims", "origin", "inv_cell", "count_ptr", "channels", "sums_ptr", "stats_ptr", "accumulate"]
    assert list(inspect.signature(runtime.Effect.deposit).parameters) == params == list(inspect.signature(runtime.Program.deposit).parameters)
    # every header declares exactly its own symbols: hanabi_amd.h and its 61 are as they were
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header)) == set(runtime.ABI_DEPOSIT_SYMBOLS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", main)) == set(runtime.ABI_SYMBOLS) and len(runtime.ABI_SYMBOLS) == 61 and not set(runtime.ABI_DEPOSIT_SYMBOLS) & set(runtime.ABI_SYMBOLS)
    bound = set(re.findall(r"pub fn (hnb_[a-z0-9_]+)\(", txt))
    assert not set(runtime.ABI_DEPOSIT_SYMBOLS) & bound                   # (the `pub fn` set mirrors hanabi_amd.h and the host header: the deposit sits in a module of its own)
    m = re.search(r"#\[repr\(C\)\]\s*pub struct HnbDepositDesc \{(.*?)\}", txt, flags=re.S)
    assert m, "INTEGRATION.md mirrors the struct"
    rust = [" ".join(line.split("//")[0].split()).rstrip(",") for line in m.group(1).splitlines() if line.split("//")[0].strip()]
    assert rust == ["pub struct_size: u32", "pub flags: u32", "pub dims: [u32; 3]", "pub n_channels: u32", "pub origin: [f32; 3]", "pub inv_cell: [f32; 3]",
                    "pub channels: [HnbDepositChannel; 4]", "pub count: *mut u32", "pub sums: *mut i64", "pub out_stats: *mut u32"]
    m = re.search(r"#\[repr\(C\)\]\s*pub struct HnbDepositChannel \{(.*?)\}", txt, flags=re.S)
    assert m and [" ".join(line.split("//")[0].split()).rstrip(",") for line in m.group(1).splitlines() if line.split("//")[0].strip()] == [f"pub {n}: u32" for n in CH_MEMBERS]
    assert "sums.to(torch.float32) * 2.0**-frac_bits" in txt and "sums.to(torch.float32) * 2.0**-frac_bits" in full
    for word in ("OUTSIDE BIN", "ties to even", "modulo 2^64", "no scratch at all", "HNB_DEPOSIT_ACCUMULATE the call first clears", "multi-cell (trilinear) splats"):
        assert word in full, word


def test_calls_fail_loudly_on_null_arguments_and_without_a_device():
    """Up to the device check: the NULL refusals come before anything is dereferenced, loaded or enqueued. The refusals of a description's members
    need an effect, and an effect a device: the stand-alone program below holds them, and tests/test_gpu_deposit.py on a live effect."""
    lib = runtime.load_library()
    d = runtime.deposit_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 0x1000)
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for call in (lib.hnb_effect_deposit, lib.hnb_program_deposit):
        for args in ((None, C.byref(d)), (fake, None), (None, None)):
            assert call(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to deposit, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------
def test_code_object_is_built_carried_and_has_its_two_kernels_without_scratch_or_spills():
    co = hb.deposit_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_deposit.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(DEPOSIT_KERNELS), sorted(rows)
    for name, r in rows.items():
        # the table of k_deposit_lds is dynamic LDS sized by the plan (at most the budget: the plan's sweep below); the fixed part is small
        assert r["group_segment_fixed_size"] <= 64, f"{name}: {r['group_segment_fixed_size']} B of fixed LDS per workgroup"
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["kernarg_segment_size"] == 184, (name, r)                # one DepositArgs by value
        assert r["vgpr_count"] <= 64, (name, r)                           # eight waves per SIMD stay possible
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_deposit_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_deposit.hip")).read()
    assert hb.DEPOSIT_CODE_OBJECTS == (hb.build_deposit_code,) and hb.build_deposit_code not in hb.EXPORT_CODE_OBJECTS + hb.QUERY_CODE_OBJECTS
    assert "DEPOSIT_CODE_OBJECTS" in inspect.getsource(hb.build_runtime) and "hanabi_amd_deposit.h" in inspect.getsource(hb.build_runtime)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_deposit_code.inc" in ignored and "*.hsaco" in ignored
    for other in (hb.bounds_code_path(), hb.export_bin_code_path(), hb.import_code_path()):
        assert not set(_rows(other)) & set(DEPOSIT_KERNELS)


# ---- csrc/hnb_deposit.h as a stand-alone host program under the sanitizers ------------------------------------------------------------------------------
ERRORS = ["Ok", "ErrStructSize", "ErrFlags", "ErrDims", "ErrOrigin", "ErrInvCell", "ErrChannelCount", "ErrAttr", "ErrComp", "ErrFracBits", "ErrChannelReserved", "ErrUnusedChannel",
          "ErrCount", "ErrSums", "ErrStats", "ErrNoPosition"]
E = {n: i for i, n in enumerate(ERRORS)}
# what the check is given: (attr, ncomp, is_f32); layout 1 has no POSITION
LAYOUT = [(A.POSITION.id, 3, 1), (A.VELOCITY.id, 3, 1), (A.AGE.id, 1, 1), (A.LIFETIME.id, 1, 1), (A.COLOR.id, 1, 0), (A.HDR_COLOR.id, 4, 1), (A.SIZE2.id, 2, 1)]

HOST_SRC = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "hnb_deposit.h"
using namespace hnb;
""" + "\n".join(f"static_assert(kDeposit{n} == {i}, \"DepositDescError\");" for i, n in enumerate(ERRORS)) + r"""
static_assert(kDepositDescErrorCount == """ + str(len(ERRORS)) + r""", "DepositDescError");
static_assert(sizeof(HnbDepositDesc) == 136 && sizeof(DepositArgs) == 184 && kDepositKLds == 0 && kDepositKGlobal == 1 && kDepositKernelCount == 2, "hnb_deposit.h");
static_assert(kDepositLdsBudget == """ + str(LDS_BUDGET) + " && kDepositSpanBytes == " + str(SPAN_BYTES) + " && kDepositTile == " + str(TILE) + r""" && kDepositBlock == 256, "hnb_deposit.h");
static_assert(kDepositLdsBudget >= 32 * 1024 && kDepositLdsBudget <= 64 * 1024, "two workgroups fit a CU");
static const DepositLayoutAttr kLayout[] = {""" + ", ".join("{%d, %d, %d}" % l for l in LAYOUT) + r"""};
int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "names")) {
            for (uint32_t i = 0; i < kDepositKernelCount; ++i) std::printf("%u:%s ", kDepositKernelNames[i].kernel, kDepositKernelNames[i].name);
            std::printf("\n");
        } else if (!std::strcmp(what, "q")) {
            unsigned bits, frac;
            if (std::scanf("%x %u", &bits, &frac) != 2) return 1;
            const DepositQuant r = deposit_quantise(bits, frac);
            std::printf("%d %lld\n", r.ok ? 1 : 0, (long long)r.q);
        } else if (!std::strcmp(what, "plan")) {
            unsigned program, n_inst, cap, n_cells, nch;
            if (std::scanf("%u %u %u %u %u", &program, &n_inst, &cap, &n_cells, &nch) != 5) return 1;
            const DepositPlan pl = deposit_launch_plan(program != 0, n_inst, cap, n_cells, nch);
            std::printf("%s %u %u %u %u %llu %llu %llu\n", pl.kernel < kDepositKernelCount ? kDepositKernelNames[pl.kernel].name : "?", pl.grid_x, pl.grid_y, pl.span, pl.lds_bytes,
                        (unsigned long long)pl.clear_count_bytes, (unsigned long long)pl.clear_sums_bytes, (unsigned long long)pl.clear_stats_bytes);
        } else if (!std::strcmp(what, "desc")) {
            HnbDepositDesc d;
            std::memset(&d, 0, sizeof d);
            unsigned long long count, sums, stats; unsigned layout_first, ob[3], ib[3];
            if (std::scanf("%u %u %u %u %u %u %u %x %x %x %x %x %x %llx %llx %llx", &layout_first, &d.struct_size, &d.flags, &d.dims[0], &d.dims[1], &d.dims[2], &d.n_channels, &ob[0], &ob[1],
                           &ob[2], &ib[0], &ib[1], &ib[2], &count, &sums, &stats) != 16) return 1;
            std::memcpy(d.origin, ob, 12); std::memcpy(d.inv_cell, ib, 12);
            d.count = (uint32_t*)(uintptr_t)count; d.sums = (int64_t*)(uintptr_t)sums; d.out_stats = (uint32_t*)(uintptr_t)stats;
            for (unsigned k = 0; k < HNB_DEPOSIT_MAX_CHANNELS; ++k)
                if (std::scanf("%u %u %u %u", &d.channels[k].attr, &d.channels[k].comp, &d.channels[k].frac_bits, &d.channels[k].reserved) != 4) return 1;
            if (layout_first > 1) return 1;
            const DepositCheck c = deposit_check_desc(d, kLayout + layout_first, (uint32_t)(sizeof kLayout / sizeof *kLayout) - layout_first);
            if (c.error >= kDepositDescErrorCount || !deposit_error_text(c.error)[1]) return 3;
            std::printf("%u %u %u %u %d", c.error, c.channel, c.n_cells, c.position_index, c.has_age ? 1 : 0);
            for (uint32_t k = 0; k < d.n_channels && k < HNB_DEPOSIT_MAX_CHANNELS; ++k) std::printf(" %u", c.layout_index[k]);
            std::printf("\n");
        } else return 4;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return _standalone(tmp_path_factory.mktemp("deposit_host"), "dep", HOST_SRC)


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()      # (a sanitizer report ends the program with an error)
    assert len(out) == len(lines)
    return out


def _f32(x):
    return int(np.array([x], F32).view(np.uint32)[0])


def _desc_line(layout_first=0, struct_size=136, flags=0, dims=(4, 4, 4), n_channels=2, origin=(0.0, 0.0, 0.0), inv_cell=(1.0, 1.0, 1.0), count=0x1000, sums=0x2000, stats=0x3000,
               channels=((A.AGE.id, 0, 16, 0), (A.HDR_COLOR.id, 3, 32, 0))):
    ch = list(channels) + [(0, 0, 0, 0)] * (4 - len(channels))
    return ("desc %d %d %d %d %d %d %d " % (layout_first, struct_size, flags, *dims, n_channels) + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell))
            + " %x %x %x " % (count, sums, stats) + " ".join("%d %d %d %d" % c for c in ch))


def test_description_check_refuses_what_the_header_lists(host_exe):
    ask = lambda **kw: [int(x) for x in _ask(host_exe, [_desc_line(**kw)])[0].split()]
    assert ask() == [E["Ok"], 0, 64, 0, 1, 2, 5]                                         # n_cells, POSITION's entry, AGE is read, the channels' entries
    assert ask(n_channels=0, channels=(), sums=0, stats=0)[:5] == [E["Ok"], 0, 64, 0, 0]      # no channel, no sums, no stats
    assert ask(flags=1)[0] == E["Ok"] and ask(dims=(1 << 24, 1, 1))[:3] == [E["Ok"], 0, 1 << 24]
    assert ask(n_channels=4, channels=((A.POSITION.id, 2, 0, 0), (A.VELOCITY.id, 0, 32, 0), (A.SIZE2.id, 1, 7, 0), (A.LIFETIME.id, 0, 1, 0))) == [E["Ok"], 0, 64, 0, 0, 0, 1, 6, 3]
    for size in (0, 132, 140):
        assert ask(struct_size=size)[0] == E["ErrStructSize"]
    for flags in (2, 3, 0x80000000):
        assert ask(flags=flags)[0] == E["ErrFlags"]
    for dims in ((0, 4, 4), (4, 0, 4), (4, 4, 0), ((1 << 24) + 1, 1, 1), (4096, 4096, 2), (65536, 65536, 65536)):
        assert ask(dims=dims)[0] == E["ErrDims"], dims
    for axis in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            o = [0.0] * 3; o[axis] = bad
            assert ask(origin=o)[:2] == [E["ErrOrigin"], axis]
        for bad in (np.nan, np.inf, 0.0, -0.0, -1.0):
            i = [1.0] * 3; i[axis] = bad
            assert ask(inv_cell=i)[:2] == [E["ErrInvCell"], axis]
    assert ask(n_channels=5)[0] == E["ErrChannelCount"]
    good = (A.AGE.id, 0, 16, 0)
    for attr in (A.COLOR.id, A.SIZE3.id, A.ID.id, A.PARTICLE_COUNTER.id, 39, 9999):      # packed u32; not in the layout; not stored; no attribute
        assert ask(channels=(good, (attr, 0, 0, 0)))[:2] == [E["ErrAttr"], 1], attr
    for attr, comp in ((A.AGE.id, 1), (A.POSITION.id, 3), (A.HDR_COLOR.id, 4), (A.SIZE2.id, 2), (A.AGE.id, 0xFFFFFFFF)):
        assert ask(channels=((attr, comp, 0, 0), good))[:2] == [E["ErrComp"], 0]
    assert ask(channels=(good, (A.AGE.id, 0, 33, 0)))[:2] == [E["ErrFracBits"], 1] and ask(channels=(good, (A.AGE.id, 0, 32, 0)))[0] == E["Ok"]
    assert ask(channels=(good, (A.AGE.id, 0, 0, 1)))[:2] == [E["ErrChannelReserved"], 1]
    for k, entry in ((2, (A.AGE.id, 0, 0, 0)), (3, (0, 1, 0, 0)), (2, (0, 0, 1, 0)), (3, (0, 0, 0, 1))):
        ch = [good, good, (0, 0, 0, 0), (0, 0, 0, 0)]; ch[k] = entry
        assert ask(channels=ch)[:2] == [E["ErrUnusedChannel"], k]
    assert ask(n_channels=1, channels=(good, good))[:2] == [E["ErrUnusedChannel"], 1]
    for count in (0, 0x1004, 0x1008):
        assert ask(count=count)[0] == E["ErrCount"]
    assert ask(sums=0)[0] == E["ErrSums"] and ask(sums=0x2008)[0] == E["ErrSums"] and ask(n_channels=0, channels=())[0] == E["ErrSums"]      # missing; misaligned; given without channels
    assert ask(stats=0x3004)[0] == E["ErrStats"] and ask(stats=0)[0] == E["Ok"]
    assert ask(layout_first=1)[0] == E["ErrNoPosition"]


def quantise_inputs():
    bits = list(EDGE_BITS)
    for e in range(256):                                                     # every exponent: the least, the middle and the greatest significand
        for frac in (0, 1, 0x400000, 0x7FFFFF):
            bits.append((e << 23) | frac)
    for x in list(range(0, 9)) + [2 ** 22 - 1, 2 ** 22, 2 ** 23 - 2, 2 ** 23 - 1]:    # the ties x.5 for even and odd x (exact in binary32 below 2^23), and their neighbours
        for v in (x + 0.5, np.nextafter(F32(x + 0.5), F32(0)), np.nextafter(F32(x + 0.5), F32(1e9))):
            bits.append(_f32(v))
    bits = np.array(bits, np.uint32)
    return np.unique(np.concatenate([bits, bits | np.uint32(0x80000000)]))             # both signs


def test_quantisation_under_the_sanitizers_is_the_numpy_restatement_bit_for_bit(host_exe):
    assert _ask(host_exe, ["names"])[0].split() == [f"{i}:{n}" for i, n in enumerate(DEPOSIT_KERNELS)]
    bits = quantise_inputs()
    assert len(bits) > 2000
    lines, want = [], []
    for s in range(33):
        ok, q = np_quantise(bits, s)
        lines += ["q %x %d" % (int(b), s) for b in bits]
        want += ["%d %d" % (int(o), int(v)) for o, v in zip(ok, q)]
    got = _ask(host_exe, lines)
    bad = [(lines[i], got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])
    rejected = sum(w.startswith("0") for w in want)
    assert 0 < rejected < len(want) // 2 and any(w.startswith("1 -") for w in want)    # the sweep holds rejected, accepted and negative contributions
    # ties by hand through the compiled function: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -3.5 -> -4 at frac_bits 0; the same values a bit lower at frac_bits 1
    ask = lambda v, s: _ask(host_exe, ["q %x %d" % (_f32(v), s)])[0]
    assert [ask(v, 0) for v in (0.5, 1.5, 2.5, -3.5)] == ["1 0", "1 2", "1 2", "1 -4"] == [ask(v / 2, 1) for v in (0.5, 1.5, 2.5, -3.5)]
    assert ask(2.0 ** 62, 0) == "0 0" and ask(2.0 ** 30, 32) == "0 0" and ask(-(2.0 ** 61), 0) == "1 %d" % -(2 ** 61) and ask(2.0 ** 29, 32) == "1 %d" % 2 ** 61


def test_launch_plan_is_its_restatement_and_the_designs_rule(host_exe):
    caps = (1, 255, 4096, 4097, 3 * 4096 + 5, 300_007, 16_777_216, 2 ** 32 - 1)
    cells = {1, 64, 512, 1364, 1365, 4095, 4096, 12287, 12288, 64 ** 3, BIN_MAX_CELLS}
    for k in range(5):
        cells |= {last_lds_cells(k), last_lds_cells(k) + 1}
    cases = [(program, n, cap, nc, k) for cap in caps for nc in sorted(cells) for k in range(5) for program, n in ((0, 1), (1, 1), (1, 300), (1, 65_535))]
    out = _ask(host_exe, ["plan %d %d %d %d %d" % c for c in cases])
    for case, line in zip(cases, out):
        w = line.split()
        got = (w[0],) + tuple(int(x) for x in w[1:])
        assert got == deposit_plan(*case), (case, got)
        kernel, gx, gy, span, lds = got[:5]
        program, n, cap, nc, k = case
        tiles = -(-cap // TILE)
        assert (kernel == "k_deposit_lds") == (table_bytes(nc, k) <= LDS_BUDGET) and lds <= LDS_BUDGET and gy == (n if program else 1)
        assert gx >= 1 and gx * span >= tiles > (gx - 1) * span          # every tile belongs to one workgroup, and every workgroup has one
        if kernel == "k_deposit_lds":                                   # the span grows with the table: 2048 bytes of table per tile at most
            assert lds == table_bytes(nc, k) and 1 <= span <= 24 and (span - 1) * SPAN_BYTES < lds <= span * SPAN_BYTES
    for k in range(5):                                                  # the last table on the LDS path and the first off it
        n = last_lds_cells(k)
        assert table_bytes(n, k) <= LDS_BUDGET < table_bytes(n + 1, k)
        assert deposit_plan(False, 1, 10_000, n, k)[0] == "k_deposit_lds" and deposit_plan(False, 1, 10_000, n + 1, k)[0] == "k_deposit_global"
    assert [last_lds_cells(k) for k in range(5)] == [12287, 4095, 2456, 1754, 1364]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## Deposit" in design
    for word in ("`k_deposit_lds`", "`k_deposit_global`", "ceil(table / 2048)", "48 KiB"):
        assert word in design, word
