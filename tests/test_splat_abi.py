"""The splat (hnb_effect_splat / hnb_program_splat, include/hanabi_amd_splat.h) without a GPU: header, ctypes and INTEGRATION.md agree on the prototypes,
and the calls fail loudly; the plain C++ of csrc/hnb_splat.h - the rule the kernels call, the check of a description and the launch plan - compiled as a
stand-alone host program under the address and undefined-behaviour sanitizers gives what the restatements in numpy / Python give, bit for bit; the two
kernels live in a code object of their own with no scratch and no spills. The restatement here (np_splat) is what tests/test_gpu_splat.py expects."""
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
from test_deposit_abi import BIN_MAX_CELLS, LDS_BUDGET, SPAN_BYTES, TILE, deposit_plan, last_lds_cells, np_deposit, np_quantise, table_bytes
from test_export_binned_abi import np_cells
from test_export_filtered_abi import CSRC, _rows
from test_export_sorted_abi import A, LLVM, ROOT
from test_sample_abi import axis_values, np_axis

SPLAT_KERNELS = ["k_splat_lds", "k_splat_global"]
ONE = 0xFFFFFFFF                                 # HNB_SPLAT_ATTR_ONE
ONE_BITS = 0x3F800000                            # its stored value: the bits of 1.0f
F32, U32 = np.float32, np.uint32


# ---- the semantics, restated in numpy: binary32 arrays, one operation per statement ---------------------------------------------------------------
def one_source(n):
    """the source of a channel of HNB_SPLAT_ATTR_ONE over n slots: 1.0f everywhere"""
    return np.full(n, ONE_BITS, U32)


def np_splat_parts(pos, dims, origin, inv_cell):
    """pos: [n, 3] binary32 -> (cells [n] int64: the deposit's; inside [n] bool; rows [m, 8] int64 and W [m, 8] binary32 of the m inside particles, corner
    i = a + 2 b + 4 c with lo (0) or hi (1) along x (a), y (b), z (c); clamped [m] bool: a corner is clamped on some axis)"""
    pos = np.asarray(pos, F32).reshape(-1, 3)
    dims = [int(d) for d in dims]
    origin, inv_cell = np.asarray(origin, F32), np.asarray(inv_cell, F32)
    cells = np_cells(pos, dims, origin, inv_cell).astype(np.int64)
    inside = cells != dims[0] * dims[1] * dims[2]
    p = pos[inside]
    idx, w, clamped = [], [], np.zeros(len(p), bool)
    with np.errstate(all="ignore"):
        for c in range(3):
            d = p[:, c] - origin[c]
            t = d * inv_cell[c]
            assert d.dtype == F32 and t.dtype == F32
            lo, hi, w1, cl = np_axis(t, dims[c])
            w0 = F32(1.0) - w1
            assert w0.dtype == F32 and w1.dtype == F32
            assert ((w0 >= 0) & (w0 <= 1) & (w1 >= 0) & (w1 <= 1)).all() and (lo >= 0).all() and (hi <= dims[c] - 1).all()
            idx.append((lo, hi)); w.append((w0, w1)); clamped |= cl
        rows, W = np.zeros((len(p), 8), np.int64), np.zeros((len(p), 8), F32)
        for i in range(8):
            a, b, c = i & 1, (i >> 1) & 1, i >> 2
            rows[:, i] = (idx[2][c] * dims[1] + idx[1][b]) * dims[0] + idx[0][a]
            xy = w[0][a] * w[1][b]
            assert xy.dtype == F32
            W[:, i] = xy * w[2][c]
    return cells, inside, rows, W, clamped


def np_corner_q(v_bits, W, frac_bits):
    """v_bits: [m] stored words, W: [m, 8] -> (ok [m, 8], q [m, 8] int64, cv [m, 8] binary32): cv = v * W, one rounded product, quantised as a stored value"""
    with np.errstate(all="ignore"):
        cv = np.asarray(v_bits, U32).view(F32)[:, None] * W
    assert cv.dtype == F32
    ok, q = np_quantise(np.ascontiguousarray(cv).view(U32), frac_bits)
    return ok, q, cv


def np_splat(pos, alive, dims, origin, inv_cell, sources=(), fracs=()):
    """pos: [slots, 3] f32, alive: [slots] bool, sources: per channel the [slots] stored words of its component (one_source for HNB_SPLAT_ATTR_ONE),
    fracs: its frac_bits -> (count [n_cells + 1] uint32, sums [n_cells + 1, k] int64 (modulo 2^64), stats [4] uint32)"""
    alive = np.asarray(alive, bool)
    n_cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    cells, inside, rows, W, _ = np_splat_parts(np.asarray(pos, F32).reshape(-1, 3)[alive], dims, origin, inv_cell)
    count = np.bincount(cells, minlength=n_cells + 1).astype(np.uint64)
    sums = np.zeros((n_cells + 1, len(sources)), np.uint64)
    rejected = 0
    for k, (src, s) in enumerate(zip(sources, fracs)):
        v = np.asarray(src, U32)[alive]
        ok, q = np_quantise(v, s)                                          # the acceptance: once, on the stored value
        out = ok & ~inside
        np.add.at(sums[:, k], cells[out], q[out].view(np.uint64))          # an outside particle: the deposit's contribution into row n_cells
        okc, qc, _ = np_corner_q(v[inside], W, s)
        acc = ok[inside]
        assert okc[acc].all(), "a corner of an accepted value is rejected"
        for i in range(8):                                                 # unsigned adds wrap: the two's-complement sum modulo 2^64
            np.add.at(sums[:, k], rows[acc, i], qc[acc, i].view(np.uint64))
        rejected += int((~ok).sum())
    stats = np.array([len(cells), int((~inside).sum()), rejected, 0], np.uint64)
    return (count & 0xFFFFFFFF).astype(np.uint32), sums.view(np.int64), (stats & 0xFFFFFFFF).astype(np.uint32)


def splat_plan(program, n_inst, capacity, n_cells, n_channels):
    """splat_launch_plan restated: the deposit's decision (test_deposit_abi.deposit_plan) with the splat's kernels"""
    p = deposit_plan(program, n_inst, capacity, n_cells, n_channels)
    return ({"k_deposit_lds": "k_splat_lds", "k_deposit_global": "k_splat_global"}[p[0]],) + p[1:]


def test_the_restatement_itself_on_cases_worked_by_hand():
    f = lambda *x: np.array(x, F32).view(U32)
    # a cell centre of 4 x 4 x 4 (edge 1 from 0): u = (1, 2, 0), every w1 = 0, so corner 0 has W = 1 and the seven others W = 0: everything in its own cell
    cell = (0 * 4 + 2) * 4 + 1
    count, sums, stats = np_splat([(1.5, 2.5, 0.5)], [True], (4, 4, 4), (0, 0, 0), (1, 1, 1), [f(-2.75), one_source(1)], [4, 30])
    assert count[cell] == 1 and count.sum() == 1 and list(stats) == [1, 0, 0, 0]
    want = np.zeros((65, 2), np.int64); want[cell] = (-44, 2 ** 30)
    np.testing.assert_array_equal(sums, want)
    # the middle of 2 x 2 x 2: every W = 1/8, eight different rows: 2^frac / 8 in each; the count is the particle's own cell alone
    count, sums, _ = np_splat([(1.0, 1.0, 1.0)], [True], (2, 2, 2), (0, 0, 0), (1, 1, 1), [one_source(1), f(3.0)], [4, 3])
    assert count.tolist() == [0] * 7 + [1, 0] and sums.tolist() == [[2, 3]] * 8 + [[0, 0]]
    # 1 x 1 x 1: every corner is cell 0. w = (0.25, 0.75) x (0.75, 0.25) x (1, 0): dyadic, the products are exact and sum to 1
    count, sums, _ = np_splat([(0.25, 0.75, 0.5)], [True], (1, 1, 1), (0, 0, 0), (1, 1, 1), [one_source(1), f(-1.0)], [8, 4])
    assert count.tolist() == [1, 0] and sums.tolist() == [[256, -16], [0, 0]]
    _, _, rows, W, clamped = np_splat_parts([(0.25, 0.75, 0.5)], (1, 1, 1), (0, 0, 0), (1, 1, 1))
    assert not rows.any() and clamped[0] and W[0].tolist() == [0.1875, 0.5625, 0.0625, 0.1875, 0, 0, 0, 0]
    # a tiny negative u: t one ulp below 0.5 gives u = -2^-25, fl = -1, w1 = 1 - 2^-25 which rounds to 1.0, w0 = 0: followed as written, both corners are cell 0
    t = np.nextafter(F32(0.5), F32(0))
    _, _, rows, W, clamped = np_splat_parts([(t, 0.5, 0.5)], (4, 4, 4), (0, 0, 0), (1, 1, 1))
    assert W[0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and rows[0, :2].tolist() == [0, 0] and clamped[0]
    # outside: the deposit's contribution into row n_cells; a rejected value counts once and adds nothing, its particle's count and other channel stay
    pos = np.array([(0.5, 0, 0), (5.0, 0, 0), (np.nan, 0, 0), (1.0, 0.5, 0.5), (1.0, 0.5, 0.5)], F32)
    src = f(1.5, -2.5, 7.0, np.inf, 100.0)
    count, sums, stats = np_splat(pos, [True, True, True, True, False], (2, 1, 1), (0, 0, 0), (1, 1, 1), [src, one_source(5)], [1, 2])
    ref = np_deposit(pos, [True, True, True, True, False], (2, 1, 1), (0, 0, 0), (1, 1, 1), [src, one_source(5)], [1, 2])
    np.testing.assert_array_equal(count, ref[0]); np.testing.assert_array_equal(sums[2], ref[1][2])
    assert count.tolist() == [1, 1, 2] and list(stats) == [4, 2, 1, 0] and sums[2].tolist() == [-5 + 14, 8]
    # (0.5, 0, 0): x on the first centre; along y and z t = 0, u = -0.5, w = (0.5, 0.5) and both corners are cell 0 (one cell): four corners of W = 1/4 in cell 0.
    # The rounding is per corner: 1.5 * 0.25 * 2 = 0.75 -> 1, four times: 4, not round(1.5 * 2) = 3; ONE at 2^2: 4 times 1.
    # (1.0, 0.5, 0.5): u = 0.5 along x, half each into cells 0 and 1: 2 and 2 of ONE; its other channel is an infinity: rejected, nothing added
    assert sums[0].tolist() == [4, 4 + 2] and sums[1].tolist() == [0, 2]
    assert splat_plan(False, 1, 16_777_216, 512, 1) == ("k_splat_lds", 1024, 1, 4, 6156, 2052, 4104, 16)
    assert splat_plan(True, 7, 300, 64 ** 3, 1)[:5] == ("k_splat_global", 1, 7, 1, 0)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------
def test_header_ctypes_and_integration_agree_on_the_prototypes(tmp_path):
    src = r'''
    #include <stdio.h>
    #include "hanabi_amd_splat.h"
    int main(void) {
        int (*fe)(HnbEffect*, const HnbDepositDesc*) = hnb_effect_splat;
        int (*fp)(HnbProgram*, const HnbDepositDesc*) = hnb_program_splat;
        int (*de)(HnbEffect*, const HnbDepositDesc*) = hnb_effect_deposit;      /* the splat's header brings the deposit's description along */
        printf("%zu %u %u %u\n", sizeof(HnbDepositDesc), HNB_SPLAT_ATTR_ONE, HNB_DEPOSIT_MAX_CHANNELS, HNB_DEPOSIT_ACCUMULATE);
        return fe == 0 || fp == 0 || de == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [136, ONE, 4, 1] and runtime.SPLAT_ATTR_ONE == ONE
    lib = runtime.load_library()
    assert runtime.ABI_SPLAT_SYMBOLS == ["hnb_effect_splat", "hnb_program_splat"]
    full = open(os.path.join(ROOT, "include", "hanabi_amd_splat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, handle, rust in (("hnb_effect_splat", "HnbEffect* fx", "fx: *mut HnbEffect"), ("hnb_program_splat", "HnbProgram* prog", "prog: *mut HnbProgram")):
        assert hasattr(lib, name) and getattr(lib, name).argtypes == [C.c_void_p, C.POINTER(runtime.DepositDesc)]
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == [handle, "const HnbDepositDesc* desc"], name
        m = re.search(r"\bfn " + name + r"\(([^)]*)\) -> c_int;", txt)
        assert m and [a.strip() for a in m.group(1).split(",")] == [rust, "desc: *const HnbDepositDesc"], name
    params = list(inspect.signature(runtime.Effect.deposit).parameters)
    assert list(inspect.signature(runtime.Effect.splat).parameters) == params == list(inspect.signature(runtime.Program.splat).parameters)
    # every header declares exactly its own symbols, and the lists do not overlap: hanabi_amd.h and its 61 are as they were
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header)) == set(runtime.ABI_SPLAT_SYMBOLS)
    assert '#include "hanabi_amd_deposit.h"' in full and re.search(r"#define\s+HNB_SPLAT_ATTR_ONE\s+0xFFFFFFFFu", header)
    for h, own in (("hanabi_amd.h", runtime.ABI_SYMBOLS), ("hanabi_amd_deposit.h", runtime.ABI_DEPOSIT_SYMBOLS), ("hanabi_amd_sample.h", runtime.ABI_SAMPLE_SYMBOLS)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", text)) == set(own), h
    assert len(runtime.ABI_SYMBOLS) == 61
    lists = [runtime.ABI_SYMBOLS, runtime.ABI_BINNED_SYMBOLS, runtime.ABI_IMPORT_SYMBOLS, runtime.ABI_DEPOSIT_SYMBOLS, runtime.ABI_SAMPLE_SYMBOLS, runtime.ABI_SPLAT_SYMBOLS]
    for a, b in itertools.combinations(lists, 2):
        assert not set(a) & set(b)
    bound = set(re.findall(r"pub fn (hnb_[a-z0-9_]+)\(", txt))
    assert not set(runtime.ABI_SPLAT_SYMBOLS) & bound                     # (the `pub fn` set mirrors hanabi_amd.h and the host header: the splat sits in a module of its own)
    assert "pub mod splat" in txt and "HNB_SPLAT_ATTR_ONE: u32 = 0xFFFF_FFFF" in txt
    for word in ("OUTSIDE BIN", "u = t[c] - 0.5f", "w0[c] = 1.0f - w1[c]", "W = (w_a[0] * w_b[1]) * w_c[2]", "cv = v * W", "|cv| <= |v|", "eight\n *   accepted corners",
                 "2^-33", "keeps or flushes f32 denormals", "OWN cell", "modulo 2^64", "HNB_SPLAT_ATTR_ONE with comp != 0", "wave-level combining of equal rows"):
        assert word in full, word
    # the deposit's header still names the splat as out of its scope, and the deposit still has no such channel
    assert "HNB_SPLAT_ATTR_ONE" not in open(os.path.join(ROOT, "include", "hanabi_amd_deposit.h")).read()


def test_calls_fail_loudly_on_null_arguments_and_without_a_device():
    """Up to the device check: the NULL refusals come before anything is dereferenced, loaded or enqueued. The refusals of a description's members
    need an effect, and an effect a device: the stand-alone program below holds them, and tests/test_gpu_splat.py on a live effect."""
    lib = runtime.load_library()
    d = runtime.deposit_desc((1, 1, 1), (0, 0, 0), (1, 1, 1), 0x1000)
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for call in (lib.hnb_effect_splat, lib.hnb_program_splat):
        for args in ((None, C.byref(d)), (fake, None), (None, None)):
            assert call(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to splat, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------
def test_code_object_is_built_carried_and_has_its_two_kernels_without_scratch_or_spills():
    co = hb.splat_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_splat.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(SPLAT_KERNELS), sorted(rows)
    for name, r in rows.items():
        # the table of k_splat_lds is dynamic LDS sized by the plan (at most the budget: the plan's sweep below); the fixed part is small
        assert r["group_segment_fixed_size"] <= 64, f"{name}: {r['group_segment_fixed_size']} B of fixed LDS per workgroup"
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["kernarg_segment_size"] == 184, (name, r)                # one SplatArgs (the deposit's block) by value
        assert r["vgpr_count"] <= 128, (name, r)                          # four waves per SIMD stay possible
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_splat_code)
    for h in ("hnb_splat.h", "hnb_deposit.h", "hnb_sample.h", "hnb_bin_cell.h", "hnb_sort_key.h"):
        assert f'"{h}"' in inspect.getsource(hb.build_splat_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_splat.hip")).read()
    assert open(os.path.join(CSRC, "hnb_splat.h")).read().count("#pragma clang fp contract(off)") == 3     # every function with f32 arithmetic
    assert hb.SPLAT_CODE_OBJECTS == (hb.build_splat_code,)
    assert hb.EXPORT_CODE_OBJECTS == (hb.build_export_code, hb.build_export_sort_code, hb.build_export_filter_code, hb.build_export_cull_code, hb.build_export_filter_prog_code,
                                      hb.build_export_cull_prog_code)
    assert (hb.BINNED_CODE_OBJECTS, hb.IMPORT_CODE_OBJECTS, hb.QUERY_CODE_OBJECTS, hb.DEPOSIT_CODE_OBJECTS, hb.SAMPLE_CODE_OBJECTS) == (
        (hb.build_export_bin_code,), (hb.build_import_code,), (hb.build_bounds_code,), (hb.build_deposit_code,), (hb.build_sample_code,))
    assert "SPLAT_CODE_OBJECTS" in inspect.getsource(hb.build_runtime) and "hanabi_amd_splat.h" in inspect.getsource(hb.build_runtime)
    assert "hanabi_amd_splat.h" in inspect.getsource(hb._build_code_object)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_splat_code.inc" in ignored and "*.hsaco" in ignored
    for other in (hb.bounds_code_path(), hb.export_bin_code_path(), hb.import_code_path(), hb.deposit_code_path(), hb.sample_code_path()):
        assert not set(_rows(other)) & set(SPLAT_KERNELS)


# ---- csrc/hnb_splat.h as a stand-alone host program under the sanitizers --------------------------------------------------------------------------------
ERRORS = ["Ok", "ErrStructSize", "ErrFlags", "ErrDims", "ErrOrigin", "ErrInvCell", "ErrChannelCount", "ErrAttr", "ErrComp", "ErrFracBits", "ErrChannelReserved", "ErrUnusedChannel",
          "ErrCount", "ErrSums", "ErrStats", "ErrNoPosition"]                # the deposit's, by the deposit's numbers ...
E = {n: i for i, n in enumerate(ERRORS)}
E["ErrOneComp"] = len(ERRORS)                                              # ... and the one the splat adds, behind them
# what the check is given: (attr, ncomp, is_f32); layout 1 has no POSITION
LAYOUT = [(A.POSITION.id, 3, 1), (A.VELOCITY.id, 3, 1), (A.AGE.id, 1, 1), (A.LIFETIME.id, 1, 1), (A.COLOR.id, 1, 0), (A.HDR_COLOR.id, 4, 1), (A.SIZE2.id, 2, 1)]

HOST_SRC = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "hnb_splat.h"
using namespace hnb;
""" + "\n".join(f"static_assert(kDeposit{n} == {i}, \"DepositDescError\");" for i, n in enumerate(ERRORS)) + r"""
static_assert(kSplatErrOneComp == """ + str(len(ERRORS)) + " && kSplatDescErrorCount == " + str(len(ERRORS) + 1) + r""", "the splat's error behind the deposit's");
static_assert(sizeof(HnbDepositDesc) == 136 && sizeof(SplatArgs) == 184 && sizeof(DepositArgs) == 184 && kSplatKLds == 0 && kSplatKGlobal == 1 && kSplatKernelCount == 2, "hnb_splat.h");
static_assert(kSplatTile == """ + str(TILE) + r""" && kSplatBlock == 256 && kSplatOneBits == 0x3F800000u && HNB_SPLAT_ATTR_ONE == 0xFFFFFFFFu, "hnb_splat.h");
static const DepositLayoutAttr kLayout[] = {""" + ", ".join("{%d, %d, %d}" % l for l in LAYOUT) + r"""};
static float f_of(unsigned b) { float f; std::memcpy(&f, &b, 4); return f; }
static unsigned b_of(float f) { unsigned b; std::memcpy(&b, &f, 4); return b; }
static bool read_desc(HnbDepositDesc& d, unsigned& layout_first) {
    std::memset(&d, 0, sizeof d);
    unsigned long long count, sums, stats; unsigned ob[3], ib[3];
    if (std::scanf("%u %u %u %u %u %u %u %x %x %x %x %x %x %llx %llx %llx", &layout_first, &d.struct_size, &d.flags, &d.dims[0], &d.dims[1], &d.dims[2], &d.n_channels, &ob[0], &ob[1],
                   &ob[2], &ib[0], &ib[1], &ib[2], &count, &sums, &stats) != 16) return false;
    std::memcpy(d.origin, ob, 12); std::memcpy(d.inv_cell, ib, 12);
    d.count = (uint32_t*)(uintptr_t)count; d.sums = (int64_t*)(uintptr_t)sums; d.out_stats = (uint32_t*)(uintptr_t)stats;
    for (unsigned k = 0; k < HNB_DEPOSIT_MAX_CHANNELS; ++k)
        if (std::scanf("%u %u %u %u", &d.channels[k].attr, &d.channels[k].comp, &d.channels[k].frac_bits, &d.channels[k].reserved) != 4) return false;
    return layout_first <= 1;
}
int main() {
    char what[16];
    BinGrid g = {};
    std::vector<uint64_t> tab;                // exactly n_cells + 1 rows on the heap: a row past them is an error the sanitizer reports
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "names")) {
            for (uint32_t i = 0; i < kSplatKernelCount; ++i) std::printf("%u:%s ", kSplatKernelNames[i].kernel, kSplatKernelNames[i].name);
            std::printf("\n");
        } else if (!std::strcmp(what, "plan")) {
            unsigned program, n_inst, cap, n_cells, nch;
            if (std::scanf("%u %u %u %u %u", &program, &n_inst, &cap, &n_cells, &nch) != 5) return 1;
            const SplatPlan pl = splat_launch_plan(program != 0, n_inst, cap, n_cells, nch);
            std::printf("%s %u %u %u %u %llu %llu %llu\n", pl.kernel < kSplatKernelCount ? kSplatKernelNames[pl.kernel].name : "?", pl.grid_x, pl.grid_y, pl.span, pl.lds_bytes,
                        (unsigned long long)pl.clear_count_bytes, (unsigned long long)pl.clear_sums_bytes, (unsigned long long)pl.clear_stats_bytes);
        } else if (!std::strcmp(what, "desc") || !std::strcmp(what, "ddesc")) {       // the splat's check; the deposit's own on the same description
            HnbDepositDesc d; unsigned layout_first;
            if (!read_desc(d, layout_first)) return 1;
            const uint32_t n = (uint32_t)(sizeof kLayout / sizeof *kLayout) - layout_first;
            const DepositCheck c = what[1] == 'd' ? deposit_check_desc(d, kLayout + layout_first, n) : splat_check_desc(d, kLayout + layout_first, n);
            if (c.error >= kSplatDescErrorCount || !splat_error_text(c.error)[1]) return 3;
            std::printf("%u %u %u %u %d", c.error, c.channel, c.n_cells, c.position_index, c.has_age ? 1 : 0);
            for (uint32_t k = 0; k < d.n_channels && k < HNB_DEPOSIT_MAX_CHANNELS; ++k) std::printf(" %u", c.layout_index[k]);
            std::printf("\n");
        } else if (!std::strcmp(what, "pack")) {
            unsigned one, ncomp, comp, frac;
            if (std::scanf("%u %u %u %u", &one, &ncomp, &comp, &frac) != 4) return 1;
            const uint32_t p = splat_pack_channel(one != 0, ncomp, comp, frac);
            std::printf("%d %u %u %u\n", splat_channel_is_one(p) ? 1 : 0, deposit_channel_ncomp(p), deposit_channel_comp(p), deposit_channel_frac_bits(p));
        } else if (!std::strcmp(what, "grid")) {
            unsigned ob[3], ib[3];
            if (std::scanf("%u %u %u %x %x %x %x %x %x", &g.dims[0], &g.dims[1], &g.dims[2], &ob[0], &ob[1], &ob[2], &ib[0], &ib[1], &ib[2]) != 9) return 1;
            for (int c = 0; c < 3; ++c) { g.origin[c] = f_of(ob[c]); g.inv_cell[c] = f_of(ib[c]); }
            g.n_cells = bin_cell_count(g.dims);
            tab.assign((size_t)g.n_cells + 1u, 0u);
            tab.shrink_to_fit();
            std::printf("%u\n", g.n_cells);
        } else if (!std::strcmp(what, "s")) {     // one particle and one value through the kernels' own functions, in the kernels' order
            unsigned pb[3], vb, frac;
            if (std::scanf("%x %x %x %x %u", &pb[0], &pb[1], &pb[2], &vb, &frac) != 5) return 1;
            const float x = f_of(pb[0]), y = f_of(pb[1]), z = f_of(pb[2]);
            const uint32_t cell = bin_cell_of(g, x, y, z);
            const DepositQuant q = deposit_quantise(vb, frac);
            std::printf("%u %d", cell, q.ok ? 1 : 0);
            if (cell == g.n_cells) {
                if (q.ok) { tab[cell] += (uint64_t)q.q; std::printf(" %lld", (long long)q.q); }
            } else {
                const SplatAxis ax = splat_axis(sample_axis_t(x, g.origin[0], g.inv_cell[0]), g.dims[0]);
                const SplatAxis ay = splat_axis(sample_axis_t(y, g.origin[1], g.inv_cell[1]), g.dims[1]);
                const SplatAxis az = splat_axis(sample_axis_t(z, g.origin[2], g.inv_cell[2]), g.dims[2]);
                const SplatCorners c = splat_corners(g.dims, ax, ay, az);
                for (int i = 0; i < 8; ++i) std::printf(" %u %x", c.row[i], b_of(c.w[i]));
                if (q.ok)
                    for (int i = 0; i < 8; ++i) {
                        const int64_t qi = splat_contribution(vb, c.w[i], frac);
                        tab[c.row[i]] += (uint64_t)qi;
                        std::printf(" %lld", (long long)qi);
                    }
            }
            std::printf("\n");
        } else if (!std::strcmp(what, "tab")) {   // the table the particles since `grid` were added into
            for (size_t i = 0; i < tab.size(); ++i) std::printf("%lld ", (long long)(int64_t)tab[i]);
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
    tmp = tmp_path_factory.mktemp("splat_host")
    (tmp / "spl.cpp").write_text(HOST_SRC)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), str(tmp / "spl.cpp"), "-o", str(tmp / "spl")])
    return str(tmp / "spl")


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()      # (a sanitizer report ends the program with an error)
    assert len(out) == len(lines)
    return out


def _f32(x):
    return int(np.array([x], F32).view(U32)[0])


def _desc_line(what="desc", layout_first=0, struct_size=136, flags=0, dims=(4, 4, 4), n_channels=2, origin=(0.0, 0.0, 0.0), inv_cell=(1.0, 1.0, 1.0), count=0x1000, sums=0x2000,
               stats=0x3000, channels=((ONE, 0, 30, 0), (A.HDR_COLOR.id, 3, 32, 0))):
    ch = list(channels) + [(0, 0, 0, 0)] * (4 - len(channels))
    return ("%s %d %d %d %d %d %d %d " % (what, layout_first, struct_size, flags, *dims, n_channels) + " ".join("%x" % _f32(x) for x in tuple(origin) + tuple(inv_cell))
            + " %x %x %x " % (count, sums, stats) + " ".join("%d %d %d %d" % c for c in ch))


def test_description_check_refuses_what_the_header_lists(host_exe):
    ask = lambda **kw: [int(x) for x in _ask(host_exe, [_desc_line(**kw)])[0].split()]
    none = 0xFFFFFFFF                                                      # kSplatLayoutOne: a channel of ONE has no entry of the layout
    assert ask() == [E["Ok"], 0, 64, 0, 0, none, 5]                        # n_cells, POSITION's entry, AGE is not read, the channels' entries
    assert ask(channels=((A.AGE.id, 0, 16, 0), (ONE, 0, 0, 0))) == [E["Ok"], 0, 64, 0, 1, 2, none]
    assert ask(n_channels=4, channels=((ONE, 0, 32, 0), (ONE, 0, 0, 0), (A.SIZE2.id, 1, 7, 0), (ONE, 0, 30, 0))) == [E["Ok"], 0, 64, 0, 0, none, none, 6, none]
    assert ask(n_channels=0, channels=(), sums=0, stats=0)[:5] == [E["Ok"], 0, 64, 0, 0]
    assert ask(flags=1)[0] == E["Ok"] and ask(dims=(1 << 24, 1, 1))[:3] == [E["Ok"], 0, 1 << 24]
    # ONE: its comp must be 0; its frac_bits and reserved follow every channel's rule; an unused entry may not hold it
    for comp in (1, 2, 0xFFFFFFFF):
        assert ask(channels=((A.AGE.id, 0, 16, 0), (ONE, comp, 30, 0)))[:2] == [E["ErrOneComp"], 1]
    assert ask(channels=((ONE, 0, 33, 0), (ONE, 0, 0, 0)))[:2] == [E["ErrFracBits"], 0] and ask(channels=((ONE, 0, 30, 1),) * 2)[:2] == [E["ErrChannelReserved"], 0]
    assert ask(n_channels=1, channels=((A.AGE.id, 0, 16, 0), (ONE, 0, 0, 0)))[:2] == [E["ErrUnusedChannel"], 1]
    # ... and hnb_effect_deposit's check keeps refusing that attr, and flags = 2
    assert [int(x) for x in _ask(host_exe, [_desc_line(what="ddesc")])[0].split()][:2] == [E["ErrAttr"], 0]
    assert [int(x) for x in _ask(host_exe, [_desc_line(what="ddesc", flags=2, channels=((A.AGE.id, 0, 0, 0),) * 2)])[0].split()][0] == E["ErrFlags"]
    # the deposit's list, unchanged
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
    for attr in (A.COLOR.id, A.SIZE3.id, A.ID.id, A.PARTICLE_COUNTER.id, 39, 9999, ONE - 1):      # packed u32; not in the layout; not stored; no attribute
        assert ask(channels=(good, (attr, 0, 0, 0)))[:2] == [E["ErrAttr"], 1], attr
    for attr, comp in ((A.AGE.id, 1), (A.POSITION.id, 3), (A.HDR_COLOR.id, 4), (A.SIZE2.id, 2), (A.AGE.id, 0xFFFFFFFF)):
        assert ask(channels=((attr, comp, 0, 0), good))[:2] == [E["ErrComp"], 0]
    assert ask(channels=(good, (A.AGE.id, 0, 33, 0)))[:2] == [E["ErrFracBits"], 1] and ask(channels=(good, (A.AGE.id, 0, 32, 0)))[0] == E["Ok"]
    assert ask(channels=(good, (A.AGE.id, 0, 0, 1)))[:2] == [E["ErrChannelReserved"], 1]
    for k, entry in ((2, (A.AGE.id, 0, 0, 0)), (3, (0, 1, 0, 0)), (2, (0, 0, 1, 0)), (3, (0, 0, 0, 1)), (2, (ONE, 0, 0, 0))):
        ch = [good, good, (0, 0, 0, 0), (0, 0, 0, 0)]; ch[k] = entry
        assert ask(channels=ch)[:2] == [E["ErrUnusedChannel"], k]
    for count in (0, 0x1004, 0x1008):
        assert ask(count=count)[0] == E["ErrCount"]
    assert ask(sums=0)[0] == E["ErrSums"] and ask(sums=0x2008)[0] == E["ErrSums"] and ask(n_channels=0, channels=())[0] == E["ErrSums"]      # missing; misaligned; given without channels
    assert ask(stats=0x3004)[0] == E["ErrStats"] and ask(stats=0)[0] == E["Ok"]
    assert ask(layout_first=1)[0] == E["ErrNoPosition"]
    # the marker of ONE in the kernels' argument block: a component count of 0, which no attribute of the layout has
    assert _ask(host_exe, ["pack 1 3 2 30", "pack 0 3 2 30", "pack 0 1 0 0", "pack 1 0 0 32"]) == ["1 0 0 30", "0 3 2 30", "0 1 0 0", "1 0 0 32"]


def test_launch_plan_is_its_restatement_and_the_deposits_decision(host_exe):
    assert _ask(host_exe, ["names"])[0].split() == [f"{i}:{n}" for i, n in enumerate(SPLAT_KERNELS)]
    caps = (1, 255, 4096, 4097, 3 * 4096 + 5, 300_007, 16_777_216, 2 ** 32 - 1)
    cells = {1, 64, 512, 1364, 1365, 4095, 4096, 12287, 12288, 64 ** 3, BIN_MAX_CELLS}
    for k in range(5):
        cells |= {last_lds_cells(k), last_lds_cells(k) + 1}
    cases = [(program, n, cap, nc, k) for cap in caps for nc in sorted(cells) for k in range(5) for program, n in ((0, 1), (1, 1), (1, 300), (1, 65_535))]
    out = _ask(host_exe, ["plan %d %d %d %d %d" % c for c in cases])
    for case, line in zip(cases, out):
        w = line.split()
        got = (w[0],) + tuple(int(x) for x in w[1:])
        assert got == splat_plan(*case), (case, got)
        kernel, gx, gy, span, lds = got[:5]
        program, n, cap, nc, k = case
        tiles = -(-cap // TILE)
        assert (kernel == "k_splat_lds") == (table_bytes(nc, k) <= LDS_BUDGET) and lds <= LDS_BUDGET and gy == (n if program else 1)
        assert gx >= 1 and gx * span >= tiles > (gx - 1) * span          # every tile belongs to one workgroup, and every workgroup has one
        if kernel == "k_splat_lds":
            assert lds == table_bytes(nc, k) and 1 <= span <= 24 and (span - 1) * SPAN_BYTES < lds <= span * SPAN_BYTES
    for k in range(5):                                                  # the last table on the LDS path and the first off it, for 0 .. 4 channels
        n = last_lds_cells(k)
        assert splat_plan(False, 1, 10_000, n, k)[0] == "k_splat_lds" and splat_plan(False, 1, 10_000, n + 1, k)[0] == "k_splat_global"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## Splat" in design and design.index("## Sample") < design.index("## Splat") < design.index("## Measurement (row d)")
    for word in ("`k_splat_lds`", "`k_splat_global`", "`ds_add_u64`", "`global_atomic_add_x2`", "profiles/splat_ab.log"):
        assert word in design, word


# ---- the rule, through the kernels' own functions -----------------------------------------------------------------------------------------------------
RULE_GRIDS = [(1, 1, 1), (1, 3, 2), (2, 1, 7), (5, 4, 1), (4, 4, 4)]
FRACS = (0, 1, 16, 30, 32)
# the deposit's edge lattice: the bound 2^62 on both sides, +-2^61, denormals, ties, zeros of both signs, what is rejected everywhere
EDGE_VALUES = [2.0 ** 62 * (1 - 2.0 ** -24), 2.0 ** 62, -(2.0 ** 62), 2.0 ** 61, -(2.0 ** 61), 2.0 ** 29, 2.0 ** 30 * (1 - 2.0 ** -24), 2.0 ** 30, 1e-45, -1e-40, 1.1754942e-38, 1.1754944e-38,
               2.0 ** -33, 2.0 ** -34, 0.5, 1.5, 2.5, -0.5, -1.5, -3.5, 0.0, -0.0, 1.0, -2.75, 3e38, -3e38, np.nan, np.inf, -np.inf]


def rule_positions(dims, rng):
    """positions at unit cells from 0 (t = p): every pair of axes at every edge value of test_sample_abi.axis_values - -0, the lowest corner, faces, centres, one
    ulp either side of a face and of t = 0.5 (below it u is a tiny negative number and w1 rounds to 1.0) and of dim - 0.5, outside, NaN - the third at a few"""
    lat = [axis_values(d) for d in dims]
    picks = [l[rng.permutation(len(l))[:4]] for l in lat]
    pts = [(F32(-0.0), F32(0.0), F32(-0.0)), tuple(F32(d - 0.5) for d in dims), tuple(np.nextafter(F32(0.5), F32(0)) for _ in dims)]
    for c in range(3):
        axes = [picks[0], picks[1], picks[2]]
        axes[c] = lat[c]
        axes[(c + 1) % 3] = lat[(c + 1) % 3]
        pts += list(itertools.product(*axes))
    lattice = np.unique(np.array(pts, F32).view(U32).reshape(-1, 3), axis=0).view(F32)
    if len(lattice) > 900:
        lattice = np.concatenate([np.array(pts[:3], F32), lattice[rng.permutation(len(lattice))[:900]]])
    return lattice


def _expect_lines(pos, v_bits, frac, dims, origin, inv_cell):
    """the line the host program prints per (particle, value): cell, ok and - inside - the eight (row, W bits), then the accepted contributions"""
    cells, inside, rows, W, clamped = np_splat_parts(pos, dims, origin, inv_cell)
    ok, q = np_quantise(v_bits, frac)
    okc, qc, cv = np_corner_q(v_bits[inside], W, frac)
    assert okc[ok[inside]].all(), "a corner of an accepted value is rejected"
    flushed = np.where(np.abs(cv) < F32(2.0 ** -126), F32(0.0), cv)       # what hardware that flushes f32 denormals would quantise
    _, qf = np_quantise(np.ascontiguousarray(flushed).view(U32), frac)
    np.testing.assert_array_equal(qf[ok[inside]], qc[ok[inside]], err_msg="zeroing a denormal product changes a contribution")
    out, m = [], 0
    for i in range(len(pos)):
        w = ["%d %d" % (cells[i], ok[i])]
        if inside[i]:
            w += ["%d %x" % (rows[m, c], W[m, c].view(U32)) for c in range(8)]
            if ok[i]:
                w += ["%d" % x for x in qc[m]]
            m += 1
        elif ok[i]:
            w.append("%d" % q[i])
        out.append(" ".join(w))
    stats = dict(inside=int(inside.sum()), clamped=int(clamped.sum()), accepted=int(ok.sum()), denormal=int(((cv != 0) & (np.abs(cv) < F32(2.0 ** -126)))[ok[inside]].sum()),
                 negative=int((qc[ok[inside]] < 0).sum()), w1_is_one=int((W == 1).any(axis=1).sum()))
    return out, stats


@pytest.mark.parametrize("dims", RULE_GRIDS, ids=["x".join(map(str, d)) for d in RULE_GRIDS])
def test_rule_under_the_sanitizers_is_the_numpy_restatement_bit_for_bit(host_exe, dims):
    rng = np.random.default_rng(dims[0] * 100 + dims[1] * 10 + dims[2])
    unit = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), rule_positions(dims, rng))
    origin = np.array([-1.5, 0.3, -7.25], F32)
    size = np.array([3.1, 0.7, 11.0], F32)
    inv_cell = (np.array(dims, F32) / size).astype(F32)
    odd = (origin, inv_cell, (origin + size * rng.uniform(-0.05, 1.05, (600, 3))).astype(F32))
    edge = np.array(EDGE_VALUES, F32).view(U32)
    total = dict(inside=0, clamped=0, accepted=0, denormal=0, negative=0, w1_is_one=0)
    n = 0
    for o, iv, pos in (unit, odd):
        lines, want = ["grid %d %d %d " % tuple(dims) + " ".join("%x" % _f32(x) for x in tuple(o) + tuple(iv))], []
        tab = np.zeros(dims[0] * dims[1] * dims[2] + 1, np.uint64)
        for frac in FRACS:
            # every position with a few values: one of the edge lattice (each in turn), a random one, a tiny one whose products fall into the denormal range
            v = np.stack([edge[(np.arange(len(pos)) + frac) % len(edge)], rng.normal(0, 30, len(pos)).astype(F32).view(U32),
                          (rng.normal(0, 1, len(pos)) * 2.0 ** -120).astype(F32).view(U32)], axis=1)
            for j in range(v.shape[1]):
                exp, st = _expect_lines(pos, v[:, j], frac, dims, o, iv)
                want += exp
                lines += ["s %x %x %x %x %d" % (*[int(b) for b in p], int(vb), frac) for p, vb in zip(pos.view(U32), v[:, j])]
                for key in total:
                    total[key] += st[key]
                n += len(pos)
                _, sums, _ = np_splat(pos, np.ones(len(pos), bool), dims, o, iv, [v[:, j]], [frac])
                tab += sums[:, 0].view(np.uint64)
        got = _ask(host_exe, lines + ["tab"])
        assert int(got[0]) == dims[0] * dims[1] * dims[2]
        bad = [(lines[1 + i], got[1 + i], want[i]) for i in range(len(want)) if got[1 + i] != want[i]]
        assert not bad, (dims, len(bad), bad[:4])
        # ... and the table the program summed them into is np_splat's over the same particles: the rows, the clamped corners that share one, the outside row
        np.testing.assert_array_equal(np.array([int(x) for x in got[-1].split()], np.int64), tab.view(np.int64), err_msg=f"{dims}: the summed table")
    # the sweep holds what it is meant to
    assert 0 < total["inside"] < n and 0 < total["accepted"] < n and total["clamped"] > 0 and total["denormal"] > 0 and total["negative"] > 0 and total["w1_is_one"] > 0, total
    if 1 in dims:
        assert total["clamped"] == total["inside"]                        # an axis of one cell: both of its corners are cell 0 for every inside particle
