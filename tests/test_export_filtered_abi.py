"""The filtered export (hnb_effect_export_filtered, include/hanabi_amd.h "Packed output") without a GPU: the ctypes mirror has the header's layout,
the call fails loudly, the predicates the kernels call (csrc/hnb_filter_pred.h) are the header's formulas bit for bit - rounded operation by
operation, which a contracted build would not be - the kernels live in a third code object with no scratch, the first two code objects are what
they were, and the scratch layout's sections do not overlap."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import runtime
from test_export_sorted_abi import A, LLVM, ROOT, key_f32

CSRC = os.path.join(ROOT, "bevy_hanabi_amd", "csrc")
F32 = np.float32


# ---- the header's formulas, restated in numpy binary32: one ufunc per operation, in the order written ---------------------------------------------
def pass_planes(p, planes):
    """p: [n, 3] f32, planes: [k, 4] f32 -> [n] bool: ((x*P0 + y*P1) + z*P2) + P3 >= 0 for every plane"""
    p, planes = np.asarray(p, F32).reshape(-1, 3), np.asarray(planes, F32).reshape(-1, 4)
    keep = np.ones(len(p), bool)
    with np.errstate(all="ignore"):
        for P in planes:
            s = ((p[:, 0] * P[0] + p[:, 1] * P[1]) + p[:, 2] * P[2]) + P[3]
            assert s.dtype == F32
            keep &= s >= F32(0)
    return keep


def pass_sphere(p, sphere):
    """p: [n, 3] f32, sphere: (cx, cy, cz, r^2) -> [n] bool: (ex*ex + ey*ey) + ez*ez <= r^2, e = p - c"""
    p, S = np.asarray(p, F32).reshape(-1, 3), np.asarray(sphere, F32)
    with np.errstate(all="ignore"):
        e = p - S[:3]
        d = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        assert d.dtype == F32
        return d <= S[3]


def range_key(bits, is_f32):
    b = np.asarray(bits, np.uint32)
    return key_f32(b) if is_f32 else b.copy()


def pass_range(bits, is_f32, lo_bits, hi_bits):
    k = range_key(bits, is_f32)
    return (range_key(lo_bits, is_f32) <= k) & (k <= range_key(hi_bits, is_f32))


def bits_of(x):
    return np.asarray(x, F32).view(np.uint32)


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_has_the_headers_size_and_offsets(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd.h"
    int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u %u %u\n", sizeof(HnbExportFilter), offsetof(HnbExportFilter, kind), offsetof(HnbExportFilter, n_planes),
                            offsetof(HnbExportFilter, attr), offsetof(HnbExportFilter, invert), offsetof(HnbExportFilter, lo_bits), offsetof(HnbExportFilter, hi_bits),
                            offsetof(HnbExportFilter, reserved), offsetof(HnbExportFilter, P),
                            HNB_FILTER_PLANES, HNB_FILTER_SPHERE, HNB_FILTER_ATTR_RANGE, HNB_FILTER_MAX_PLANES);
                     return hnb_effect_export_filtered == 0; }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    S = runtime.ExportFilter
    assert got == [C.sizeof(S), S.kind.offset, S.n_planes.offset, S.attr.offset, S.invert.offset, S.lo_bits.offset, S.hi_bits.offset, S.reserved.offset, S.P.offset,
                   runtime.FILTER_PLANES, runtime.FILTER_SPHERE, runtime.FILTER_ATTR_RANGE, runtime.FILTER_MAX_PLANES]
    assert C.sizeof(S) == 32 + 16 * 6
    f = runtime.export_filter("planes", planes=[(1, 0, 0, -2.5), (0, -1, 0, 4)], invert=True)
    assert (f.struct_size, f.kind, f.n_planes, f.attr, f.invert, f.lo_bits, f.hi_bits, f.reserved) == (C.sizeof(S), runtime.FILTER_PLANES, 2, 0, 1, 0, 0, 0)
    assert [list(r) for r in f.P][:3] == [[1.0, 0.0, 0.0, -2.5], [0.0, -1.0, 0.0, 4.0], [0.0] * 4]
    f = runtime.export_filter("sphere", sphere=(1, 2, 3, 6.25))
    assert (f.kind, f.n_planes, f.invert, list(f.P[0])) == (runtime.FILTER_SPHERE, 0, 0, [1.0, 2.0, 3.0, 6.25])
    f = runtime.export_filter("attr_range", attr=A.AGE.id, lo=0.5, hi=np.float32(2.0))
    assert (f.kind, f.attr, f.lo_bits, f.hi_bits) == (runtime.FILTER_ATTR_RANGE, A.AGE.id, 0x3F000000, 0x40000000)
    f = runtime.export_filter(runtime.FILTER_ATTR_RANGE, attr=A.COLOR.id, lo=0x80000000, hi=0xFFFFFFFF)         # ints: bit patterns
    assert (f.lo_bits, f.hi_bits) == (0x80000000, 0xFFFFFFFF)
    assert "hnb_effect_export_filtered" in runtime.ABI_SYMBOLS and hasattr(runtime.load_library(), "hnb_effect_export_filtered")


def test_call_fails_loudly_on_null_arguments_and_without_a_device():
    lib = runtime.load_library()
    d = runtime.export_desc([(A.POSITION.id, 0)], 0x1000, 16, 1)
    f = runtime.export_filter("sphere", sphere=(0, 0, 0, 1))
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for args in ((None, C.byref(d), C.byref(f)), (fake, None, C.byref(f)), (fake, C.byref(d), None), (None, None, None)):
        assert lib.hnb_effect_export_filtered(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to export from, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the predicates -------------------------------------------------------------------------------------------------------------------------------
PRED_SRC = r'''
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "hnb_filter_pred.h"
static float f(unsigned b) { float v; std::memcpy(&v, &b, 4); return v; }
int main() {
    char tag;
    while (std::scanf(" %c", &tag) == 1) {
        if (tag == 'P') {
            unsigned n, x, y, z; float P[6][4] = {};
            if (std::scanf("%u %x %x %x", &n, &x, &y, &z) != 4) return 1;
            for (unsigned i = 0; i < n; ++i) for (int c = 0; c < 4; ++c) { unsigned b; if (std::scanf("%x", &b) != 1) return 1; P[i][c] = f(b); }
            std::printf("%d\n", (int)hnb::filter_pass_planes(f(x), f(y), f(z), P, n));
        } else if (tag == 'S') {
            unsigned x, y, z, s[4]; float S[4];
            if (std::scanf("%x %x %x %x %x %x %x", &x, &y, &z, &s[0], &s[1], &s[2], &s[3]) != 7) return 1;
            for (int c = 0; c < 4; ++c) S[c] = f(s[c]);
            std::printf("%d\n", (int)hnb::filter_pass_sphere(f(x), f(y), f(z), S));
        } else if (tag == 'R') {
            unsigned b, isf, lo, hi;
            if (std::scanf("%x %u %x %x", &b, &isf, &lo, &hi) != 4) return 1;
            std::printf("%d\n", (int)hnb::filter_pass_range(b, isf != 0, lo, hi));
        } else return 1;
    }
    return 0;
}
'''

ONE = 0x3F800000
EDGE_BITS = [0x00000000, 0x80000000,             # +-0
             0x00000001, 0x80000001,             # +-denormal min
             0x007FFFFF,                         # denormal max
             0x00800000,                         # FLT_MIN
             ONE - 1, ONE, ONE + 1,              # one ulp either side of 1
             0xBF800000,                         # -1
             0x7F7FFFFF, 0xFF7FFFFF,             # +-FLT_MAX
             0x7F800000, 0xFF800000,             # +-inf
             0x7FC00000, 0xFFC00001]             # NaNs of both signs

# x * a rounds (to even, downwards) where a fused multiply-add keeps the product whole: x = a = 1 + 2^-12, x*a = 1 + 2^-11 + 2^-24 -> 1 + 2^-11.
# With y * b = -(1 + 2^-11) exactly: (x*a + y*b) = 0 rounded operation by operation, 2^-24 fused; d = -2^-25 puts the two on either side of 0.
FMA_P = np.array([1 + 2.0 ** -12, -1.0, 0.0], F32)
FMA_PLANE = np.array([1 + 2.0 ** -12, 1 + 2.0 ** -11, 0.0, -(2.0 ** -25)], F32)
# ey*ey = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11; + ex*ex = 2^-24 is a tie that rounds back to 1 + 2^-11, exactly the squared radius: kept. With ey*ey
# left whole inside a fused add the sum is 1 + 2^-11 + 2^-23: outside.
FMA_SPHERE_P = np.array([2.0 ** -12, 1 + 2.0 ** -12, 0.0], F32)
FMA_SPHERE = np.array([0.0, 0.0, 0.0, 1 + 2.0 ** -11], F32)


def _compile_pred(tmp_path):
    (tmp_path / "pred.cpp").write_text(PRED_SRC)
    exe = str(tmp_path / "pred")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + CSRC, str(tmp_path / "pred.cpp"), "-o", exe])
    return exe


def _hex(a):
    return " ".join(f"{int(b):x}" for b in np.asarray(a, F32).reshape(-1).view(np.uint32))


def test_predicates_agree_with_the_numpy_restatement_bit_for_bit(tmp_path):
    exe = _compile_pred(tmp_path)
    lines, want = [], []
    pos = np.array(list(itertools.product(EDGE_BITS, repeat=3)), np.uint32).view(F32)                 # 4096 positions of edge operands
    rng = np.random.default_rng(3)
    plane_sets = [np.array([[1, 0, 0, 0]], F32),                                                      # s == x: -0 and +0 pass, NaN does not
                  np.array([[1, 0, 0, -1]], F32),                                                     # x exactly on, one ulp either side of, the plane
                  np.array([[0.3, -0.5, 0.8, 0.25], [-1, -1, -1, 3e38]], F32),
                  np.concatenate([rng.uniform(-2, 2, (5, 4)).astype(F32), FMA_PLANE[None]]),          # six planes
                  FMA_PLANE[None]]
    with np.errstate(all="ignore"):
        for planes in plane_sets:
            ps = np.concatenate([pos, FMA_P[None], rng.uniform(-3, 3, (200, 3)).astype(F32)])
            want.append(pass_planes(ps, planes))
            lines += [f"P {len(planes)} {_hex(p)} {_hex(planes)}" for p in ps]
        for sphere in (np.array([0, 0, 0, 1], F32), np.array([0, 0, 0, 0], F32), np.array([1, -1, 0.5, 3], F32), np.array([0, 0, 0, np.float32(3.4e38)], F32), FMA_SPHERE):
            ps = np.concatenate([pos, FMA_SPHERE_P[None], rng.uniform(-2, 2, (200, 3)).astype(F32)])
            want.append(pass_sphere(ps, sphere))
            lines += [f"S {_hex(p)} {_hex(sphere)}" for p in ps]
    edges = np.array(EDGE_BITS + [0x7FFFFFFF, 0xFFFFFFFF, 0x3F000000], np.uint32)
    for is_f32 in (1, 0):
        for lo, hi in itertools.product(edges, repeat=2):
            if range_key(lo, is_f32) > range_key(hi, is_f32):
                continue                                                                              # (the library refuses these; the function is total anyway)
            want.append(pass_range(edges, is_f32, lo, hi))
            lines += [f"R {int(b):x} {is_f32} {int(lo):x} {int(hi):x}" for b in edges]
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.split()
    want = np.concatenate(want)
    got = np.array([int(x) for x in out], bool)
    assert got.shape == want.shape and len(want) > 30_000
    np.testing.assert_array_equal(got, want)
    assert 0.05 < want.mean() < 0.95
    # the edges behave as the header says
    assert pass_planes([-0.0, 5, 5], [[1, 0, 0, 0]])[0] and pass_planes([0.0, 5, 5], [[1, 0, 0, 0]])[0]          # -0 >= 0
    assert not pass_planes([np.nan, 0, 0], [[1, 0, 0, 0]])[0] and not pass_sphere([np.nan, 0, 0], [0, 0, 0, np.inf])[0]              # a NaN never passes
    x = np.array([ONE - 1, ONE, ONE + 1], np.uint32).view(F32)
    assert list(pass_planes(np.stack([x, 0 * x, 0 * x], 1), [[1, 0, 0, -1]])) == [False, True, True]                               # s == 0 is kept
    assert list(pass_sphere(np.stack([x, 0 * x, 0 * x], 1), [0, 0, 0, 1])) == [True, True, False]                                   # d == r^2 is kept
    assert list(pass_range(np.array([0x80000000, 0], np.uint32), 1, 0, 0x3F800000)) == [False, True]                               # -0 is below +0 in the key order
    assert list(pass_range(np.array([0x7FFFFFFF, 0x80000000], np.uint32), 0, 0x80000000, 0xFFFFFFFF)) == [False, True]             # unsigned


def test_a_contracted_evaluation_would_be_seen(tmp_path):
    """The operands above, evaluated as a fused multiply-add would (the product kept whole: float64 holds it exactly), give the OTHER answer: the
    agreement of the test above is agreement on the rounding of every operation, not an accident of forgiving inputs."""
    x, y, _ = FMA_P.astype(np.float64)
    a, b, _, d = FMA_PLANE.astype(np.float64)
    by = F32(F32(y) * F32(b))
    fused = F32(F32(x * a + np.float64(by)) + F32(d))                    # fma(x, a, y*b), then + d
    plain = F32(F32(F32(F32(x) * F32(a)) + by) + F32(d))
    assert plain == F32(-(2.0 ** -25)) and fused > 0 and fused != plain
    assert not pass_planes(FMA_P, FMA_PLANE)[0] and fused >= 0           # operation by operation the row fails; fused it would pass
    ex, ey, _ = FMA_SPHERE_P.astype(np.float64)
    r2 = FMA_SPHERE[3]
    fused_d = F32(ey * ey + np.float64(F32(F32(ex) * F32(ex))))          # fma(ey, ey, ex*ex)
    plain_d = F32(F32(F32(ex) * F32(ex)) + F32(F32(ey) * F32(ey)))
    assert plain_d == r2 and fused_d == F32(1 + 2.0 ** -11 + 2.0 ** -23) and fused_d > r2
    assert pass_sphere(FMA_SPHERE_P, FMA_SPHERE)[0]                      # operation by operation the row is exactly at the radius; fused it would be outside
    exe = _compile_pred(tmp_path)
    out = subprocess.run([exe], input=f"P 1 {_hex(FMA_P)} {_hex(FMA_PLANE)}\nS {_hex(FMA_SPHERE_P)} {_hex(FMA_SPHERE)}\n", capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0", "1"]
    # the same source built WITH contraction allowed on a target that has the instruction gives the fused answer where the compiler fuses; the
    # library's units are built with -ffp-contract=off and carry the pragma, which this checks in the sources themselves
    assert "-ffp-contract=off" in hb.HIP_FLAGS
    text = open(os.path.join(CSRC, "hnb_export_filter.hip")).read() + open(os.path.join(CSRC, "hnb_filter_pred.h")).read()
    assert text.count("#pragma clang fp contract(off)") >= 3
    import inspect
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_export_filter_code)


# ---- the code objects ---------------------------------------------------------------------------------------------------------------------------
def _rows(path):
    """kernel name -> its resource row, from the code object's notes (not from disassembly)"""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], check=True, capture_output=True, text=True).stdout
    keys = ("group_segment_fixed_size", "kernarg_segment_size", "private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count")
    kernels, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s+\.(" + "|".join(keys) + r"|name):\s+(.*)", line)
        if not m or (m.group(1) == "name" and not m.group(2).strip().startswith("k_")):
            continue
        cur[m.group(1)] = m.group(2).strip()
        if len(cur) == len(keys) + 1:
            name = cur.pop("name")
            kernels[name] = {k: int(v) for k, v in cur.items()}
            cur = {}
    return kernels


FILTER_KERNELS = ["k_export_filter_mark", "k_export_filter_scan", "k_export_filter_compact", "k_export_filter_tile"] + [f"k_export_filter_rows_{v}" for v in (32, 64, 128, 256)]


def test_third_code_object_is_built_carried_and_declares_its_lds_and_no_scratch():
    co = hb.export_filter_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_export_filter.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(FILTER_KERNELS), sorted(rows)
    for name, r in rows.items():
        assert 0 < r["group_segment_fixed_size"] <= 32 * 1024, f"{name}: {r['group_segment_fixed_size']} B of LDS per workgroup"
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
    lds = {n: r["group_segment_fixed_size"] for n, r in rows.items()}
    assert (lds["k_export_filter_rows_32"], lds["k_export_filter_rows_64"], lds["k_export_filter_rows_128"], lds["k_export_filter_rows_256"]) == (256 * 32, 256 * 64, 256 * 128, 128 * 256)
    assert all(lds[n] <= 64 * 8 + 64 * 4 + 8 for n in ("k_export_filter_mark", "k_export_filter_compact", "k_export_filter_tile"))    # the tile's mask words and their prefix
    assert lds["k_export_filter_scan"] == 257 * 4
    assert rows["k_export_filter_rows_32"]["kernarg_segment_size"] == _rows(hb.export_code_path())["k_export_rows_32"]["kernarg_segment_size"]   # ExportArgs did not grow
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    for other in (hb.export_code_path(), hb.export_sort_code_path()):
        assert open(other, "rb").read() in lib                           # three embedded code objects


def test_first_two_code_objects_keep_their_kernels_and_resource_rows():
    """tests/golden/export_code_object_rows.json: the rows of hnb_export.hsaco and hnb_export_sort.hsaco as they were before the third code object
    and the kRowsFiltered branches of the shared gather body existed."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "export_code_object_rows.json")))
    for unit, path in (("hnb_export", hb.export_code_path()), ("hnb_export_sort", hb.export_sort_code_path())):
        rows = _rows(path)
        assert sorted(rows) == sorted(golden[unit]), (unit, sorted(rows))
        for name, want in golden[unit].items():
            assert rows[name] == want, (unit, name, rows[name], want)
    assert len(golden["hnb_export"]) == 5 and len(golden["hnb_export_sort"]) == 23


# ---- the scratch layout ---------------------------------------------------------------------------------------------------------------------------
def test_scratch_layout_sections_do_not_overlap_and_stay_inside(tmp_path):
    src = r'''
    #include <cstdio>
    #include <cstdint>
    #include "hnb_export.h"
    int main() {
        unsigned long long cap;
        while (std::scanf("%llu", &cap) == 1) {
            const hnb::ExportFilterScratch l = hnb::export_filter_scratch_layout((uint32_t)cap);
            std::printf("%u %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", l.tiles, (unsigned long long)l.order_off, (unsigned long long)l.order_bytes,
                        (unsigned long long)l.mask_off, (unsigned long long)l.mask_bytes, (unsigned long long)l.count_off, (unsigned long long)l.count_bytes,
                        (unsigned long long)l.offset_off, (unsigned long long)l.offset_bytes, (unsigned long long)l.state_off, (unsigned long long)l.state_bytes,
                        (unsigned long long)l.total);
        }
        return 0;
    }
    '''
    (tmp_path / "l.cpp").write_text(src)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + CSRC, str(tmp_path / "l.cpp"), "-o", str(tmp_path / "l")])
    caps = [1, 63, 64, 300, 4095, 4096, 4097, 10_000, 135_245, 16_777_216, (1 << 32) - 4096, (1 << 32) - 1]
    out = subprocess.run([str(tmp_path / "l")], input="\n".join(str(c) for c in caps), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(caps)
    for cap, line in zip(caps, out):
        tiles, *rest, total = [int(x) for x in line.split()]
        sections = list(zip(rest[0::2], rest[1::2]))                     # (offset, bytes): order, mask, tile counts, tile offsets, state
        assert tiles == -(-cap // 4096), (cap, tiles)
        order, mask, count, offset, state = sections
        assert order[1] >= 4 * cap and mask[1] >= 8 * -(-cap // 64) and mask[1] == tiles * 512 and count[1] >= 4 * tiles and offset[1] >= 4 * tiles and state[1] >= 4
        end = 0
        for off, size in sections:                                       # in this order, none starting before the one in front of it ends
            assert off >= end and off % 256 == 0 and size > 0, (cap, sections)
            end = off + size
        assert end <= total, (cap, sections, total)
        assert total <= 4 * cap + 520 * tiles + 6 * 256                  # 4 bytes per slot, 520 per tile, the alignment


# ---- the sort's scratch layout and the launch plan of every form (csrc/hnb_export.h), as stand-alone host programs --------------------------------
def _standalone(tmp_path, name, src):
    """g++ alone, with the address and undefined-behaviour sanitizers: the header is plain C++ on the host"""
    (tmp_path / f"{name}.cpp").write_text(src)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                           str(tmp_path / f"{name}.cpp"), "-o", str(tmp_path / name)])
    return str(tmp_path / name)


SORT_ROWS_MAX = 0xFFFFFF00
INSTANCE, PROGRAM = 0, 1


def sort_layout(n_inst, cap, scope):
    """export_sort_scratch_layout restated: (sections, rows, pitch, tiles, groups, vals_off, state_off, gsum_off, hist_off, zero_bytes, total)"""
    rows = n_inst * cap if scope == PROGRAM else cap
    if rows > SORT_ROWS_MAX:
        return (0,) * 11
    sections = 1 if scope == PROGRAM else n_inst
    pitch, tiles = (rows + 63) & ~63, -(-rows // 4096)
    groups = -(-tiles // 32)
    vals_off = sections * pitch * 8
    state_off = 2 * vals_off
    gsum_off = state_off + ((sections * 16 + 255) & ~255)
    hist_off = gsum_off + sections * 8192 * groups
    return (sections, rows, pitch, tiles, groups, vals_off, state_off, gsum_off, hist_off, hist_off - state_off, hist_off + sections * 4096 * tiles)


def test_sort_scratch_layout_sections_are_ordered_aligned_and_the_effect_layout_is_the_one_instance_case(tmp_path):
    assert runtime.SORT_SCOPE_INSTANCE == INSTANCE and runtime.SORT_SCOPE_PROGRAM == PROGRAM
    exe = _standalone(tmp_path, "sl", r"""
    #include <cstdio>
    #include <cstdint>
    #include "hnb_export.h"
    int main() {
        unsigned long long n, cap, scope;
        while (std::scanf("%llu %llu %llu", &n, &cap, &scope) == 3) {
            const hnb::ExportSortScratch l = hnb::export_sort_scratch_layout((uint32_t)n, (uint32_t)cap, (uint32_t)scope);
            std::printf("%u %u %u %u %u %llu %llu %llu %llu %llu %llu\n", l.sections, l.rows, l.pitch, l.tiles, l.groups, (unsigned long long)l.vals_off, (unsigned long long)l.state_off,
                        (unsigned long long)l.gsum_off, (unsigned long long)l.hist_off, (unsigned long long)l.zero_bytes, (unsigned long long)l.total);
        }
        return 0;
    }
    """)
    caps = [1, 63, 64, 300, 4095, 4096, 4097, 10_000, 131_072, 131_073, 16_777_216, SORT_ROWS_MAX]
    cases = [(n, cap, scope) for cap in caps for n in (1, 5) for scope in (INSTANCE, PROGRAM)] + [(1, SORT_ROWS_MAX + 1, INSTANCE), (5, SORT_ROWS_MAX + 1, INSTANCE), (65535, 16_777_216, PROGRAM)]
    out = subprocess.run([exe], input="\n".join("%d %d %d" % c for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (n, cap, scope), line in zip(cases, out):
        got = tuple(int(x) for x in line.split())
        sections, rows, pitch, tiles, groups, vals_off, state_off, gsum_off, hist_off, zero_bytes, total = got
        want_rows = n * cap if scope == PROGRAM else cap
        if want_rows > SORT_ROWS_MAX:
            assert rows == 0, (n, cap, scope, got)                       # refused: 32 bits of pitch do not hold the section
            continue
        assert rows == want_rows and sections == (1 if scope == PROGRAM else n), (n, cap, scope, got)
        assert pitch >= rows and pitch % 64 == 0 and tiles == -(-rows // 4096) and groups == -(-tiles // 32), (n, cap, scope, got)
        # (offset, bytes) in the order of the allocation: keys, vals, state, gsum, hist
        sects = [(0, sections * 2 * pitch * 4), (vals_off, sections * 2 * pitch * 4), (state_off, sections * 16), (gsum_off, sections * 2 * 4 * groups * 1024), (hist_off, sections * 4 * tiles * 1024)]
        end = 0
        for off, size in sects:
            assert off >= end and off % 256 == 0 and size > 0, (n, cap, scope, sects)
            end = off + size
        assert end == total, (n, cap, scope, sects, total)               # total covers hist, and no more
        assert state_off + zero_bytes == hist_off and gsum_off + sects[3][1] == hist_off, (n, cap, scope, got)   # the memset: state and gsum, exactly
        assert got == sort_layout(n, cap, scope), (n, cap, scope, got)
        if n == 1 and scope == INSTANCE:                                 # the closed forms of the effect form's own layout
            p = (cap + 63) & ~63
            assert (pitch, vals_off, state_off, gsum_off, hist_off, total) == (p, 8 * p, 16 * p, 16 * p + 256, 16 * p + 256 + 8192 * groups, 16 * p + 256 + 8192 * groups + 4096 * tiles)
    assert (131_072 // 4096, sort_layout(1, 131_072, INSTANCE)[4], sort_layout(1, 131_073, INSTANCE)[4]) == (32, 1, 2)   # where a second group of tiles starts


def plan_table(form, program, scope, n, cap, stride):
    """The launches of an export as the design states them: ([(kernel, grid x, grid y, argument block, pass)], index of the launch behind the memset or None)"""
    T = -(-cap // 4096)
    v = {32: 0, 64: 1, 128: 2, 256: 3}[stride]
    tile_rows = 128 if v == 3 else 256
    whole = program and form == "sorted" and scope == PROGRAM
    rows = n * cap if whole else cap
    G, Tp = -(-rows // tile_rows), -(-rows // 4096)
    if not program:
        n = 1
    L, memset = [], None
    if program:
        L.append(("kExpOffsets", 1, 1, "offsets", 0))
    if form == "plain":
        L.append((f"kExpRows{v}", G, n, "rows", 0))
    elif form == "filtered":
        if T <= 1:
            L.append(("kExpFilterTile", 1, 1, "filter", 0))
        else:
            L += [("kExpFilterMark", T, 1, "filter", 0), ("kExpFilterScan", 1, 1, "filter", 0), ("kExpFilterCompact", T, 1, "filter", 0)]
        L.append((f"kExpFilterRows{v}", G, 1, "rows", 0))
    elif whole:
        memset = len(L)
        L.append(("kExpSortFill", T, n, "sort", 0))
        for p in range(4):
            L += [("kExpSortHistAll", Tp, 1, "sort+pass", p), ("kExpSortScatterAll", Tp, 1, "sort+pass", p)]
        L.append((f"kExpSortRowsAll{v}", G, 1, "rows", 0))
    else:
        sfx = "Inst" if program else ""
        if T <= 1:
            L.append((f"kExpSortTile{sfx}", 1, n, "sort", 0))
        else:
            memset = len(L)
            L += [(f"kExpSortKeys{sfx}", T, n, "sort", 0), (f"kExpSortScatter{sfx}", T, n, "sort+pass", 0)]
            for p in (1, 2, 3):
                L += [(f"kExpSortHist{sfx}", T, n, "sort+pass", p), (f"kExpSortScatter{sfx}", T, n, "sort+pass", p)]
        L.append((f"kExpSortRows{sfx}{v}", G, n, "rows", 0))
    return L, memset


def test_launch_plan_of_every_form_is_the_designs_table(tmp_path):
    kernels = (["kExpOffsets"] + [f"kExp{f}Rows{s}{v}" for f, s in (("", ""), ("Sort", ""), ("Sort", "Inst"), ("Sort", "All"), ("Filter", "")) for v in range(4)]
               + [f"kExpSort{k}{s}" for s in ("", "Inst") for k in ("Tile", "Keys", "Hist", "Scatter")] + ["kExpSortFill", "kExpSortHistAll", "kExpSortScatterAll"]
               + [f"kExpFilter{k}" for k in ("Tile", "Mark", "Scan", "Compact")])
    assert len(kernels) == len(set(kernels)) == 5 + 23 + 8
    exe = _standalone(tmp_path, "pl", r"""
    #include <cstdio>
    #include <cstdint>
    #include "hnb_export.h"
    using namespace hnb;
    static const char* kernel_name(uint32_t k) {
        switch (k) {
    """ + "\n".join(f'        case {k}: return "{k}";' for k in kernels) + r"""
        }
        return "?";
    }
    int main() {
        static_assert(kExpCullTile == """ + str(len(kernels)) + r""", "every kernel of the first three units has a name here; the fourth's follow");
        static const char* const args[] = {"rows", "sort", "sort+pass", "filter", "offsets"};
        static_assert(kExportArgsRows == 0 && kExportArgsSort == 1 && kExportArgsSortPass == 2 && kExportArgsFilter == 3 && kExportArgsOffsets == 4, "args[]");
        unsigned form, program, scope, n, cap, stride;
        while (std::scanf("%u %u %u %u %u %u", &form, &program, &scope, &n, &cap, &stride) == 6) {
            const ExportPlan pl = export_launch_plan(form, program != 0, scope, n, cap, stride);
            if (pl.n > kExportPlanMax) return 2;
            std::printf("%u %d %llu %llu", pl.n, pl.memset_before == kExportNoMemset ? -1 : (int)pl.memset_before, (unsigned long long)pl.zero_off, (unsigned long long)pl.zero_bytes);
            for (uint32_t i = 0; i < pl.n; ++i) std::printf(" %s %u %u %s %u", kernel_name(pl.launch[i].kernel), pl.launch[i].grid_x, pl.launch[i].grid_y, args[pl.launch[i].args], pl.launch[i].pass);
            std::printf("\n");
        }
        return 0;
    }
    """)
    forms = {"plain": 0, "sorted": 1, "filtered": 2}
    rows_of_the_table = [("plain", 0, INSTANCE), ("plain", 1, INSTANCE), ("sorted", 0, INSTANCE), ("sorted", 1, INSTANCE), ("sorted", 1, PROGRAM), ("filtered", 0, INSTANCE)]
    cases = [(form, program, scope, n, cap, stride) for form, program, scope in rows_of_the_table for cap in (300, 4096, 4097, 10_000) for n in (1, 5) for stride in (32, 256)]
    assert ("sorted", 1, PROGRAM, 5, 300, 32) in cases                   # n * capacity <= 4096: still the fill / hist_all path
    out = subprocess.run([exe], input="\n".join("%d %d %d %d %d %d" % ((forms[c[0]],) + c[1:]) for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for case, line in zip(cases, out):
        form, program, scope, n, cap, stride = case
        w = line.split()
        count, memset, zero_off, zero_bytes = int(w[0]), int(w[1]), int(w[2]), int(w[3])
        got = [(w[i], int(w[i + 1]), int(w[i + 2]), w[i + 3], int(w[i + 4])) for i in range(4, len(w), 5)]
        want, want_memset = plan_table(*case)
        assert count == len(got) <= 12 and got == want, (case, got, want)
        assert memset == (-1 if want_memset is None else want_memset), (case, memset, want_memset)
        if want_memset is not None:
            l = sort_layout(n if program else 1, cap, scope)
            assert (zero_off, zero_bytes) == (l[6], l[9]), (case, zero_off, zero_bytes, l)
    whole_small = dict(zip(cases, out))[("sorted", 1, PROGRAM, 5, 300, 32)].split()
    assert whole_small[4] == "kExpOffsets" and whole_small[9] == "kExpSortFill" and whole_small[1] == "1" and "kExpSortTileInst" not in whole_small
