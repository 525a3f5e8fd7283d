"""The sorted export (hnb_effect_export_sorted, include/hanabi_amd.h "Packed output") without a GPU: the ctypes mirror has the header's layout,
the call fails loudly, the key transform the kernels call (csrc/hnb_sort_key.h) is the order the header states, and the kernels live in a code
object of their own that the library carries - the fat binary knows nothing of them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
A = bh.Attribute


def key_f32(bits):
    """The header's formula, restated: k = b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000)."""
    b = np.asarray(bits, np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def test_ctypes_mirror_has_the_headers_size_and_offsets(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd.h"
    int main(void) { printf("%zu %zu %zu %zu %zu %zu %u %u %u\n", sizeof(HnbExportSort), offsetof(HnbExportSort, key), offsetof(HnbExportSort, attr),
                            offsetof(HnbExportSort, descending), offsetof(HnbExportSort, v), offsetof(HnbExportSort, reserved),
                            HNB_SORT_KEY_DEPTH, HNB_SORT_KEY_DISTANCE, HNB_SORT_KEY_ATTR); return 0; }
    '''
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    S = runtime.ExportSort
    assert got == [C.sizeof(S), S.key.offset, S.attr.offset, S.descending.offset, S.v.offset, S.reserved.offset,
                   runtime.SORT_KEY_DEPTH, runtime.SORT_KEY_DISTANCE, runtime.SORT_KEY_ATTR]
    s = runtime.export_sort("distance", v=(1, 2.5, -3), descending=True)
    assert (s.struct_size, s.key, s.attr, s.descending, list(s.v), s.reserved) == (C.sizeof(S), runtime.SORT_KEY_DISTANCE, 0, 1, [1.0, 2.5, -3.0], 0)
    s = runtime.export_sort("attr", attr=A.AGE.id)
    assert (s.key, s.attr, s.descending, list(s.v)) == (runtime.SORT_KEY_ATTR, A.AGE.id, 0, [0.0, 0.0, 0.0])
    assert runtime.export_sort(runtime.SORT_KEY_DEPTH).key == 0
    assert "hnb_effect_export_sorted" in runtime.ABI_SYMBOLS


def test_call_fails_loudly_on_null_arguments():
    lib = runtime.load_library()
    d = runtime.export_desc([(A.POSITION.id, 0)], 0x1000, 16, 1)
    s = runtime.export_sort("depth", v=(0, 0, 1))
    assert lib.hnb_effect_export_sorted(None, C.byref(d), C.byref(s)) == -1 and b"NULL" in lib.hnb_last_error()
    assert lib.hnb_effect_export_sorted(None, None, None) == -1 and b"NULL" in lib.hnb_last_error()
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL sort is refused first
    assert lib.hnb_effect_export_sorted(fake, C.byref(d), None) == -1 and b"NULL" in lib.hnb_last_error()


EDGES = [0x00000000, 0x80000000,                 # +-0
         0x00000001, 0x80000001,                 # +-denormal min
         0x007FFFFF, 0x807FFFFF,                 # +-denormal max
         0x00800000, 0x80800000,                 # +-FLT_MIN
         0x3F800000, 0xBF800000,                 # +-1
         0x7F7FFFFF, 0xFF7FFFFF,                 # +-FLT_MAX
         0x7F800000, 0xFF800000,                 # +-inf
         0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFFFFFFF,      # quiet NaNs of both signs
         0x7F800001, 0xFF800001, 0x7FA00000, 0xFFBFFFFF]      # signalling NaNs of both signs


def test_key_transform_is_the_headers_total_order(tmp_path):
    """A stand-alone C++ program over the header the kernels include prints the key of every pattern: equal to the numpy restatement, and
    strictly monotonic in the float order (with -0 < +0) over everything that is no NaN; NaNs sort outside the infinities by their sign."""
    src = r'''
    #include <cstdio>
    #include <cstdint>
    #include "hnb_sort_key.h"
    int main() {
        unsigned b;
        while (std::scanf("%x", &b) == 1)
            std::printf("%08x %08x %08x %08x\n", hnb::sort_key_f32(b), hnb::sort_key_of(b, true, false), hnb::sort_key_of(b, true, true), hnb::sort_key_of(b, false, true));
        return 0;
    }
    '''
    (tmp_path / "k.cpp").write_text(src)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "bevy_hanabi_amd", "csrc"), str(tmp_path / "k.cpp"), "-o", str(tmp_path / "k")])
    rng = np.random.default_rng(11)
    bits = np.concatenate([np.array(EDGES, np.uint32), rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)])
    out = subprocess.run([str(tmp_path / "k")], input="\n".join(f"{int(b):x}" for b in bits), capture_output=True, text=True, check=True).stdout
    got = np.array([[int(x, 16) for x in line.split()] for line in out.splitlines()], np.uint64).astype(np.uint32)
    assert got.shape == (len(bits), 4)
    k = key_f32(bits)
    np.testing.assert_array_equal(got[:, 0], k)
    np.testing.assert_array_equal(got[:, 1], k)
    np.testing.assert_array_equal(got[:, 2], ~k)                # descending: the complement
    np.testing.assert_array_equal(got[:, 3], ~bits)             # not f32: the bits themselves
    f = bits.view(np.float32)
    num = ~np.isnan(f)
    # the float order with the sign of zero as a tie-break, as a sortable pair
    order = np.lexsort((~np.signbit(f[num]), f[num]))
    fk, kk = f[num][order], k[num][order].astype(np.int64)
    same = (fk[1:] == fk[:-1]) & (np.signbit(fk[1:]) == np.signbit(fk[:-1]))
    assert ((kk[1:] > kk[:-1]) | same).all() and (kk[1:][same] == kk[:-1][same]).all()
    assert key_f32(0x80000000) + 1 == key_f32(0x00000000)                                   # -0 directly below +0
    nan_neg, nan_pos = k[~num & (bits >> 31 == 1)], k[~num & (bits >> 31 == 0)]
    assert len(nan_neg) and len(nan_pos)
    assert nan_neg.max() < key_f32(0xFF800000) and nan_pos.min() > key_f32(0x7F800000)      # -NaN < -inf, +inf < +NaN


def _notes(path):
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s+\.(group_segment_fixed_size|private_segment_fixed_size|name):\s+(.*)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2).strip()
        if len(cur) == 3:
            kernels[cur["name"]] = (int(cur["group_segment_fixed_size"]), int(cur["private_segment_fixed_size"]))
            cur = {}
    return kernels


def test_sort_code_object_is_built_carried_and_declares_its_lds_and_no_scratch(tmp_path):
    co = hb.export_sort_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_export_sort.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    kernels = _notes(co)
    assert all(k.startswith("k_export_sort_") for k in kernels), kernels
    for name in ("k_export_sort_keys", "k_export_sort_hist", "k_export_sort_scatter", "k_export_sort_tile",
                 "k_export_sort_rows_32", "k_export_sort_rows_64", "k_export_sort_rows_128", "k_export_sort_rows_256"):
        assert name in kernels, (name, sorted(kernels))
    for name, (lds, scratch) in kernels.items():
        assert lds <= 32 * 1024, f"{name}: {lds} B of LDS per workgroup"
        assert scratch == 0, f"{name}: {scratch} B of scratch per thread"
    assert kernels["k_export_sort_keys"][0] == 4 * 256 * 4                 # the four digit histograms, nothing else
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    # ... while the library's fat binary holds no export kernel at all
    fat, fco = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", hb.runtime_lib_path(), fat], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={fco}"], check=True)
    names = list(_notes(fco))
    assert len(names) > 20 and not [n for n in names if "export" in n], [n for n in names if "export" in n]
