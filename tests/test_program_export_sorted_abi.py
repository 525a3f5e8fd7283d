"""The sorted program export (hnb_program_export_sorted, include/hanabi_amd.h "Packed output") without a GPU: the scope constants of the header are
the binding's, the call fails loudly, the (instance, slot) value of the program scope (csrc/hnb_export.h) packs, unpacks, orders and refuses as the
header states, and the new kernels live in the second code object with no scratch."""
import ctypes as C
import os
import subprocess

from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import runtime
from test_export_sorted_abi import A, ROOT, _notes

NEW_KERNELS = (["k_export_sort_keys_inst", "k_export_sort_hist_inst", "k_export_sort_scatter_inst", "k_export_sort_tile_inst",
                "k_export_sort_fill", "k_export_sort_hist_all", "k_export_sort_scatter_all"]
               + [f"k_export_sort_rows_{scope}_{v}" for scope in ("inst", "all") for v in (32, 64, 128, 256)])


def test_scope_constants_and_symbol(tmp_path):
    src = r'''
    #include <stdio.h>
    #include "hanabi_amd.h"
    int main(void) { printf("%u %u %zu %zu\n", HNB_SORT_SCOPE_INSTANCE, HNB_SORT_SCOPE_PROGRAM, sizeof(HnbExportDesc), sizeof(HnbExportSort));
                     return hnb_program_export_sorted == 0; }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    assert got == [runtime.SORT_SCOPE_INSTANCE, runtime.SORT_SCOPE_PROGRAM, C.sizeof(runtime.ExportDesc), C.sizeof(runtime.ExportSort)]
    assert runtime.SORT_SCOPES == {"instance": 0, "program": 1}
    assert "hnb_program_export_sorted" in runtime.ABI_SYMBOLS
    assert hasattr(runtime.load_library(), "hnb_program_export_sorted")
    assert "there is no program form" not in open(os.path.join(ROOT, "include", "hanabi_amd.h")).read()


def test_call_fails_loudly_on_null_arguments():
    lib = runtime.load_library()
    d = runtime.export_desc([(A.POSITION.id, 0)], 0x1000, 16, 1)
    s = runtime.export_sort("depth", v=(0, 0, 1))
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for args in ((None, C.byref(d), C.byref(s)), (fake, None, C.byref(s)), (fake, C.byref(d), None), (None, None, None)):
        for scope in (0, 1, 2):
            assert lib.hnb_program_export_sorted(*args, scope, None) == -1 and b"NULL" in lib.hnb_last_error()


def test_instance_slot_value_packs_orders_and_refuses(tmp_path):
    """A stand-alone C++ program over the header the kernels include. Per capacity: slot_bits, the largest instance count that fits and whether
    that count and the next one fit; then pack -> unpack of pairs at the edges of both ranges, printed in the order of the pairs."""
    src = r'''
    #include <cstdio>
    #include <cstdint>
    #include "hnb_export.h"
    using namespace hnb;
    int main() {
        const uint64_t caps[] = {1, 2, 3, 4096, 4097, 65536, 1ull << 31};
        for (uint64_t cap64 : caps) {
            const uint32_t cap = (uint32_t)cap64, bits = export_sort_slot_bits(cap);
            const uint64_t limit = (1ull << 32) >> bits;                      // n_inst << bits <= 2^32
            std::printf("C %u %u %llu %d %d %d\n", cap, bits, (unsigned long long)limit, (int)export_sort_pack_fits(limit, cap), (int)export_sort_pack_fits(limit + 1, cap),
                        (int)export_sort_pack_fits(1, cap));
            const uint32_t last_k = (uint32_t)(limit - 1), last_s = cap - 1u;
            const uint32_t ks[] = {0u, 1u, last_k / 2u, last_k - (last_k ? 1u : 0u), last_k};
            const uint32_t ss[] = {0u, 1u, last_s / 2u, last_s - (last_s ? 1u : 0u), last_s};
            for (uint32_t k : ks) for (uint32_t s : ss) {
                if (k > last_k || s > last_s) continue;
                const uint32_t v = export_sort_pack(k, s, bits);
                std::printf("P %u %u %u %u %u\n", k, s, v, export_sort_unpack_instance(v, bits), export_sort_unpack_slot(v, bits));
            }
        }
        return 0;
    }
    '''
    (tmp_path / "p.cpp").write_text(src)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "bevy_hanabi_amd", "csrc"), str(tmp_path / "p.cpp"), "-o", str(tmp_path / "p")])
    out = subprocess.check_output([str(tmp_path / "p")], text=True).splitlines()
    want_bits = {1: 0, 2: 1, 3: 2, 4096: 12, 4097: 13, 65536: 16, 1 << 31: 31}
    caps, pairs = [], []
    for line in out:
        tag, *nums = line.split()
        nums = [int(x) for x in nums]
        if tag == "C":
            cap, bits, limit, fits_at, fits_past, fits_one = nums
            assert bits == want_bits[cap] and (1 << bits) >= cap and (bits == 0 or (1 << (bits - 1)) < cap)      # ceil(log2(capacity))
            assert limit << bits == 1 << 32 and (fits_at, fits_past, fits_one) == (1, 0, 1), line               # flips exactly at n_inst << slot_bits > 2^32
            if pairs:
                caps.append(pairs)
            pairs = []
        else:
            k, s, v, uk, us = nums
            assert (uk, us) == (k, s) and v < 1 << 32, line                                                      # pack -> unpack is the identity
            pairs.append(((k, s), v))
    caps.append(pairs)
    assert len(caps) == len(want_bits)
    for pairs in caps:
        assert len(pairs) >= 1
        by_pair = sorted(set(pairs))
        values = [v for _, v in by_pair]
        assert values == sorted(values) and len(set(values)) == len(values), pairs                              # ordered like the pairs, no two alike


def test_new_kernels_are_in_the_second_code_object_without_scratch():
    co = hb.export_sort_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_export_sort.hip into it"
    kernels = _notes(co)
    for name in NEW_KERNELS:
        assert name in kernels, (name, sorted(kernels))
        lds, scratch = kernels[name]
        assert lds <= 32 * 1024, f"{name}: {lds} B of LDS per workgroup"
        assert scratch == 0, f"{name}: {scratch} B of scratch per thread"
    assert kernels["k_export_sort_keys_inst"][0] == kernels["k_export_sort_keys"][0]            # the same bodies: the same LDS
    assert kernels["k_export_sort_scatter_all"][0] == kernels["k_export_sort_scatter"][0]
    assert open(co, "rb").read() in open(hb.runtime_lib_path(), "rb").read()                    # the library carries that object
