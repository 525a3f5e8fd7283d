"""The packed input (hnb_effect_import, include/hanabi_amd_import.h) without a GPU: header, ctypes mirror and INTEGRATION.md agree on HnbImportDesc
and the prototype, and the two older headers declare what they declared; the plain C++ of csrc/hnb_import.h - the launch plan, the range test of an
id and the check of a description - compiled as a stand-alone host program under the address and undefined-behaviour sanitizers gives what a
restatement in Python gives; the eight kernels live in a code object of their own with no scratch, no spills and at most 32 KiB of LDS; NULL
arguments fail loudly."""
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

IMPORT_KERNELS = [f"k_import_{m}_{v}" for m in ("rows", "ids") for v in (32, 64, 128, 256)]
ROWS, IDS = 0, 1


# ---- the binding ------------------------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirror_header_and_integration_agree_on_the_struct_and_the_prototype(tmp_path):
    members = ["struct_size", "n_fields", "record_stride", "mode", "flags", "reserved", "src", "src_capacity_records", "src_count", "out_count", "fields"]
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd_import.h"
    int main(void) {
        int (*f)(HnbEffect*, const HnbImportDesc*) = hnb_effect_import;
        printf("%zu", sizeof(HnbImportDesc));
    ''' + "\n".join(f'        printf(" %zu", offsetof(HnbImportDesc, {m}));' for m in members) + r'''
        printf(" %u %u %zu\n", HNB_IMPORT_ROWS, HNB_IMPORT_IDS, sizeof(((HnbImportDesc*)0)->fields) / sizeof(HnbExportField));
        return f == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    S = runtime.ImportDesc
    assert got == [184, 0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 0, 1, 16]
    assert [C.sizeof(S)] + [getattr(S, m).offset for m in members] == got[:12]
    assert (runtime.IMPORT_ROWS, runtime.IMPORT_IDS, runtime.EXPORT_MAX_FIELDS) == tuple(got[12:])
    d = runtime.import_desc([(A.POSITION.id, 4), (A.ID.id, 0)], 0x1000, 16, 7, runtime.IMPORT_IDS, 0x2000, 0x3000)
    assert (d.struct_size, d.n_fields, d.record_stride, d.mode, d.flags, d.reserved, d.src, d.src_capacity_records, d.src_count, d.out_count) == (184, 2, 16, 1, 0, 0, 0x1000, 7, 0x2000,
                                                                                                                                                0x3000)
    assert (d.fields[0].attr, d.fields[0].reserved, d.fields[0].dst_offset, d.fields[1].attr, d.fields[1].dst_offset) == (A.POSITION.id, 0, 4, A.ID.id, 0)
    d = runtime.import_desc([(A.AGE.id, 0)], 0x1000, 4, 1, "rows")
    assert (d.mode, d.src_count, d.out_count) == (0, None, None)
    lib = runtime.load_library()
    assert runtime.ABI_IMPORT_SYMBOLS == ["hnb_effect_import"] and hasattr(lib, "hnb_effect_import")
    assert lib.hnb_effect_import.argtypes == [C.c_void_p, C.POINTER(runtime.ImportDesc)]
    assert list(inspect.signature(runtime.Effect.import_records).parameters) == ["self", "fields", "src_ptr", "stride", "capacity_records", "mode", "src_count_ptr", "out_count_ptr"]
    full = open(os.path.join(ROOT, "include", "hanabi_amd_import.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    m = re.search(r"int\s+hnb_effect_import\s*\(([^)]*)\)\s*;", header)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["HnbEffect* fx", "const HnbImportDesc* desc"]
    # the header pins: every header declares exactly its own symbols
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", header)) == set(runtime.ABI_IMPORT_SYMBOLS)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", main)) == set(runtime.ABI_SYMBOLS) and len(runtime.ABI_SYMBOLS) == 61 and "hnb_effect_import" not in runtime.ABI_SYMBOLS
    binned = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd_binned.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(hnb_[a-z0-9_]+)\s*\(", binned)) == set(runtime.ABI_BINNED_SYMBOLS) == {"hnb_effect_export_binned"}
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"\bfn hnb_effect_import\(([^)]*)\) -> c_int;", txt)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["fx: *mut HnbEffect", "desc: *const HnbImportDesc"]
    bound = set(re.findall(r"pub fn (hnb_[a-z0-9_]+)\(", txt))             # (the `pub fn` set mirrors hanabi_amd.h and the host header: tests/test_abi.py)
    assert set(runtime.ABI_SYMBOLS) <= bound and "hnb_effect_import" not in bound and "hnb_effect_export_binned" not in bound
    m = re.search(r"#\[repr\(C\)\]\s*pub struct HnbImportDesc \{(.*?)\}", txt, flags=re.S)
    assert m, "INTEGRATION.md mirrors the struct"
    rust = [" ".join(line.split("//")[0].split()).rstrip(",") for line in m.group(1).splitlines() if line.split("//")[0].strip()]
    assert rust == ["pub struct_size: u32", "pub n_fields: u32", "pub record_stride: u32", "pub mode: u32", "pub flags: u32", "pub reserved: u32", "pub src: *const c_void",
                    "pub src_capacity_records: u64", "pub src_count: *const u32", "pub out_count: *mut u32", "pub fields: [HnbExportField; 16]"]
    for word in ("a program form", "spawning or killing", "any transform of the values", "a defined winner among duplicate ids",       # out of scope, said where a caller reads it
                 "every stored dword is a\n *                    whole dword of one of the records", "No host synchronisation and no readback"):
        assert word in full, word


def test_call_fails_loudly_on_null_arguments_and_without_a_device():
    """Up to the device check: the NULL refusals come before anything is dereferenced, loaded or enqueued. The refusals of a description's members
    need an effect, and an effect a device: the stand-alone program below holds them, and tests/test_gpu_import.py on a live effect."""
    lib = runtime.load_library()
    d = runtime.import_desc([(A.POSITION.id, 0)], 0x1000, 16, 1)
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for args in ((None, C.byref(d)), (fake, None), (None, None)):
        assert lib.hnb_effect_import(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to import into, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- csrc/hnb_import.h as a stand-alone host program under the sanitizers ------------------------------------------------------------------------------
ERRORS = ["Ok", "ErrStructSize", "ErrFieldCount", "ErrFlags", "ErrReserved", "ErrMode", "ErrStride", "ErrSrc", "ErrCountPtr", "ErrFieldReserved", "ErrAttr", "ErrNotInLayout",
          "ErrFieldPlace", "ErrOverlap", "ErrIdInRows", "ErrIdCount", "ErrCapacity"]
LAYOUT = [(A.POSITION.id, 3), (A.VELOCITY.id, 3), (A.AGE.id, 1), (A.LIFETIME.id, 1), (A.COLOR.id, 1), (A.HDR_COLOR.id, 4), (A.SIZE2.id, 2)]     # what the check is given: (attr, ncomp)

HOST_SRC = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "hnb_import.h"
using namespace hnb;
""" + "\n".join(f"static_assert(kImport{n} == {i}, \"ImportDescError\");" for i, n in enumerate(ERRORS)) + r"""
static_assert(kImportDescErrorCount == """ + str(len(ERRORS)) + r""", "ImportDescError");
static_assert(sizeof(HnbImportDesc) == 184 && kImportKernelCount == 8 && kImportPlanMax == 3, "hnb_import.h");
static_assert(kExpKernelCount == 48 && kExportUnitCount == 6 && kExportArgsCullProg == 7, "hnb_export.h is what it was");
static const ImportLayoutAttr kLayout[] = {""" + ", ".join("{%d, %d}" % l for l in LAYOUT) + r"""};
int main() {
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (!std::strcmp(what, "names")) {
            for (uint32_t i = 0; i < kImportKernelCount; ++i) std::printf("%u:%s ", kImportKernelNames[i].kernel, kImportKernelNames[i].name);
            std::printf("\n");
        } else if (!std::strcmp(what, "plan")) {
            unsigned cap, stride, mode, mat, cnt; unsigned long long src_cap;
            if (std::scanf("%u %u %u %llu %u %u", &cap, &stride, &mode, &src_cap, &mat, &cnt) != 6) return 1;
            const ImportPlan pl = import_launch_plan(cap, stride, mode, src_cap, mat != 0, cnt != 0);
            if (pl.n > kImportPlanMax) return 2;
            std::printf("%u", pl.n);
            for (uint32_t i = 0; i < pl.n; ++i) {
                const ImportLaunch& l = pl.launch[i];
                if (l.step == kImportStepScatter) std::printf(" %s %u", l.kernel < kImportKernelCount ? kImportKernelNames[l.kernel].name : "?", l.grid_x);
                else std::printf(" %s", l.step == kImportStepMaterialise ? "materialise" : l.step == kImportStepZeroCounts ? "memset" : "?");
            }
            std::printf("\n");
        } else if (!std::strcmp(what, "id")) {
            unsigned id, base, cap;
            if (std::scanf("%u %u %u", &id, &base, &cap) != 3) return 1;
            uint32_t slot = 0;
            const bool ok = import_slot_of_id(id, base, cap, &slot);
            std::printf("%d %u\n", ok ? 1 : 0, slot);
        } else if (!std::strcmp(what, "desc")) {
            HnbImportDesc d;
            std::memset(&d, 0, sizeof d);
            unsigned long long src, src_cap, src_count, out_count; unsigned listed;
            if (std::scanf("%u %u %u %u %u %u %llx %llu %llx %llx %u", &d.struct_size, &d.n_fields, &d.record_stride, &d.mode, &d.flags, &d.reserved, &src, &src_cap, &src_count,
                           &out_count, &listed) != 11 || listed > HNB_EXPORT_MAX_FIELDS) return 1;
            d.src = (const void*)(uintptr_t)src; d.src_capacity_records = src_cap; d.src_count = (const uint32_t*)(uintptr_t)src_count; d.out_count = (uint32_t*)(uintptr_t)out_count;
            for (unsigned f = 0; f < listed; ++f) {
                unsigned attr, reserved, off;
                if (std::scanf("%u %u %u", &attr, &reserved, &off) != 3) return 1;
                d.fields[f].attr = (uint16_t)attr; d.fields[f].reserved = (uint16_t)reserved; d.fields[f].dst_offset = off;
            }
            const ImportCheck c = import_check_desc(d, kLayout, sizeof kLayout / sizeof *kLayout);
            if (c.error >= kImportDescErrorCount || !import_error_text(c.error)[1]) return 3;
            std::printf("%u %u %u %u %d", c.error, c.field, c.n_payload, c.id_dw, c.has_age ? 1 : 0);
            for (uint32_t f = 0; f < c.n_payload; ++f) std::printf(" %u %u %u", c.payload[f].layout_index, c.payload[f].src_dw, c.payload[f].ncomp);
            std::printf("\n");
        } else return 4;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    return _standalone(tmp_path_factory.mktemp("import_host"), "imp", HOST_SRC)


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()      # (a sanitizer report ends the program with an error)
    assert len(out) == len(lines)
    return out


def import_plan_table(cap, stride, mode, src_cap, materialise, has_out_count):
    """The launches of an import as DESIGN.md "Packed input" lists them: (materialise) + (IDS with an out_count: memset) + the scatter, whose grid is
    sized from the capacity (ROWS) or from src_capacity_records (IDS, at most 2^32 - 1; no kernel for 0)"""
    v = 32 if stride <= 32 else 64 if stride <= 64 else 128 if stride <= 128 else 256
    tile = 128 if v == 256 else 256
    rows = min(src_cap, 0xFFFFFFFF) if mode == IDS else cap
    L = []
    if materialise:
        L.append("materialise")
    if mode == IDS and has_out_count:
        L.append("memset")
    if rows:
        L += [f"k_import_{'ids' if mode == IDS else 'rows'}_{v}", str(-(-rows // tile))]
    return L


def test_launch_plan_is_the_designs_table(host_exe):
    assert _ask(host_exe, ["names"])[0].split() == [f"{i}:{n}" for i, n in enumerate(IMPORT_KERNELS)]
    caps = (1, 256, 257, 4096, 4097, 10_000, 2 ** 32 - 1)
    cases = [(cap, stride, mode, src_cap, mat, cnt) for cap in caps for stride in (4, 32, 36, 132, 256) for mode in (ROWS, IDS) for mat in (0, 1) for cnt in (0, 1)
             for src_cap in {0, 1, cap, cap + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40}]
    out = _ask(host_exe, ["plan %d %d %d %d %d %d" % c for c in cases])
    for case, line in zip(cases, out):
        w = line.split()
        want = import_plan_table(*case)
        assert int(w[0]) == len(want) - (1 if want and want[-1].isdigit() else 0) <= 3 and w[1:] == want, (case, w, want)
    # the edges by hand: one workgroup up to a tile, 128-row tiles above 128 bytes, ROWS never sized from the source, IDS never from the capacity
    ask = lambda *c: _ask(host_exe, ["plan %d %d %d %d %d %d" % c])[0].split()
    assert ask(256, 32, ROWS, 7, 0, 1) == ["1", "k_import_rows_32", "1"] and ask(257, 32, ROWS, 7, 0, 1) == ["1", "k_import_rows_32", "2"]
    assert ask(257, 132, ROWS, 7, 0, 0) == ["1", "k_import_rows_256", "3"] and ask(4097, 128, ROWS, 0, 0, 0) == ["1", "k_import_rows_128", "17"]
    assert ask(10_000, 36, IDS, 257, 1, 1) == ["3", "materialise", "memset", "k_import_ids_64", "2"] and ask(10_000, 36, IDS, 0, 0, 1) == ["1", "memset"]
    assert ask(2 ** 32 - 1, 256, ROWS, 1, 1, 1) == ["2", "materialise", "k_import_rows_256", str(2 ** 25)] and ask(1, 4, IDS, 2 ** 40, 0, 0) == ["1", "k_import_ids_32", str(2 ** 24)]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Packed input (`hnb_effect_import`)" in design
    sec = design[design.index("Packed input (`hnb_effect_import`)"):]
    for word in ("k_materialise_age", "hipMemsetAsync", "k_import_rows_", "k_import_ids_", "ceil(capacity / tile_rows)", "ceil(min(src_capacity_records, 2^32 - 1) / tile_rows)"):
        assert word in sec, word


def test_slot_of_an_id_is_wrap_safe(host_exe):
    cases = []
    for base in (0, 7, 2 ** 32 - 5):
        for cap in (1, 300, 4097):
            lo, hi = base, (base + cap) % 2 ** 32                       # the range is [lo, hi), through 2^32 for the last base
            for id_ in {(lo - 1) % 2 ** 32, lo, (lo + 1) % 2 ** 32, (hi - 1) % 2 ** 32, hi, (hi + 1) % 2 ** 32, 0, 2 ** 32 - 1}:
                cases.append((id_, base, cap))
    out = _ask(host_exe, ["id %d %d %d" % c for c in cases])
    inside = 0
    for (id_, base, cap), line in zip(cases, out):
        slot = (id_ - base) % 2 ** 32
        assert [int(x) for x in line.split()] == [1 if slot < cap else 0, slot], (id_, base, cap, line)
        inside += slot < cap
    assert 20 < inside < len(cases) - 20
    # by hand: one below the base is outside (it wraps to 2^32 - 1), the base is slot 0, base + capacity is outside, and a base near 2^32 runs through 0
    assert _ask(host_exe, ["id 6 7 300", "id 7 7 300", "id 306 7 300", "id 307 7 300", "id 4294967295 4294967291 10", "id 0 4294967291 10", "id 4 4294967291 10", "id 5 4294967291 10",
                           "id 4294967290 4294967291 10", "id 4294967295 0 4294967295"]) == ["0 4294967295", "1 0", "1 299", "0 300", "1 4", "1 5", "1 9", "0 10", "0 4294967295", "0 4294967295"]


def _desc(fields, stride=32, mode=ROWS, struct_size=184, n_fields=None, flags=0, reserved=0, src=0x7000, src_cap=100, src_count=0, out_count=0):
    fields = [(f[0], f[2] if len(f) > 2 else 0, f[1]) for f in fields]          # (attr, offset[, reserved]) -> attr reserved offset
    listed = fields[:16]
    return "desc %d %d %d %d %d %d %x %d %x %x %d " % (struct_size, len(fields) if n_fields is None else n_fields, stride, mode, flags, reserved, src, src_cap, src_count, out_count,
                                                      len(listed)) + " ".join("%d %d %d" % f for f in listed)


def test_description_check_refuses_what_the_header_lists_and_accepts_the_edges(host_exe):
    P, V, AGE, LIFE, HDR, S2, ID = A.POSITION.id, A.VELOCITY.id, A.AGE.id, A.LIFETIME.id, A.HDR_COLOR.id, A.SIZE2.id, A.ID.id
    pv = [(P, 0), (V, 12)]
    refused = [
        ("ErrNotInLayout", 1, _desc([(P, 0), (A.SIZE.id, 12)])),                       # an attribute the layout lacks
        ("ErrAttr", 0, _desc([(A.PARTICLE_COUNTER.id, 0)])),
        ("ErrAttr", 1, _desc([(P, 0), (39, 12)])),                                     # no such attribute
        ("ErrOverlap", 1, _desc([(P, 0), (AGE, 8)])),
        ("ErrOverlap", 2, _desc([(ID, 0), (P, 4), (HDR, 12)], mode=IDS)),
        ("ErrFieldPlace", 0, _desc([(AGE, 2)])),                                       # not dword aligned
        ("ErrFieldPlace", 1, _desc([(P, 0), (V, 24)])),                                # ends past the stride
        ("ErrFieldPlace", 0, _desc([(HDR, 244)], stride=256)),
        ("ErrFieldPlace", 0, _desc([(AGE, 0xFFFFFFFC)])),                              # (the end is taken in 64 bits)
        ("ErrStride", 0, _desc(pv, stride=34)), ("ErrStride", 0, _desc([(AGE, 0)], stride=260)), ("ErrStride", 0, _desc([(AGE, 0)], stride=0)),
        ("ErrSrc", 0, _desc(pv, src=0)), ("ErrSrc", 0, _desc(pv, src=0x7004)), ("ErrSrc", 0, _desc(pv, src=0x7008)),
        ("ErrCountPtr", 0, _desc(pv, src_count=0x8002)), ("ErrCountPtr", 0, _desc(pv, out_count=0x8001)),
        ("ErrFieldCount", 0, _desc([])), ("ErrFieldCount", 0, _desc([(AGE, 4 * i) for i in range(17)], stride=128)), ("ErrFieldCount", 0, _desc(pv, n_fields=0xFFFFFFFF)),
        ("ErrFlags", 0, _desc(pv, flags=1)), ("ErrReserved", 0, _desc(pv, reserved=1)), ("ErrFieldReserved", 1, _desc([(P, 0, 0), (V, 12, 1)])),
        ("ErrStructSize", 0, _desc(pv, struct_size=168)), ("ErrStructSize", 0, _desc(pv, struct_size=0)), ("ErrStructSize", 0, _desc(pv, struct_size=192)),
        ("ErrMode", 0, _desc(pv, mode=2)), ("ErrMode", 0, _desc(pv, mode=0xFFFFFFFF)),
        ("ErrIdInRows", 1, _desc([(P, 0), (ID, 12)])),                                 # the ID as a field of ROWS
        ("ErrIdCount", 0, _desc(pv, mode=IDS)),                                        # IDS: no ID ...
        ("ErrIdCount", 0, _desc([(ID, 0), (P, 4), (ID, 16)], mode=IDS)),               # ... or two
        ("ErrCapacity", 0, _desc([(ID, 0)], stride=4, mode=IDS, src_cap=2 ** 32)),     # IDS reads src_capacity_records records when there is no src_count
    ]
    out = _ask(host_exe, [r[2] for r in refused])
    for (err, field, line), got in zip(refused, out):
        w = [int(x) for x in got.split()]
        assert (ERRORS[w[0]], w[1]) == (err, field), (line, got)
    assert {r[0] for r in refused} == set(ERRORS[1:])                                  # every refusal occurred
    legal = [
        (_desc([(P, 0), (AGE, 12), (LIFE, 16), (V, 20)]), [0, 0, 4, 0, 1, 0, 0, 3, 2, 3, 1, 3, 4, 1, 1, 5, 3]),         # payload: (layout index, source dword, ncomp)
        (_desc([(V, 20), (P, 8)], stride=32), [0, 0, 2, 0, 0, 1, 5, 3, 0, 2, 3]),      # a field ending exactly at the stride; fields in any order
        (_desc([(AGE, 0)], stride=4), [0, 0, 1, 0, 1, 2, 0, 1]),                       # stride 4
        (_desc([(LIFE, 252)], stride=256), [0, 0, 1, 0, 0, 3, 63, 1]),                 # the last dword of the largest record
        (_desc([(HDR, 240), (S2, 0)], stride=256), [0, 0, 2, 0, 0, 5, 60, 4, 6, 0, 2]),
        (_desc([(ID, 0)], stride=4, mode=IDS), [0, 0, 0, 0, 0]),                       # IDS: the ID as only field
        (_desc([(P, 0), (ID, 12), (AGE, 16)], stride=20, mode=IDS, src_cap=2 ** 32 - 1), [0, 0, 2, 3, 1, 0, 0, 3, 2, 4, 1]),
        (_desc([(ID, 4)], stride=8, mode=IDS, src_cap=2 ** 40, src_count=0x8004), [0, 0, 0, 1, 0]),                      # with a src_count the capacity is only a clamp
        (_desc(pv, src_cap=2 ** 63, src_count=0x8000, out_count=0x8008), [0, 0, 2, 0, 0, 0, 0, 3, 1, 3, 3]),
        (_desc([(AGE, 4 * i) for i in range(1)] + [(LIFE, 4)], stride=8), [0, 0, 2, 0, 1, 2, 0, 1, 3, 1, 1]),
    ]
    out = _ask(host_exe, [l[0] for l in legal])
    for (line, want), got in zip(legal, out):
        assert [int(x) for x in got.split()] == want, (line, got)
    every = _desc([(ID, 0)] + [(a, 4 + 16 * i) for i, a in enumerate([P, V, AGE, LIFE, A.COLOR.id, HDR, S2])], stride=128, mode=IDS)    # every attribute of the layout
    w = [int(x) for x in _ask(host_exe, [every])[0].split()]
    assert w[:5] == [0, 0, 7, 0, 1] and w[5::3] == list(range(7))


# ---- the code object --------------------------------------------------------------------------------------------------------------------------------
def test_code_object_is_gfx950_embedded_and_holds_the_named_kernels_without_scratch_or_spills():
    co = hb.import_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_import.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    named = re.findall(r'"(k_import_[a-z0-9_]+)"', open(os.path.join(CSRC, "hnb_import.h")).read())
    assert named == IMPORT_KERNELS and sorted(rows) == sorted(named), sorted(rows)                 # exactly the instantiations hnb_import.h names
    for name, r in rows.items():
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)                           # eight waves per SIMD stay possible
        assert r["group_segment_fixed_size"] <= 32 * 1024, (name, r)
    lds = {n: r["group_segment_fixed_size"] for n, r in rows.items()}      # the image alone: the export's four variants, in both modes
    export_rows = _rows(hb.export_code_path())
    for m in ("rows", "ids"):
        for v in (32, 64, 128, 256):
            assert lds[f"k_import_{m}_{v}"] == (128 if v == 256 else 256) * v == export_rows[f"k_export_rows_{v}"]["group_segment_fixed_size"]
    assert len({r["kernarg_segment_size"] for r in rows.values()}) == 1   # one ImportArgs by value
    src = open(os.path.join(CSRC, "hnb_import.hip")).read()
    assert len(re.findall(r'extern "C" __global__ void __launch_bounds__\(256\)[^\n]* k_import_', src)) == len(re.findall(r"__global__", src)) == 8
    assert "asm" not in src and "atomicAdd(a.out_count" in src and not re.search(r"atomic(Add|Max|Min|Exch|CAS)\s*\(\s*(?!a\.out_count)", src)      # integer adds on the counts alone
    assert hb.IMPORT_CODE_OBJECTS == (hb.build_import_code,) and hb.build_import_code not in hb.EXPORT_CODE_OBJECTS + hb.BINNED_CODE_OBJECTS + hb.QUERY_CODE_OBJECTS
    assert "IMPORT_CODE_OBJECTS" in inspect.getsource(hb.build_runtime)
    # the older tuples are what they were
    assert hb.EXPORT_CODE_OBJECTS == (hb.build_export_code, hb.build_export_sort_code, hb.build_export_filter_code, hb.build_export_cull_code, hb.build_export_filter_prog_code,
                                      hb.build_export_cull_prog_code)
    assert hb.BINNED_CODE_OBJECTS == (hb.build_export_bin_code,) and hb.QUERY_CODE_OBJECTS == (hb.build_bounds_code,)
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    for other in (hb.export_code_path(), hb.export_sort_code_path(), hb.export_filter_code_path(), hb.export_cull_code_path(), hb.export_filter_prog_code_path(),
                  hb.export_cull_prog_code_path(), hb.export_bin_code_path(), hb.bounds_code_path()):
        assert open(other, "rb").read() in lib and not set(_rows(other)) & set(IMPORT_KERNELS)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_import_code.inc" in ignored and "*.hsaco" in ignored


def test_write_attr_and_the_import_share_one_reset_helper():
    src = open(os.path.join(CSRC, "hanabi_amd.hip")).read()
    body = lambda name: src[src.index(name):].split("\n}\n", 1)[0]
    assert "reset_plane_proofs(fx, attr == HNB_ATTR_AGE)" in body("int hnb_effect_write_attr(") and body("int hnb_effect_write_attr(").count("hipStreamSynchronize") == 2
    assert "reset_plane_proofs(fx, c.has_age)" in body("int run_import(") and "Synchronize" not in body("int run_import(") and "hipMemcpy(" not in body("int run_import(")
    helper = body("static int reset_plane_proofs(")
    for word in ("skip_hist.dirty = true", "ribbon_hist.dirty = true", "front_broken = true", "values_broken = true", "horizon_off", "lmin_off", "age_cohort"):
        assert word in helper, word
    assert src.count("skip_hist.dirty = true;  // the published") == 1 and "ribbon_hist.front_broken = true" not in src.replace(helper, "")
