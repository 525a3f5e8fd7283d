"""Particle bounds (hnb_effect_bounds / hnb_program_bounds, include/hanabi_amd.h "Bounds") without a GPU: header, ctypes mirror and INTEGRATION.md
agree on the structures and the prototypes, and the calls fail loudly; the kernels live in a sixth code object of exactly four kernels with no
scratch, no spills and under 1 KiB of LDS, next to the five of the exports, which are as they were; the launch plan and the scratch layout of
csrc/hnb_bounds.h are DESIGN.md's table; and the fold of that header, compiled as a stand-alone host program, gives the bits of a numpy restatement
over the lattice of edge values whatever the order and the grouping of the particles."""
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
from bevy_hanabi_amd import _hanabi_host as h
from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import runtime
from test_export_filtered_abi import CSRC, EDGE_BITS, _rows, _standalone
from test_export_sorted_abi import A, LLVM, ROOT, key_f32

BOUNDS_KERNELS = ["k_bounds_tile", "k_bounds_finish", "k_bounds_union", "k_bounds_small"]
POS_INF, NEG_INF = 0x7F800000, 0xFF800000


# ---- an asset with a 4-component f32 attribute (tests/test_gpu_bounds.py; tools/warm_jit_cache.py compiles its kernels ahead) ------------------------
def trails_vec4(capacity):
    """The firework's trails with a 4-component f32 attribute in the layout: POSITION and VELOCITY (3), AGE and LIFETIME (1), F32X4_0 (4)"""
    w = h.ExprWriter()
    direction = w.rand(h.VectorType.VEC3F).mul(w.lit(2.0)).sub(w.lit(1.0)).normalized()
    mods = [h.SetAttributeModifier(h.Attribute.POSITION, w.lit((0.0, 0.0, 0.0)).expr()),
            h.SetAttributeModifier(h.Attribute.VELOCITY, (direction * w.lit(40.0).uniform(w.lit(60.0))).expr()),
            h.SetAttributeModifier(h.Attribute.AGE, w.lit(0.0).expr()),
            h.SetAttributeModifier(h.Attribute.LIFETIME, w.lit(0.8).uniform(w.lit(1.2)).expr()),
            h.SetAttributeModifier(h.Attribute.F32X4_0, (w.rand(h.VectorType.VEC4F) * w.lit(8.0) - w.lit(4.0)).expr())]
    asset = h.EffectAsset(capacity, h.SpawnerSettings.once(float(capacity)), w.finish()).with_name("trail4")
    for m in mods:
        asset = asset.init(m)
    return asset


# ---- the semantics, restated in numpy ---------------------------------------------------------------------------------------------------------------
def np_bounds(bits, alive):
    """bits: [slots, ncomp] stored words, alive: [slots] bool -> the 12 words of the HnbBounds record. Per component the stored value with the
    smallest / largest key k = b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000) among the alive slots whose component is not a NaN; (+inf, -inf) if there
    is none; components past ncomp 0; alive slots; alive slots with a NaN in any component."""
    bits = np.asarray(bits, np.uint32)
    bits = bits.reshape(len(bits), bits.shape[1] if bits.ndim > 1 else 1)
    alive = np.asarray(alive, bool)
    is_nan = (bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    rec = np.zeros(12, np.uint32)
    for c in range(bits.shape[1]):
        v = bits[alive & ~is_nan[:, c], c]
        k = key_f32(v)
        rec[c] = v[np.argmin(k)] if len(v) else POS_INF
        rec[4 + c] = v[np.argmax(k)] if len(v) else NEG_INF
    rec[8] = alive.sum()
    rec[9] = (alive & is_nan.any(axis=1)).sum()
    return rec


def np_union(records, ncomp):
    """[n, 12] instance records -> the union record: lo / hi folded by the same rule (a record's lo / hi are never NaNs), alive and nan summed"""
    records = np.asarray(records, np.uint32).reshape(-1, 12)
    rec = np.zeros(12, np.uint32)
    for c in range(ncomp):
        rec[c] = records[np.argmin(key_f32(records[:, c])), c]
        rec[4 + c] = records[np.argmax(key_f32(records[:, 4 + c])), 4 + c]
    rec[8] = records[:, 8].sum(dtype=np.uint64) & 0xFFFFFFFF
    rec[9] = records[:, 9].sum(dtype=np.uint64) & 0xFFFFFFFF
    return rec


def test_the_restatement_itself_on_a_case_worked_by_hand():
    f = lambda *x: np.array(x, np.float32).view(np.uint32)
    bits = np.stack([f(1.0, -0.0, np.nan), f(-2.0, 0.0, np.nan), f(np.nan, 5.0, np.nan), f(np.inf, -7.0, 3.0)])
    rec = np_bounds(bits, [True, True, True, False])                      # the last slot is dead: its inf, -7 and 3 do not enter
    assert list(rec[:3]) == [f(-2.0)[0], 0x80000000, POS_INF] and list(rec[4:7]) == [f(1.0)[0], f(5.0)[0], NEG_INF]      # -0 < +0; z is a NaN in every alive slot
    assert list(np_bounds(bits[:2, 1:2], [True, True])[[0, 4]]) == [0x80000000, 0x00000000]                               # ... and +0 is the larger of the two zeros
    assert (rec[3], rec[7], rec[8], rec[9], rec[10], rec[11]) == (0, 0, 3, 3, 0, 0)
    assert list(np_bounds(bits[:0], [])) == [POS_INF] * 3 + [0] + [NEG_INF] * 3 + [0] * 5
    assert list(np_union([rec, np_bounds(bits[3:], [True])], 3)[[0, 4, 2, 6, 8, 9]]) == [f(-2.0)[0], POS_INF, f(3.0)[0], f(3.0)[0], 4, 3]


# ---- the binding --------------------------------------------------------------------------------------------------------------------------------
def test_ctypes_mirrors_have_the_headers_sizes_and_offsets(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd.h"
    int main(void) {
        int (*fe)(HnbEffect*, const HnbBoundsDesc*) = hnb_effect_bounds;
        int (*fp)(HnbProgram*, const HnbBoundsDesc*) = hnb_program_bounds;
        printf("%zu %zu %zu %zu %zu %zu", sizeof(HnbBounds), offsetof(HnbBounds, lo), offsetof(HnbBounds, hi), offsetof(HnbBounds, alive), offsetof(HnbBounds, nan),
               offsetof(HnbBounds, reserved));
        printf(" %zu %zu %zu %zu %zu %zu %zu\n", sizeof(HnbBoundsDesc), offsetof(HnbBoundsDesc, struct_size), offsetof(HnbBoundsDesc, attr), offsetof(HnbBoundsDesc, flags),
               offsetof(HnbBoundsDesc, reserved), offsetof(HnbBoundsDesc, dst), offsetof(HnbBoundsDesc, dst_capacity_records));
        return fe == 0 || fp == 0;
    }
    '''
    (tmp_path / "t.c").write_text(src)
    lib_dir = os.path.dirname(hb.runtime_lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-L" + lib_dir, "-lhanabi_amd",
                           "-Wl,-rpath," + lib_dir, "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True, text=True).stdout.split()]
    B, D = runtime.Bounds, runtime.BoundsDesc
    assert got == [C.sizeof(B), B.lo.offset, B.hi.offset, B.alive.offset, B.nan.offset, B.reserved.offset,
                   C.sizeof(D), D.struct_size.offset, D.attr.offset, D.flags.offset, D.reserved.offset, D.dst.offset, D.dst_capacity_records.offset]
    assert got[:6] == [48, 0, 16, 32, 36, 40] and got[6:] == [32, 0, 4, 8, 12, 16, 24]
    d = runtime.bounds_desc(A.POSITION.id, 0x1000, 3)
    assert (d.struct_size, d.attr, d.flags, d.reserved, d.dst, d.dst_capacity_records) == (32, A.POSITION.id, 0, 0, 0x1000, 3)


def test_header_ctypes_and_integration_agree_on_the_prototypes():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = runtime.load_library()
    for name, handle, rust in (("hnb_effect_bounds", "HnbEffect* fx", "fx: *mut HnbEffect"), ("hnb_program_bounds", "HnbProgram* prog", "prog: *mut HnbProgram")):
        assert name in runtime.ABI_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == [C.c_void_p, C.POINTER(runtime.BoundsDesc)]
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == [handle, "const HnbBoundsDesc* desc"], name
        m = re.search(r"pub fn " + name + r"\(([^)]*)\) -> c_int;", txt)
        assert m and [a.strip() for a in m.group(1).split(",")] == [rust, "desc: *const HnbBoundsDesc"], name
    assert runtime.ABI_SYMBOLS[-2:] == ["hnb_effect_bounds", "hnb_program_bounds"] and len(runtime.ABI_SYMBOLS) == 61      # numbered behind the 59 before them
    assert callable(runtime.Effect.bounds) and callable(runtime.Program.bounds)
    assert "hnb_effect_set_simulated(fx, visible)" in txt                                  # ... and a paragraph on feeding the visibility decision


def test_calls_fail_loudly_on_null_arguments_and_without_a_device():
    lib = runtime.load_library()
    d = runtime.bounds_desc(A.POSITION.id, 0x1000, 1)
    fake = C.c_void_p(0x1000)            # never dereferenced: the NULL argument is refused first
    for call in (lib.hnb_effect_bounds, lib.hnb_program_bounds):
        for args in ((None, C.byref(d)), (fake, None), (None, None)):
            assert call(*args) == -1 and b"NULL" in lib.hnb_last_error()
    if not torch.cuda.is_available():   # no device: there is no effect to take bounds of, and creating a context is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


# ---- the code object ----------------------------------------------------------------------------------------------------------------------------
def test_sixth_code_object_is_built_carried_and_has_its_four_kernels_without_scratch_or_spills():
    co = hb.bounds_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_bounds.hip into it"
    code = open(co, "rb").read()
    assert code[:4] == b"\x7fELF"
    head = subprocess.run([f"{LLVM}/llvm-readelf", "-h", co], check=True, capture_output=True, text=True).stdout
    assert "gfx950" in head, head
    rows = _rows(co)
    assert sorted(rows) == sorted(BOUNDS_KERNELS), sorted(rows)
    for name, r in rows.items():
        assert 0 < r["group_segment_fixed_size"] <= 1024, f"{name}: {r['group_segment_fixed_size']} B of LDS per workgroup"
        assert r["private_segment_fixed_size"] == 0, f"{name}: {r['private_segment_fixed_size']} B of scratch per thread"
        assert r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)
        assert r["kernarg_segment_size"] == 72, (name, r)                 # one BoundsArgs by value
        assert r["vgpr_count"] <= 64, (name, r)                           # eight waves per SIMD stay possible
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert code in lib
    assert '"-ffp-contract=off"' in inspect.getsource(hb.build_bounds_code)
    assert "#pragma clang fp contract(off)" in open(os.path.join(CSRC, "hnb_bounds.hip")).read()
    assert hb.build_bounds_code in hb.QUERY_CODE_OBJECTS and hb.build_bounds_code not in hb.EXPORT_CODE_OBJECTS
    assert "QUERY_CODE_OBJECTS" in inspect.getsource(hb.build_runtime)
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "bevy_hanabi_amd/csrc/hnb_bounds_code.inc" in ignored and "*.hsaco" in ignored


def test_the_exports_five_code_objects_and_tables_are_as_they_were():
    lib = open(hb.runtime_lib_path(), "rb").read()
    for other in (hb.export_code_path(), hb.export_sort_code_path(), hb.export_filter_code_path(), hb.export_cull_code_path(), hb.export_filter_prog_code_path()):
        assert open(other, "rb").read() in lib
        assert not set(_rows(other)) & set(BOUNDS_KERNELS)
    assert len(hb.EXPORT_CODE_OBJECTS) == 6
    export_h = open(os.path.join(CSRC, "hnb_export.h")).read()
    assert "bounds" not in export_h.lower()                               # ExportUnit, ExportKernel, ExportArgBlock and export_launch_plan know nothing of the new unit


# ---- the launch plan and the scratch layout (csrc/hnb_bounds.h), as a stand-alone host program ---------------------------------------------------
def plan_table(program, n, cap):
    """DESIGN.md "Bounds": the launches of a call"""
    T = -(-cap // 4096)
    g = n if program else 1
    plan = [("small", 1, g)] if T <= 1 else [("tile", T, g), ("finish", 1, g)]
    return plan + ([("union", 1, 1)] if program else [])


def layout_table(n, cap):
    """... and the scratch: (tiles, bytes between two instances' sections, bytes in all)"""
    T = -(-cap // 4096)
    pitch = 0 if T <= 1 else -(-T * 64 // 256) * 256
    return T, pitch, n * pitch


PLAN_SRC = r"""
#include <cstdio>
#include <cstdint>
#include "hnb_bounds.h"
using namespace hnb;
int main() {
    static_assert(kBoundsKTile == 0 && kBoundsKFinish == 1 && kBoundsKUnion == 2 && kBoundsKSmall == 3 && kBoundsKernelCount == 4, "four kernels");
    static_assert(kBoundsTile == 4096 && kBoundsBlock == 256 && sizeof(BoundsPartial) == 64 && sizeof(BoundsArgs) == 72, "tiles, lanes, partials");
    static const char* const names[] = {"tile", "finish", "union", "small"};
    unsigned program; unsigned long long n, cap;
    while (std::scanf("%u %llu %llu", &program, &n, &cap) == 3) {
        const BoundsPlan pl = bounds_launch_plan(program != 0, (uint32_t)n, (uint32_t)cap);
        const BoundsScratch l = bounds_scratch_layout((uint32_t)n, (uint32_t)cap);
        if (pl.n > kBoundsPlanMax) return 2;
        std::printf("%u %u %llu %llu %llu %llu %u", l.n_inst, l.tiles, (unsigned long long)l.pitch_bytes, (unsigned long long)l.total,
                    (unsigned long long)bounds_partial_offset(l, 0, l.tiles - 1), (unsigned long long)bounds_partial_offset(l, (uint32_t)n - 1, l.tiles - 1), pl.n);
        for (uint32_t i = 0; i < pl.n; ++i) std::printf(" %s %u %u", names[pl.launch[i].kernel], pl.launch[i].grid_x, pl.launch[i].grid_y);
        std::printf("\n");
    }
    return 0;
}
"""


def test_launch_plan_and_scratch_layout_are_the_designs_table(tmp_path):
    exe = _standalone(tmp_path, "bpl", PLAN_SRC)
    cases = [(program, n, cap) for cap in (1, 4096, 4097, 10_000, (1 << 32) - 1) for n in (1, 5, 65_535) for program in (0, 1)]
    out = subprocess.run([exe], input="\n".join("%d %d %d" % c for c in cases), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (program, n, cap), line in zip(cases, out):
        w = line.split()
        n_inst, tiles, pitch, total, last0, last, count = [int(x) for x in w[:7]]
        got = [(w[i], int(w[i + 1]), int(w[i + 2])) for i in range(7, len(w), 3)]
        assert count == len(got) and got == plan_table(program, n, cap), (program, n, cap, got)
        assert count == (1 if cap <= 4096 else 2) + program                # one launch / two; two / three above 4096 slots, whatever the instance count
        assert (n_inst, tiles, pitch, total) == (n,) + layout_table(n, cap), (n, cap, line)
        assert pitch % 256 == 0 and (cap <= 4096) == (total == 0)
        if total:                                                        # the last partial of an instance ends inside its section, the last instance's inside the allocation
            assert last0 == (tiles - 1) * 64 and last0 + 64 <= pitch < last0 + 64 + 256
            assert last == (n - 1) * pitch + last0 and last + 64 <= total  # (in 64 bits: 65,535 instances of 2^32 - 1 slots are 2^42 bytes)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## Bounds" in design
    for row in ("| effect | <= 4096 | 1 | `k_bounds_small` (1, 1) |", "| effect | > 4096 | 2 | `k_bounds_tile` (T, 1), `k_bounds_finish` (1, 1) |",
                "| program | <= 4096 | 2 | `k_bounds_small` (1, n), `k_bounds_union` (1, 1) |",
                "| program | > 4096 | 3 | `k_bounds_tile` (T, n), `k_bounds_finish` (1, n), `k_bounds_union` (1, 1) |"):
        assert row in design, row


# ---- the fold ---------------------------------------------------------------------------------------------------------------------------------------
FOLD_SRC = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "hnb_bounds.h"
using namespace hnb;
static void print(const HnbBounds& r) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&r);
    for (int i = 0; i < 12; ++i) std::printf("%x ", w[i]);
}
// input: "ncomp slots groups", then per slot "group alive word..."; output: the record of all slots (the groups' partials merged in group order),
// then the union of the groups' own records (every group taken for an instance)
int main() {
    unsigned nc, n, g;
    while (std::scanf("%u %u %u", &nc, &n, &g) == 3) {
        std::vector<BoundsPartial> part(g, bounds_empty());
        for (unsigned i = 0; i < n; ++i) {
            unsigned grp, alive, bits[4] = {};
            if (std::scanf("%u %u", &grp, &alive) != 2 || grp >= g) return 1;
            for (unsigned c = 0; c < nc; ++c) if (std::scanf("%x", &bits[c]) != 1) return 1;
            bounds_fold_slot(part[grp], bits, nc, alive != 0);
        }
        BoundsPartial all = bounds_empty(), uni = bounds_empty();
        for (unsigned k = 0; k < g; ++k) {
            bounds_merge(all, part[k]);
            const HnbBounds r = bounds_record(part[k], nc);
            bounds_fold_record(uni, reinterpret_cast<const uint32_t*>(&r), nc);
        }
        print(bounds_record(all, nc));
        print(bounds_record(uni, nc));
        std::printf("\n");
    }
    return 0;
}
"""


def test_fold_of_the_edge_lattice_is_the_numpy_restatement_whatever_the_order_and_the_grouping(tmp_path):
    exe = _standalone(tmp_path, "bfold", FOLD_SRC)
    rng = np.random.default_rng(11)
    lattice = np.array(list(itertools.product(EDGE_BITS, repeat=3)), np.uint32)          # 4096 particles: +-0, +-inf, +-NaN, denormals in every component
    sets = [(lattice, rng.random(len(lattice)) < 0.7), (lattice, np.ones(len(lattice), bool)), (lattice, np.zeros(len(lattice), bool))]
    for nc in (1, 2, 4):
        sets.append((rng.choice(np.array(EDGE_BITS, np.uint32), (600, nc)), rng.random(600) < 0.5))
    only_nan_y = lattice[(lattice[:, 1] & 0x7FFFFFFF) > 0x7F800000]
    sets.append((only_nan_y, np.ones(len(only_nan_y), bool)))                            # a component that is a NaN in every particle
    sets.append((np.array([[0x80000000, 0, 0x7FC00000]], np.uint32), np.array([True])))  # one particle
    lines, want = [], []
    for bits, alive in sets:
        n, nc = bits.shape
        rec = np_bounds(bits, alive)
        groupings = [np.zeros(n, int), np.arange(n), np.arange(n) // 100, rng.integers(0, 7, n), np.arange(n) % 64]
        for grp in groupings:
            order = rng.permutation(n)
            g = int(grp.max()) + 1
            lines.append(f"{nc} {n} {g}")
            lines += [f"{grp[i]} {int(alive[i])} " + " ".join(f"{int(b):x}" for b in bits[i]) for i in order]
            want.append(rec)
    out = subprocess.run([exe], input="\n".join(lines), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(want)
    for line, rec in zip(out, want):
        got = np.array([int(x, 16) for x in line.split()], np.uint32)
        np.testing.assert_array_equal(got[:12], rec)                     # the same bits whatever the grouping
        np.testing.assert_array_equal(got[12:], rec)                     # ... and through records and the union's fold
    assert any(r[8] and r[1] == POS_INF and r[5] == NEG_INF for r in want)                # the all-NaN component came out empty next to contributing ones
    assert any(r[0] == NEG_INF and r[4] == POS_INF for r in want)                         # infinities take part
