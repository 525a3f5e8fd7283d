"""The packed export (hnb_effect_export / hnb_program_export, include/hanabi_amd.h "Packed output") without a GPU: the ctypes mirrors have the
header's layout, the calls fail loudly, the kernels' code object exists and declares what the sources promise, and
hnb_asset_particle_layout_aos gives the reference's interleaved layout (ParticleLayout) as export fields."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import build as hb
from bevy_hanabi_amd import effects, runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
A = bh.Attribute


def test_ctypes_mirrors_have_the_headers_sizes_and_offsets(tmp_path):
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "hanabi_amd.h"
    int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u\n", sizeof(HnbExportField), offsetof(HnbExportField, dst_offset), sizeof(HnbExportDesc),
                            offsetof(HnbExportDesc, n_fields), offsetof(HnbExportDesc, record_stride), offsetof(HnbExportDesc, flags), offsetof(HnbExportDesc, dst),
                            offsetof(HnbExportDesc, dst_capacity_records), offsetof(HnbExportDesc, out_count), offsetof(HnbExportDesc, fields), HNB_EXPORT_MAX_FIELDS); return 0; }
    '''
    (tmp_path / "t.c").write_text(src)
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    F, D = runtime.ExportField, runtime.ExportDesc
    assert got == [C.sizeof(F), F.dst_offset.offset, C.sizeof(D), D.n_fields.offset, D.record_stride.offset, D.flags.offset, D.dst.offset,
                   D.dst_capacity_records.offset, D.out_count.offset, D.fields.offset, runtime.EXPORT_MAX_FIELDS]
    d = runtime.export_desc([(A.POSITION.id, 0), (A.AGE.id, 12)], 0x1000, 16, 7, 0x2000)
    assert (d.struct_size, d.n_fields, d.record_stride, d.flags, d.dst, d.dst_capacity_records, d.out_count) == (C.sizeof(D), 2, 16, 0, 0x1000, 7, 0x2000)
    assert (d.fields[1].attr, d.fields[1].reserved, d.fields[1].dst_offset) == (A.AGE.id, 0, 12)


def test_calls_fail_loudly_without_an_effect_or_a_device():
    lib = runtime.load_library()
    d = runtime.export_desc([(A.POSITION.id, 0)], 0x1000, 16, 1)
    assert lib.hnb_effect_export(None, C.byref(d)) == -1 and b"NULL" in lib.hnb_last_error()
    assert lib.hnb_program_export(None, C.byref(d), None) == -1
    assert lib.hnb_effect_export(None, None) == -1 and lib.hnb_program_export(None, None, None) == -1
    if not torch.cuda.is_available():   # no device: there is no context to export from, and creating one is an error, not a CPU path
        with pytest.raises(bh.HanabiError):
            bh.Context(0)


def test_export_code_object_is_built_and_declares_its_lds_and_no_scratch():
    """The gather kernels live in a code object of their own (nothing is added to the fat binary of libhanabi_amd.so, whose kernel table
    tests/test_kernel_resources.py pins): at most 32 KiB of LDS per workgroup and no scratch, read from the code object's notes."""
    co = hb.export_code_path()
    assert os.path.exists(co), f"{co} is missing: build() compiles csrc/hnb_export.hip into it"
    assert open(co, "rb").read(4) == b"\x7fELF"
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s+\.(group_segment_fixed_size|private_segment_fixed_size|name):\s+(.*)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2).strip()
        if len(cur) == 3:
            kernels[cur["name"]] = (int(cur["group_segment_fixed_size"]), int(cur["private_segment_fixed_size"]))
            cur = {}
    rows = sorted(k for k in kernels if k.startswith("k_export_rows"))
    assert rows == ["k_export_rows_128", "k_export_rows_256", "k_export_rows_32", "k_export_rows_64"] and "k_export_offsets" in kernels, kernels
    for name, (lds, scratch) in kernels.items():
        assert lds <= 32 * 1024, f"{name}: {lds} B of LDS per workgroup"
        assert scratch == 0, f"{name}: {scratch} B of scratch per thread"
    assert kernels["k_export_rows_32"][0] == 256 * 32 and kernels["k_export_rows_256"][0] == 128 * 256    # the tile's records, nothing else
    # ... and the library carries exactly these bytes (csrc/hnb_export_code.inc) while its fat binary knows nothing of them
    lib = open(hb.runtime_lib_path(), "rb").read()
    assert open(co, "rb").read() in lib


def _host_lib():
    l = C.CDLL(hb.build_host_lib())
    l.hnb_host_last_error.restype = C.c_char_p
    l.hnb_asset_from_ron.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
    l.hnb_asset_destroy.argtypes = [C.c_void_p]
    l.hnb_asset_particle_layout_aos.argtypes = [C.c_void_p, C.POINTER(runtime.ExportField), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    return l


def aos_layout(asset):
    """-> ([(attribute id, byte offset)], stride) from hnb_asset_particle_layout_aos, the asset handed over as RON text."""
    l = _host_lib()
    ron = bh.to_ron(asset).encode()
    h = C.c_void_p()
    assert l.hnb_asset_from_ron(ron, len(ron), C.byref(h)) == 0, l.hnb_host_last_error()
    n, stride = C.c_uint32(), C.c_uint32()
    assert l.hnb_asset_particle_layout_aos(h, None, 0, C.byref(n), C.byref(stride)) == 0      # the count alone
    out = (runtime.ExportField * n.value)()
    n2 = C.c_uint32()
    assert l.hnb_asset_particle_layout_aos(h, out, n.value, C.byref(n2), C.byref(stride)) == 0 and n2.value == n.value
    assert l.hnb_asset_particle_layout_aos(None, out, n.value, C.byref(n2), C.byref(stride)) != 0
    l.hnb_asset_destroy(h)
    assert all(f.reserved == 0 for f in out)
    return [(f.attr, f.dst_offset) for f in out], stride.value


def mixed_width_asset(capacity=64):
    """vec4 + vec3 + vec3 + vec2 + scalars: every packing rule of ParticleLayoutBuilder::build at once (a vec3 paired with a scalar, a vec3 left
    over and padded, the odd vec2, trailing padding up to the struct's alignment)."""
    w = bh.ExprWriter()
    mods = [bh.SetAttributeModifier(A.POSITION, w.lit((1.0, 2.0, 3.0)).expr()), bh.SetAttributeModifier(A.VELOCITY, w.lit((4.0, 5.0, 6.0)).expr()),
            bh.SetAttributeModifier(A.HDR_COLOR, w.lit((0.1, 0.2, 0.3, 0.4)).expr()), bh.SetAttributeModifier(A.SIZE2, w.lit((7.0, 8.0)).expr()),
            bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr())]
    asset = bh.EffectAsset(capacity, bh.SpawnerSettings.once(float(capacity)), w.finish())
    for m in mods:
        asset.init(m)
    return asset


def _expected_layout(layout):
    return [(bh.Attribute.from_name(name).id, off) for name, off in layout.entries() if name != "pad"], layout.min_binding_size()


def test_aos_layout_is_the_references_particle_layout():
    default = bh.ParticleLayout.default()
    assert [(n, o) for n, o in default.entries()] == [("position", 0), ("age", 12), ("velocity", 16), ("lifetime", 28)] and default.min_binding_size() == 32
    for asset in (effects.firework_trails(4096), mixed_width_asset(), effects.ribbon(4096)):
        fields, stride = aos_layout(asset)
        ref = asset.reference_particle_layout()
        assert (fields, stride) == _expected_layout(ref), asset.name
        assert stride % 16 == 0 and stride >= ref.size()
        ends = sorted((o, o + 4 * runtime.ATTR_COMPONENTS[a]) for a, o in fields)
        assert all(e0 <= s1 for (_, e0), (s1, _) in zip(ends, ends[1:])) and ends[-1][1] <= stride      # no overlap, inside the stride
    # an asset whose stored attributes are exactly the default layout's gives the default layout
    w = bh.ExprWriter()
    mods = [bh.SetAttributeModifier(a, w.lit(v).expr()) for a, v in ((A.POSITION, (0.0, 0.0, 0.0)), (A.VELOCITY, (1.0, 2.0, 3.0)), (A.AGE, 0.0), (A.LIFETIME, 5.0))]
    plain = bh.EffectAsset(64, bh.SpawnerSettings.once(64.0), w.finish())
    for m in mods:
        plain.init(m)
    assert aos_layout(plain) == ([(A.POSITION.id, 0), (A.AGE.id, 12), (A.VELOCITY.id, 16), (A.LIFETIME.id, 28)], 32)
    fields, stride = aos_layout(effects.firework_trails(4096))
    assert fields == [(A.POSITION.id, 0), (A.AGE.id, 12), (A.VELOCITY.id, 16), (A.COLOR.id, 28), (A.LIFETIME.id, 32)] and stride == 48
    fields, stride = aos_layout(mixed_width_asset())
    assert fields == [(A.HDR_COLOR.id, 0), (A.POSITION.id, 16), (A.AGE.id, 28), (A.VELOCITY.id, 32), (A.SIZE2.id, 48)] and stride == 64   # velocity's pad at 44, tail pad 56..64
