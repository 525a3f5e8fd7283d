"""The steps kernel of a streaming update specialised at run time (hnb_jit.h "steps modules"), without a GPU: hnb_jit_precompile_steps fills the cache
with a module of its own that holds exactly the FUSED instantiation of the program's stream kernel, leaves what hnb_jit_precompile writes alone, and the
fused form stays inside the LDS / scratch ceilings of tests/test_kernel_resources.py. (That spans actually run fused, bit for bit: the GPU tests of
tests/test_gpu_simulate_steps_jit.py.)"""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, reference_examples, runtime
from steps_jit_assets import accel_radial_tangent_drag, pinned_set_accel, tangent_drag
from test_kernel_resources import LDS_BUDGET, LLVM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hnb_program_prepare_steps", "hnb_jit_precompile_steps")
LDS_MAX = LDS_BUDGET["k_update_slots_stream"]      # 24,672 B
SCRATCH_MAX = 640                                  # test_kernel_resources.test_scratch_only_where_expected
STACKS = {"tangent_drag": tangent_drag, "accel_radial_tangent_drag": accel_radial_tangent_drag}


def _entries(cache):
    return {p.name: p for p in cache.glob("*.hnbjit")}


def _read_entry(path):
    """A cache entry (hnb_jit.h CacheHeader: 64 bytes, then the lowered names, one per line, then the code object)."""
    raw = path.read_bytes()
    assert raw[:7] == b"HNBJIT2"
    code_size, _, n_names, names_bytes = struct.unpack_from("<QQII", raw, 40)
    names = raw[64:64 + names_bytes].decode().split("\n")[:-1]
    assert len(names) == n_names and len(raw) == 64 + names_bytes + code_size
    return names, raw[64 + names_bytes:]


def _resources(path, tmp_path):
    """{lowered kernel name: (VGPRs, SGPRs, LDS bytes, scratch bytes)} of the code object of a cache entry."""
    if not os.path.exists(f"{LLVM}/llvm-readelf"):
        pytest.skip("LLVM tools not present")
    names, code = _read_entry(path)
    co = tmp_path / (path.name + ".co")
    if code[:4] == b"\x7fELF":
        co.write_bytes(code)
    else:
        bundle = tmp_path / (path.name + ".bundle")
        bundle.write_bytes(code)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={bundle}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)
        out[g("name")] = tuple(int(g(k)) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size"))
    assert set(names) <= set(out), (names, sorted(out))
    return out


def _stream_kernels(names):
    return [n for n in names if "k_update_slots_stream" in n]


def _is_fused(lowered):
    """k_update_slots_stream<PROG, WAVES, PROBE, COHORT, FUSED>: the Itanium mangling ends the template arguments with ...Lb<COHORT>ELb<FUSED>EEE."""
    m = re.search(r"Lb([01])ELb([01])EEEv", lowered)
    assert m, lowered
    return m.group(2) == "1"


@pytest.fixture
def cache(tmp_path, monkeypatch):
    d = tmp_path / "cache"
    monkeypatch.setenv("HNB_JIT_CACHE", str(d))
    return d


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hanabi_amd.h")).read(), flags=re.S)
    lib = runtime.load_library()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW:
        assert re.search(r"\bint " + n + r"\s*\(", hdr), f"{n} is not declared in include/hanabi_amd.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in runtime.ABI_SYMBOLS
        assert f"pub fn {n}(" in integration
    assert callable(bh.Program.prepare_steps) and callable(bh.jit_precompile_steps)


def test_new_entry_points_reject_null_arguments():
    lib = runtime.load_library()
    assert lib.hnb_program_prepare_steps(None) != 0
    assert b"NULL" in lib.hnb_last_error()
    assert lib.hnb_jit_precompile_steps(None, 0) != 0
    assert lib.hnb_jit_precompile_steps(b"garbage", 7) != 0
    with pytest.raises(bh.HanabiError):
        bh.jit_precompile_steps(b"")


# ---- the cache ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack", sorted(STACKS))
def test_precompile_steps_adds_one_entry_with_the_fused_kernel(cache, stack):
    blob = bh.lower(STACKS[stack](300_077))
    bh.jit_precompile_steps(blob)
    entries = _entries(cache)
    assert len(entries) == 1
    path = next(iter(entries.values()))
    names, code = _read_entry(path)
    assert len(names) == 1 and "k_update_slots_stream" in names[0] and _is_fused(names[0]), names     # exactly one kernel: the FUSED template argument
    assert names[0].encode() in code
    t0 = os.stat(path).st_mtime_ns
    bh.jit_precompile_steps(blob)                                                                     # a hit: not rewritten
    assert os.stat(path).st_mtime_ns == t0 and len(_entries(cache)) == 1
    bh.jit_precompile_steps(bh.lower(STACKS[stack](1 << 20)))                                         # capacity does not enter the key
    assert len(_entries(cache)) == 1
    assert not list(cache.glob("*.tmp*"))


def test_precompile_steps_writes_nothing_for_prebuilt_and_generic_updates(cache):
    for asset in (effects.firework_trails(1 << 20), reference_examples.example_expr(), effects.ribbon(4096), effects.single_particle(16)):
        bh.jit_precompile_steps(bh.lower(asset))
    assert not cache.exists() or not list(cache.iterdir())


def test_precompile_writes_what_it_wrote_with_or_without_the_steps_module(tmp_path, monkeypatch):
    """hnb_jit_precompile of a jit-stream blob: one entry, the same key and the same kernels (single-frame: FUSED = false) whether or not the steps
    module of the blob is in the cache."""
    blob = bh.lower(tangent_drag(300_077))
    a, b = tmp_path / "a", tmp_path / "b"
    monkeypatch.setenv("HNB_JIT_CACHE", str(a))
    bh.jit_precompile(blob)
    monkeypatch.setenv("HNB_JIT_CACHE", str(b))
    bh.jit_precompile_steps(blob)
    steps = set(_entries(b))
    bh.jit_precompile(blob)
    assert len(_entries(a)) == 1 and len(steps) == 1 and len(_entries(b)) == 2
    assert set(_entries(b)) - steps == set(_entries(a))                     # the same key: source, name expressions, options and headers are what they were
    names, _ = _read_entry(next(iter(_entries(a).values())))
    stream = _stream_kernels(names)
    assert len(names) == 3 and len(stream) == 1 and not _is_fused(stream[0]), names     # k_init, k_init_slots, the single-frame stream kernel
    bh.jit_precompile(bh.lower(effects.firework_trails(2048)))              # (a pre-built update: init only, as before)
    assert len(_entries(b)) == 3


# ---- the generated translation units ------------------------------------------------------------------------------------------------------------
def test_translation_units(cache, tmp_path, monkeypatch):
    """HNB_JIT_DUMP writes <key>.hip beside the name of the cache entry. The steps module: no code of its own - the kernel headers and ONE name
    expression. The program's module of the same blob: byte for byte the text the commit before the steps modules generated (tests/golden/jit_steps)."""
    dump = tmp_path / "dump"
    dump.mkdir()
    monkeypatch.setenv("HNB_JIT_DUMP", str(dump))
    blob = bh.lower(tangent_drag(300_077))
    bh.jit_precompile_steps(blob)
    (key,) = [p.stem for p in cache.glob("*.hnbjit")]
    steps_tu = (dump / (key + ".hip")).read_text()
    assert '#include "hnb_kernels.hip.h"' in steps_tu and "__global__" not in steps_tu and "struct" not in steps_tu and "vm_exec" not in steps_tu
    names, _ = _read_entry(cache / (key + ".hnbjit"))
    assert len(names) == 1
    bh.jit_precompile(blob)
    (pkey,) = [p.stem for p in cache.glob("*.hnbjit") if p.stem != key]
    golden = open(os.path.join(ROOT, "tests", "golden", "jit_steps", "tangent_drag_program_tu.txt")).read()
    assert (dump / (pkey + ".hip")).read_text() == golden


# ---- registers, LDS, scratch --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack", sorted(STACKS) + ["pinned_set_accel"])
def test_fused_kernel_resources(cache, tmp_path, stack):
    """The S-loop runs on registers: LDS and scratch inside the ceilings of tests/test_kernel_resources.py, and no more scratch than the single-frame
    instantiation of the same stack under the same __launch_bounds__ (DESIGN.md records the values)."""
    make = dict(STACKS, pinned_set_accel=pinned_set_accel)[stack]
    blob = bh.lower(make(300_077))
    bh.jit_precompile_steps(blob)
    (steps_path,) = _entries(cache).values()
    bh.jit_precompile(blob)
    (prog_path,) = [p for n, p in _entries(cache).items() if n != steps_path.name]
    fused = _resources(steps_path, tmp_path)
    single = _resources(prog_path, tmp_path)
    (fk,) = _stream_kernels(fused)
    (sk,) = _stream_kernels(single)
    assert _is_fused(fk) and not _is_fused(sk)
    assert fk.replace("Lb1EEEv", "Lb0EEEv") == sk, (fk, sk)             # the same ops, wave budget and cohort choice
    fv, fs, flds, fscratch = fused[fk]
    sv, ss, slds, sscratch = single[sk]
    print(f"{stack}: fused VGPRs {fv} SGPRs {fs} LDS {flds} scratch {fscratch} | single frame VGPRs {sv} SGPRs {ss} LDS {slds} scratch {sscratch}")
    assert flds <= LDS_MAX, (stack, flds)
    assert fscratch <= SCRATCH_MAX, (stack, fscratch)
    assert fscratch <= sscratch, (stack, fscratch, sscratch)
