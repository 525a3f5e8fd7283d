"""plan::prove_fused_span (bevy_hanabi_amd/csrc/hnb_plan.h) without a device: every premise of "these S frames may run as one launch", and the
equivalence it must keep - the returned span is exactly the number of leading steps a fresh frame-by-frame replay of prove_skip_lists accepts
(cut at the caps), and the history afterwards is the replay's. Plus the device-free facts of the new entry points: declarations, null-argument
rejections, no device, and the LDS / scratch of the fused instantiations."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "fused_span")
NONE = 0xFFFFFFFF
MAX_STEPS, BLOCK_WORDS = 8, 16384


class Row(C.Structure):
    _fields_ = [("simulated", C.c_uint32), ("has_parent", C.c_uint32), ("spawn_count", C.c_uint32), ("event_capacity", C.c_uint32), ("ublock", C.c_uint32 * 8)]


def f2u(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    """The shim is compiled here, from the file beside this test, into a temporary directory."""
    so = str(tmp_path_factory.mktemp("fused_span") / "libfused_span.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", os.path.join(HERE, "fused_span.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.fsp_new.restype = C.c_void_p
    L.fsp_new.argtypes = [C.c_int, C.c_uint32]
    L.fsp_clone.restype = C.c_void_p
    L.fsp_clone.argtypes = [C.c_void_p]
    L.fsp_free.argtypes = [C.c_void_p]
    L.fsp_mark_dirty.argtypes = [C.c_void_p]
    L.fsp_same_history.argtypes = [C.c_void_p, C.c_void_p]
    L.fsp_single.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Row), C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.fsp_span.restype = C.c_uint32
    L.fsp_span.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Row), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32]
    L.fsp_cap.restype = C.c_uint32
    L.fsp_cap.argtypes = [C.c_uint32] * 4
    return L


def rows_of(steps):
    """steps: per step a list of instances (dict: tick [float or raw bits], spawn, simulated, parent) -> Row[n_steps * n], step-major."""
    n = len(steps[0])
    arr = (Row * (len(steps) * n))()
    for s, insts in enumerate(steps):
        assert len(insts) == n
        for i, d in enumerate(insts):
            r = arr[s * n + i]
            r.simulated, r.has_parent, r.spawn_count = int(d.get("simulated", 1)), int(d.get("parent", 0)), int(d.get("spawn", 0))
            t = d.get("tick", 1 / 60)
            r.ublock[1] = t if isinstance(t, int) else f2u(t)      # the AGE_TICK's operand: U register 1
    return arr, n


class Prog:
    """A program's proof state after `warm` single frames (frame 0 spawns: a burst), with a bound published for frame `tag`."""

    def __init__(self, lib, eligible=True, warm=3, tick=1 / 60):
        self.lib, self.h, self.frame = lib, lib.fsp_new(int(eligible), 0x101), 0     # decoded operand: U register 1
        for f in range(warm):
            arr, n = rows_of([[{"tick": tick, "spawn": 1000 if f == 0 else 0}]])
            lib.fsp_single(self.h, self.frame, arr, n, NONE, 0, 1)
            self.frame += 1

    def span(self, steps, tag, bound, skip=1, fuse=1, prog=1, n_uregs=8, max_steps=MAX_STEPS, block_words=BLOCK_WORDS):
        arr, n = rows_of(steps)
        return self.lib.fsp_span(self.h, self.frame, arr, n, len(steps), n_uregs, tag, f2u(bound), skip, fuse, prog, max_steps, block_words)

    def replay(self, steps, tag, bound, skip=1):
        """A fresh copy of the history stepped frame by frame: (leading steps that prove_skip_lists accepts, the copies after each step)."""
        h = self.lib.fsp_clone(self.h)
        lead, broke, after = 0, False, []
        for s, insts in enumerate(steps):
            arr, n = rows_of([insts])
            ok = self.lib.fsp_single(h, self.frame + s, arr, n, tag, f2u(bound), skip)
            broke = broke or not ok
            lead += 0 if broke else 1
            after.append(self.lib.fsp_clone(h))
        return lead, after


def quiet(k, tick=1 / 60, n=1):
    return [[{"tick": tick} for _ in range(n)] for _ in range(k)]


def test_a_quiet_span_is_fused_whole_and_leaves_the_replays_history(lib):
    p = Prog(lib)
    steps = quiet(6)
    lead, after = p.replay(steps, tag=1, bound=0.7)
    assert lead == 6
    assert p.span(steps, tag=1, bound=0.7) == 6
    assert lib.fsp_same_history(p.h, after[5]) == 1


def test_every_premise_ends_the_span_where_the_single_frames_would(lib):
    def span_of(steps, **kw):
        return Prog(lib).span(steps, tag=1, bound=0.7, **kw)

    for k in range(8):                                           # a spawn in step k: prefix k (below two: no span)
        steps = quiet(8)
        steps[k][0]["spawn"] = 5
        assert span_of(steps) == (k if k >= 2 else 0), k
    steps = quiet(8, n=2)
    steps[0][1]["parent"] = 1                                    # an instance with a parent: never
    for st in steps:
        st[1]["parent"] = 1
    assert span_of(steps) == 0
    for bad in (-1 / 60, f2u(float("nan")) | 0, 0x7FC00001, 0x80000000 | f2u(1 / 60)):     # negative or NaN tick in step 4
        steps = quiet(8)
        steps[4][0]["tick"] = bad
        assert span_of(steps) == 4, bad
    steps = quiet(8, n=3)
    steps[5][2]["tick"] = 1 / 30                                 # instances that tick differently in step 5
    assert span_of(steps) == 5
    steps[5][2]["simulated"] = 0                                 # ... unless the odd one is frozen
    assert span_of(steps) == 8
    uneven = [[{"tick": t}] for t in (1 / 60, 1 / 120, 0.0, 1 / 30, 1 / 60)]     # ticks may differ between steps
    assert span_of(uneven) == 5
    # the bound runs out mid-span: frames 2 .. 2 + k accumulate (k + 1) / 60 on top of frame 2's own tick
    p = Prog(lib)
    steps = quiet(8)
    lead, _ = p.replay(steps, tag=1, bound=5.5 / 60)
    assert 2 <= lead < 8 and p.span(steps, tag=1, bound=5.5 / 60) == lead
    assert Prog(lib).span(quiet(8), tag=1, bound=0.0) == 0
    assert Prog(lib).span(quiet(8), tag=NONE, bound=0.7) == 0    # nothing published yet
    assert Prog(lib).span(quiet(8), tag=0, bound=0.7) == 8       # the burst frame's own bound covers what follows it
    # a bound older than 64 frames
    p = Prog(lib, warm=70, tick=1e-4)
    assert p.span(quiet(8, tick=1e-4), tag=1, bound=0.7) == 0
    lead, _ = Prog(lib, warm=70, tick=1e-4).replay(quiet(8, tick=1e-4), tag=8, bound=0.7)
    assert Prog(lib, warm=70, tick=1e-4).span(quiet(8, tick=1e-4), tag=8, bound=0.7) == (lead if lead >= 2 else 0) and 0 < lead < 8
    # dirty: a host write, a thawed instance
    p = Prog(lib)
    lib.fsp_mark_dirty(p.h)
    assert p.span(quiet(8), tag=1, bound=0.7) == 0
    # options and eligibility
    assert span_of(quiet(8), skip=0) == 0 and span_of(quiet(8), fuse=0) == 0 and span_of(quiet(8), prog=0) == 0
    assert Prog(lib, eligible=False).span(quiet(8), tag=1, bound=0.7) == 0
    # caps: HNB_MAX_FUSED_STEPS, the parameter block, at least two steps
    assert span_of(quiet(12)) == 8 and span_of(quiet(12), max_steps=5) == 5
    assert span_of(quiet(8), n_uregs=64, block_words=64 * 3) == 3
    assert span_of(quiet(8, n=4), n_uregs=64, block_words=64 * 4 * 2 + 17) == 2
    assert span_of(quiet(8), n_uregs=64, block_words=64) == 0
    assert span_of(quiet(1)) == 0
    assert lib.fsp_cap(8, 100, 8, 16384) == 8 and lib.fsp_cap(8, 1000, 8, 16384) == 2 and lib.fsp_cap(0, 0, 8, 16384) == 8


def test_a_refused_span_leaves_the_history_untouched(lib):
    p = Prog(lib)
    before = lib.fsp_clone(p.h)
    steps = quiet(8)
    steps[1][0]["spawn"] = 9
    assert p.span(steps, tag=1, bound=0.7) == 0
    assert lib.fsp_same_history(p.h, before) == 1


def test_random_spans_equal_the_frame_by_frame_replay(lib):
    rng = random.Random(20260)
    fused_total = 0
    for trial in range(400):
        warm = rng.choice([2, 3, 5, 40, 70])
        tick0 = rng.choice([1 / 60, 1 / 240, 1e-4])
        p = Prog(lib, warm=warm, tick=tick0)
        if rng.random() < 0.1:
            lib.fsp_mark_dirty(p.h)
        n, k = rng.choice([1, 1, 2, 5]), rng.randint(1, 12)
        steps = []
        for s in range(k):
            tick = rng.choice([tick0, tick0, tick0 / 2, 0.0, 2 * tick0])
            insts = [{"tick": tick} for _ in range(n)]
            r = rng.random()
            if r < 0.04:
                insts[rng.randrange(n)]["spawn"] = rng.randint(1, 100)
            elif r < 0.07:
                insts[rng.randrange(n)]["tick"] = rng.choice([-tick0, 0x7FC00000, 3 * tick0])
            elif r < 0.10:
                insts[rng.randrange(n)]["simulated"] = 0
            steps.append(insts)
        tag = rng.choice([NONE, 0, 1, max(0, warm - 2), warm - 1, warm])
        bound = rng.choice([0.0, 0.5 * k * tick0, 2 * k * tick0, 0.7, float("inf")])
        skip = 0 if rng.random() < 0.05 else 1
        cap = rng.choice([MAX_STEPS, MAX_STEPS, 3])
        lead, after = p.replay(steps, tag, bound, skip)
        want = min(lead, cap)
        want = want if want >= 2 else 0
        got = p.span(steps, tag, bound, skip=skip, max_steps=cap)
        assert got == want, (trial, got, want, lead)
        if got:
            assert lib.fsp_same_history(p.h, after[got - 1]) == 1, trial
            fused_total += got
    assert fused_total > 200      # (the generator does produce provable spans)


# ---- the new entry points without a device ------------------------------------------------------------------------------------------------------
def _header():
    txt = open(os.path.join(ROOT, "include", "hanabi_amd.h")).read()
    return txt, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_new_entries_are_declared_exported_and_bound():
    raw, code = _header()
    lib = runtime.load_library()
    for name in ("hnb_simulate_steps", "hnb_effect_set_frames_ahead", "hnb_program_set_frames_ahead", "hnb_ctx_step_stats"):
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert hasattr(lib, name) and name in runtime.ABI_SYMBOLS
    m = re.search(r"#define HNB_MAX_FUSED_STEPS (\d+)u", code)
    assert m and int(m.group(1)) >= 8 and int(m.group(1)) == runtime.MAX_FUSED_STEPS
    m = re.search(r"#define HNB_OPT_FUSE_STEPS (\d+)u", code)
    assert m and int(m.group(1)) == runtime.OPTIONS["fuse_steps"]
    assert len(set(runtime.OPTIONS.values())) == len(runtime.OPTIONS)
    fields = re.search(r"typedef struct HnbStepStats \{(.*?)\} HnbStepStats;", code, flags=re.S).group(1)
    assert re.findall(r"uint64_t (\w+);", fields) == [n for n, _ in runtime.StepStats._fields_]
    assert C.sizeof(runtime.StepStats) == 40
    assert "without hnb_effect_set_frame" in raw      # the header states what an effect without inputs does in a step


def test_null_arguments_are_rejected():
    lib = runtime.load_library()
    one = runtime.SimParams(1 / 60, 0, 1 / 60, 0, 1 / 60, 0)
    u = (C.c_uint32 * 4)()
    assert lib.hnb_simulate_steps(None, 1, C.byref(one)) == -1
    assert lib.hnb_simulate_steps(None, 0, None) == -1
    assert lib.hnb_effect_set_frames_ahead(None, 4, u, u, None) == -1
    assert lib.hnb_program_set_frames_ahead(None, 0, 1, 4, u, u, None) == -1
    assert lib.hnb_ctx_step_stats(None, None) == -1
    assert b"NULL" in lib.hnb_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="needs a box without a GPU")
def test_without_a_device_there_is_no_context_to_step():
    """hnb_simulate_steps has no device path of its own: it steps a context, and without a device hnb_ctx_create gives none (HNB_ERR_NO_DEVICE - the
    binding raises it before simulate_steps is reached); called with the handle that was never filled in it is HNB_ERR_INVALID_ARG, not a silent no-op."""
    lib = runtime.load_library()
    h = C.c_void_p()
    assert lib.hnb_ctx_create(0, C.byref(h)) == runtime.HNB_ERR_NO_DEVICE and not h.value
    with pytest.raises(bh.HanabiError) as ei:
        bh.Context(0).simulate_steps([1 / 60] * 4)
    assert ei.value.code == runtime.HNB_ERR_NO_DEVICE
    one = runtime.SimParams(1 / 60, 0, 1 / 60, 0, 1 / 60, 0)
    assert lib.hnb_simulate_steps(h, 1, C.byref(one)) == -1


def test_fused_kernels_lds_and_scratch():
    """The fused instantiations of k_update_slots_stream (last template argument FUSED = true), in the manner of tests/test_kernel_resources.py: the
    LDS the sources declare (StreamLds: 24,672 B), scratch within what that test allows the streaming kernels (640 B) - and none at all in the
    firework stack's instantiations (drag, acceleration, Euler: the headline path), whose point is to keep the planes in registers over the
    steps. Every pre-built op sequence has both cohort forms; the interpreter has no fused form."""
    from test_kernel_resources import _kernels
    # (the code object's kernel names, mangled or demangled: the last two template arguments are COHORT and FUSED)
    fused = [(n, lds, scr) for n, lds, scr in _kernels()
             if re.search(r"k_update_slots_streamI.*Lb[01]ELb1EEEv", n) or re.search(r"k_update_slots_stream<.*, (true|false), true>", n)]
    assert len(fused) >= 18, [k[0] for k in fused]
    _, code = _header()
    ops = [m for m in re.findall(r"\b(HNB_OP_[A-Z0-9_]+)\b\s*[,=}]", code[code.index("typedef enum HnbOp"):code.index("} HnbOp;") + 1])]
    op = {name: i for i, name in enumerate(ops)}
    stacks = [[op["HNB_OP_M_AGE_TICK"], op[a], op[b], op["HNB_OP_M_EULER"]] for a, b in (("HNB_OP_M_VEL_SCALE", "HNB_OP_M_VEL_ADD"), ("HNB_OP_M_VEL_ADD", "HNB_OP_M_VEL_SCALE"))]
    firework = 0
    for name, lds, scratch in fused:
        assert "ProgInterp" not in name, name
        assert lds <= 24672, (name, lds)
        assert scratch <= 640, f"{name}: {scratch} B of scratch per thread"
        for st in stacks:
            if "".join(f"Lj{o}E" for o in st) + "EE" in name or "<" + ", ".join(f"{o}u" for o in st) + ">" in name:
                firework += 1
                assert scratch == 0, f"{name}: {scratch} B of scratch per thread"
    assert firework == 4       # drag + acceleration in either order, each with and without cohorts
