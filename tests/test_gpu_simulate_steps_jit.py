"""hnb_simulate_steps for streamable update stacks WITHOUT a pre-built kernel (update=jit-stream): their provable spans run as one launch of the
steps kernel hiprtc builds for them (hnb_jit.h "steps modules"; hnb_program_prepare_steps). As in tests/test_gpu_simulate_steps.py every comparison is
bit exact against an oracle stepped frame by frame (or a single-frame replay context), and that fusion happened is read off hnb_ctx_step_stats."""
import os
import sys

import numpy as np
import pytest

import bevy_hanabi_amd as bh
from helpers import Frame, GpuRunner, frame_seed, translation
from steps_jit_assets import accel_radial_tangent_drag, pinned_set_accel, tangent_drag
from test_gpu_simulate_steps import COHORT, Stepper, _ctx, _delta

pytestmark = pytest.mark.gpu
CAP = 300_000 + 77            # more than 65,536 slots, a last chunk that is not full
STACKS = {"tangent_drag": tangent_drag, "accel_radial_tangent_drag": accel_radial_tangent_drag}


def _steps_line(prog):
    return [l for l in prog.kernel_info().split("\n") if l.startswith("steps kernel:")][0]


def _burst_and_bound(s, cap):
    """The burst and two quiet frames: the bound the second computed is published by the third, visible to the host after the synchronisation."""
    s.single(1 / 60, cap)
    s.single(1 / 60)
    s.single(1 / 60)
    s.ctx.synchronize()


def _uneven_calls(s, what):
    """Calls of 5 and 3 uneven steps (per-step dt, time and seeds), exact after each: 8 fused frames in 2 launches, no list kernel."""
    before = s.ctx.step_stats()
    s.call([1 / 60, 1 / 120, 0.0, 1 / 30, 1 / 60])
    s.check(f"{what}: 5 uneven steps")
    s.ctx.synchronize()
    s.call([1 / 240, 1 / 15, 1 / 60])
    s.check(f"{what}: 3 uneven steps")
    d = _delta(s.ctx.step_stats(), before)
    assert d["frames"] == 8 and d["fused_frames"] == 8 and d["fused_launches"] == 2 and d["list_launches"] == 0, d
    c = s.g.fx.check()
    assert c["ok"] == 1 and c["fault"] == 0, c


# ---- 1. parity: the two stacks, the three cohort modes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "lean", "off"])
@pytest.mark.parametrize("stack", sorted(STACKS))
def test_uneven_steps_are_fused_and_exact(stack, mode):
    ctx = _ctx(age_cohort=COHORT[mode])
    s = Stepper(STACKS[stack](CAP), ctx)
    assert "jit-stream" in s.g.prog.kernel_info(), s.g.prog.kernel_info()
    assert _steps_line(s.g.prog) == "steps kernel: not requested"
    _burst_and_bound(s, CAP)
    _uneven_calls(s, f"{stack}, {mode}")
    assert _steps_line(s.g.prog).startswith("steps kernel: built"), s.g.prog.kernel_info()
    ctx.close()


# ---- 2. a pinned SetAttributeModifier whose value depends on `time` -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "lean", "off"])
def test_pinned_set_stack_with_a_uniform_block_per_step(mode):
    ctx = _ctx(age_cohort=COHORT[mode])
    s = Stepper(pinned_set_accel(CAP), ctx)
    assert "jit-stream" in s.g.prog.kernel_info(), s.g.prog.kernel_info()
    _burst_and_bound(s, CAP)
    _uneven_calls(s, f"PIN_SET, {mode}")
    ctx.close()


# ---- 3. from the burst through the complete die-off ---------------------------------------------------------------------------------------------
def test_calls_of_four_steps_through_the_die_off():
    cap = 200_000 + 13
    ctx = _ctx()
    s = Stepper(tangent_drag(cap, life=(0.4, 0.7)), ctx)
    assert "jit-stream" in s.g.prog.kernel_info(), s.g.prog.kernel_info()
    s.call([1 / 60] * 4, [cap, 0, 0, 0])
    s.check("call 0")
    fused_at = []
    for call in range(1, 14):          # 56 frames of 1/60: 0.93 s
        s.call([1 / 60] * 4)
        s.check(f"call {call}")         # (reads back: synchronises, so the next call sees the newest published bound)
        fused_at.append(ctx.step_stats()["fused_frames"])
    st = ctx.step_stats()
    assert st["frames"] == 56 and 0 < st["fused_frames"] < st["frames"], st
    # fused frames stop where the proof stops: lifetimes are uniform(0.4, 0.7) s, so particles die in every frame from 24 to 42; the calls before
    # (frames 4 .. 27) can fuse at most what precedes the first death, the calls 7 .. 9 (frames 28 .. 39) nothing
    assert 0 < fused_at[5] <= 24 and fused_at[8] == fused_at[5], fused_at
    assert s.g.fx.alive_count() == 0
    c = s.g.fx.check()
    assert c["ok"] == 1 and c["fault"] == 0, c
    ctx.close()


# ---- 4. eight instances through the per-program range form, a frozen one, against a single-frame replay -----------------------------------------
def test_eight_instances_equal_their_single_frame_replay():
    n, cap = 8, 70_000 + 1
    blob = bh.lower(tangent_drag(cap))
    a, b = _ctx(), _ctx()
    pa, pb = a.create_program(blob), b.create_program(blob)
    assert "jit-stream" in pa.kernel_info(), pa.kernel_info()
    fa, fb = [pa.create_effect() for _ in range(n)], [pb.create_effect() for _ in range(n)]
    xfs = np.array([translation(float(i), 0.5 * i, -float(i)) for i in range(n)], dtype=np.float32)
    f, t = [0], [0.0]

    def call(dts, spawn_first=0):
        k = len(dts)
        spawns = np.zeros((k, n), dtype=np.uint32)
        spawns[0, :] = spawn_first
        seeds = np.array([[frame_seed(f[0] + j, base=0xABC000 + 977 * i) for i in range(n)] for j in range(k)], dtype=np.uint32)
        pa.set_frames_ahead(spawns, seeds, np.array([xfs] * k))
        params = []
        for j, dt in enumerate(dts):
            params.append((dt, t[0]))
            pb.set_frames(spawns[j], seeds[j], xfs)          # the replay: one hnb_simulate per step
            b.frame_begin(dt, t[0])
            b.simulate()
            t[0] += dt
        f[0] += k
        a.simulate_steps(params)

    def check(what):
        for i, (x, y) in enumerate(zip(fa, fb)):
            d = x.compare(y)
            assert d["equal"] == 1, (what, i, d)

    call([1 / 60] * 3, spawn_first=cap)
    check("call 0")
    before = a.step_stats()
    call([1 / 60, 1 / 30, 1 / 60, 1 / 60])
    check("call 1")
    call([1 / 60] * 4)
    check("call 2")
    d = _delta(a.step_stats(), before)
    assert d["fused_frames"] == 8 and d["fused_launches"] == 2 and d["list_launches"] == 0, d
    fa[3].set_simulated(False)
    fb[3].set_simulated(False)
    call([1 / 60] * 4)
    check("instance 3 frozen")
    fa[3].set_simulated(True)
    fb[3].set_simulated(True)
    call([1 / 60] * 4)
    check("instance 3 thawed")
    call([1 / 60] * 4)
    check("one call later")
    assert b.step_stats()["fused_frames"] == 0 and a.step_stats()["fused_frames"] >= 12
    assert all(x.check()["fault"] == 0 for x in fa)
    a.close()
    b.close()


# ---- 5. hnb_program_prepare_steps ---------------------------------------------------------------------------------------------------------------
def test_prepare_steps_before_the_first_call(tmp_path, monkeypatch):
    monkeypatch.setenv("HNB_JIT_CACHE", str(tmp_path / "cache"))
    asset = tangent_drag(CAP)
    ctx = _ctx()
    s = Stepper(asset, ctx)
    assert "jit-stream" in s.g.prog.kernel_info(), s.g.prog.kernel_info()
    s.g.prog.prepare_steps()
    assert _steps_line(s.g.prog) == "steps kernel: built", s.g.prog.kernel_info()        # compiled: the cache was empty
    s.g.prog.prepare_steps()                                                             # (again: nothing to do)
    _burst_and_bound(s, CAP)
    before = ctx.step_stats()
    s.call([1 / 60] * 4)
    d = _delta(ctx.step_stats(), before)
    assert d["fused_frames"] == 4 and d["fused_launches"] == 1, d                        # the first call is already fused
    s.check("first call")
    ctx.close()
    ctx2 = _ctx()
    g2 = GpuRunner(asset, ctx=ctx2)
    g2.prog.prepare_steps()
    assert _steps_line(g2.prog) == "steps kernel: built (jit cache hit)", g2.prog.kernel_info()
    ctx2.close()


def test_prepare_steps_does_nothing_where_no_steps_kernel_is_needed():
    from bevy_hanabi_amd import effects, reference_examples
    ctx = _ctx()
    for asset, why in ((effects.firework_trails(1 << 17), "pre-built fused kernel"), (reference_examples.example_expr(), "never fuses"), (effects.ribbon(1 << 17), "never fuses")):
        prog = ctx.create_program(bh.lower(asset))
        prog.prepare_steps()
        line = _steps_line(prog)
        assert line.startswith("steps kernel: not requested") and why in line, line
    ctx.close()


# ---- 6. fallbacks are exact ---------------------------------------------------------------------------------------------------------------------
def test_without_specialisation_the_stack_runs_single_frames(monkeypatch):
    monkeypatch.setenv("HNB_JIT", "0")
    ctx = _ctx()
    s = Stepper(tangent_drag(CAP), ctx)
    assert "interp-stream" in s.g.prog.kernel_info(), s.g.prog.kernel_info()
    s.g.prog.prepare_steps()
    assert _steps_line(s.g.prog).startswith("steps kernel: not requested (never fuses"), s.g.prog.kernel_info()
    _burst_and_bound(s, CAP)
    s.call([1 / 60, 1 / 120, 0.0, 1 / 30, 1 / 60])
    s.check("interpreter, 5 steps")
    s.call([1 / 240, 1 / 15, 1 / 60])
    s.check("interpreter, 3 steps")
    st = ctx.step_stats()
    assert st["frames"] == 11 and st["fused_frames"] == 0 and st["update_launches"] == 11, st
    ctx.close()


def test_fuse_steps_off_gives_the_same_state():
    asset = tangent_drag(CAP)
    on, off = _ctx(), _ctx(fuse_steps=0)
    a, b = GpuRunner(asset, ctx=on), GpuRunner(asset, ctx=off)
    assert "jit-stream" in a.prog.kernel_info(), a.prog.kernel_info()
    f = 0
    for call in range(5):
        frames = [Frame(1 / 60, CAP if f + j == 0 else 0, frame_seed(f + j), time=(f + j) / 60) for j in range(6)]
        f += 6
        for r, ctx in ((a, on), (b, off)):
            r.fx.set_frames_ahead([fr.spawn for fr in frames], [fr.seed for fr in frames])
            ctx.simulate_steps([(fr.dt, fr.time) for fr in frames])
        d = a.fx.compare(b.fx)
        assert d["equal"] == 1, (call, d)
    assert on.step_stats()["fused_frames"] > 0 and off.step_stats()["fused_frames"] == 0 and off.step_stats()["frames"] == 30
    assert _steps_line(b.prog) == "steps kernel: not requested"          # (nothing was built for a context that never fuses)
    on.close()
    off.close()


# ---- 7. HNB_OPT_JIT_ASYNC with an empty cache ---------------------------------------------------------------------------------------------------
def test_async_specialisation_with_an_empty_cache(tmp_path, monkeypatch):
    """Every call is exact whether or not the modules have arrived (interpreter, then the specialised single-frame kernel, then the steps kernel);
    hnb_program_prepare_steps waits for what is in flight, and the next eligible call is fused."""
    monkeypatch.setenv("HNB_JIT_CACHE", str(tmp_path / "empty"))
    ctx = _ctx(jit_async=1)
    s = Stepper(tangent_drag(CAP), ctx)
    _burst_and_bound(s, CAP)
    for call in range(3):
        s.call([1 / 60] * 4)
        s.check(f"call {call}, {s.g.prog.kernel_info().splitlines()[0]}, {_steps_line(s.g.prog)}")
    s.g.prog.prepare_steps()
    info = s.g.prog.kernel_info()
    assert "jit-stream" in info and "pending" not in info and _steps_line(s.g.prog).startswith("steps kernel: built"), info
    ctx.synchronize()
    before = ctx.step_stats()
    s.call([1 / 60] * 4)
    d = _delta(ctx.step_stats(), before)
    assert d["fused_frames"] == 4 and d["fused_launches"] == 1, d
    s.check("after prepare_steps")
    c = s.g.fx.check()
    assert c["ok"] == 1 and c["fault"] == 0, c
    ctx.close()


# ---- 8. BASELINE size ---------------------------------------------------------------------------------------------------------------------------
def test_tangent_drag_at_baseline_size_in_calls_of_four_steps():
    """16,777,216 slots under the library defaults: burst, two frames, then 7 calls of 4 steps; a slab of 16,384 slots against an oracle effect fed
    the same frames (tools/steps_ab.py's check: a burst gives slot i the PRNG stream of particle slot_base + i)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import steps_ab
    cap, dt = 1 << 24, 1 / 60
    ctx = _ctx()
    prog = ctx.create_program(bh.lower(steps_ab.make_asset("tangent_drag", cap)))
    assert "jit-stream" in prog.kernel_info(), prog.kernel_info()
    fx = prog.create_effect()
    f = 0
    for _ in range(3):
        ctx.frame_begin(dt, f * dt)
        fx.set_frame(cap if f == 0 else 0, steps_ab.frame_seed(f))
        ctx.simulate()
        f += 1
    ctx.synchronize()
    for call in range(7):
        fx.set_frames_ahead([0] * 4, [steps_ab.frame_seed(f + j) for j in range(4)])
        ctx.simulate_steps([(dt, (f + j) * dt) for j in range(4)])
        f += 4
        ctx.synchronize()
    slab = steps_ab.slab_check(fx, cap, f, dt, asset_name="tangent_drag")
    assert slab["ok"] and slab["alive_in_slab"] == 16384, slab
    st = ctx.step_stats()
    assert st["frames"] == 31 and st["fused_frames"] == 28 and st["fused_launches"] == 7, st
    c = fx.check()
    assert c["ok"] == 1 and c["alive_count"] == cap and c["fault"] == 0, c
    ctx.close()
