"""hnb_simulate_steps (include/hanabi_amd.h): N frames per call, provable spans of list-free frames fused into one launch per program.
Every comparison is helpers.assert_same_state against an oracle stepped frame by frame: bit exact, no tolerance anywhere. That fusion
actually happened is read off hnb_ctx_step_stats."""
import numpy as np
import pytest

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects
from helpers import (EffectSpec, Frame, GpuRunner, GpuSystem, OracleRunner, OracleSystem, assert_same_state, assert_same_system_state, frame_seed,
                     translation)

pytestmark = pytest.mark.gpu
A = bh.Attribute
COHORT = {"default": None, "lean": 1, "off": 0}


def _ctx(**options):
    c = bh.Context(0)
    for k, v in options.items():
        if v is not None:
            c.set_option(k, v)
    return c


class Stepper:
    """One effect on the GPU and in the oracle, driven by the same frame script: `single` through hnb_simulate, `call` through ONE hnb_simulate_steps."""

    def __init__(self, asset, ctx):
        self.ctx, self.g, self.o = ctx, GpuRunner(asset, ctx=ctx), OracleRunner(asset, omp=True)
        self.f, self.t = 0, 0.0

    def _frame(self, dt, spawn):
        fr = Frame(dt, spawn, frame_seed(self.f), time=self.t)
        self.f += 1
        self.t += dt
        return fr

    def single(self, dt, spawn=0):
        fr = self._frame(dt, spawn)
        self.g.step(fr)
        self.o.step(fr)

    def call(self, dts, spawns=None):
        frames = [self._frame(dt, 0 if spawns is None else spawns[i]) for i, dt in enumerate(dts)]
        self.g.fx.set_frames_ahead([fr.spawn for fr in frames], [fr.seed for fr in frames])
        self.ctx.simulate_steps([(fr.dt, fr.time) for fr in frames])
        for fr in frames:
            self.o.step(fr)

    def check(self, what):
        assert_same_state(self.o.state(), self.g.state(), what)


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


# ---- 1. fusion happens and is exact ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "lean", "off"])
def test_eight_steps_after_a_burst_are_one_launch_and_exact(mode):
    """firework_trails, 1,048,576 particles: lifetimes >= 0.8, age 0.05 after the burst and two frames, eight ticks of 1/60 = 0.133: nobody can die."""
    cap = 1 << 20
    ctx = _ctx(age_cohort=COHORT[mode])
    s = Stepper(effects.firework_trails(cap), ctx)
    s.single(1 / 60, cap)
    s.single(1 / 60)
    s.single(1 / 60)
    ctx.synchronize()               # the bound the second frame computed is published by the third: visible to the host now
    before = ctx.step_stats()
    s.call([1 / 60] * 8)
    if mode == "default":           # the AGE plane as a device-side consumer reads it, without materialise (tests/test_device_view.py)
        from test_device_view import _consumer, _gather
        assert s.g.fx.device_view().stale_attr_mask == 0
        _, got, cnt = _gather(_consumer(), s.g.fx, A.AGE.id, 1, cap)
        ctx.synchronize()
        ref = s.o.state()
        n = int(cnt.item())
        assert n == len(ref["alive"]) == cap
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32)[:n], ref["attrs"]["age"].reshape(-1)[ref["alive"]])
    d = _delta(ctx.step_stats(), before)
    assert d == {"frames": 8, "fused_frames": 8, "fused_launches": 1, "update_launches": 1, "list_launches": 0}, d
    s.check(f"11 frames, {mode}")
    c = s.g.fx.check()
    assert c["ok"] == 1 and c["fault"] == 0, c
    ctx.close()


# ---- 2. uneven steps, a parameter block that differs in every step --------------------------------------------------------------------------
def _time_accel_asset(cap):
    """Burst, lifetime uniform(2, 3), AccelModifier((sin(time), -9 * time, time * time)): the uniform stream depends on `time`."""
    w = bh.ExprWriter()
    t = w.time()
    accel = bh.AccelModifier(t.sin().vec3(t * w.lit(-9.0), t * t).expr())
    init = [bh.SetAttributeModifier(A.POSITION, w.lit((0.0, 0.0, 0.0)).expr()),
            bh.SetAttributeModifier(A.VELOCITY, ((w.rand(bh.VectorType.VEC3F) * w.lit(2.0) - w.lit(1.0)) * w.lit(5.0)).expr()),
            bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr()),
            bh.SetAttributeModifier(A.LIFETIME, w.lit(2.0).uniform(w.lit(3.0)).expr())]
    asset = bh.EffectAsset(cap, bh.SpawnerSettings.once(float(cap)), w.finish())
    for m in init:
        asset = asset.init(m)
    return asset.update(accel)


@pytest.mark.parametrize("mode", ["default", "off"])
def test_uneven_steps_with_per_step_time_and_seeds(mode):
    cap = 300_000 + 77        # (a last chunk that is not full)
    ctx = _ctx(age_cohort=COHORT[mode])
    s = Stepper(_time_accel_asset(cap), ctx)
    s.single(1 / 60, cap)
    s.single(1 / 60)
    s.single(1 / 60)
    ctx.synchronize()
    before = ctx.step_stats()
    s.call([1 / 60, 1 / 120, 0.0, 1 / 30, 1 / 60])
    s.check("uneven steps")
    ctx.synchronize()
    s.call([1 / 240, 1 / 15, 1 / 60])
    s.check("uneven steps, second call")
    d = _delta(ctx.step_stats(), before)
    assert d["frames"] == 8 and d["fused_frames"] == 8 and d["fused_launches"] == 2 and d["list_launches"] == 0, d
    ctx.close()


# ---- 3. spans that end: from the burst through the complete die-off -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "lean", "off"])
def test_calls_of_four_steps_through_the_die_off(mode):
    cap = 200_000 + 13
    ctx = _ctx(age_cohort=COHORT[mode])
    s = Stepper(effects.firework_trails(cap), ctx)
    s.call([1 / 60] * 4, [cap, 0, 0, 0])
    s.check("call 0")
    for call in range(1, 21):
        s.call([1 / 60] * 4)
        s.check(f"call {call}")     # (reads back: synchronises, so the next call sees the newest published bound)
    st = ctx.step_stats()
    assert st["frames"] == 84 and 0 < st["fused_frames"] < st["frames"], st
    assert s.g.fx.alive_count() == 0
    c = s.g.fx.check()
    assert c["ok"] == 1 and c["fault"] == 0, c
    ctx.close()


# ---- 4. spawns inside a call ----------------------------------------------------------------------------------------------------------------
def test_steps_that_spawn_are_single_frames():
    cap = 1 << 18
    asset = effects.firework_trails(cap, bh.SpawnerSettings.rate(float(cap) / 1.0))
    ctx = _ctx()
    s = Stepper(asset, ctx)
    sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
    for call in range(8):
        dts = [1 / 30, 1 / 60, 1 / 60, 1 / 30]
        spawns = [sp.tick(dt, rng) for dt in dts]
        spawns[2] = 0                         # (a step without spawns between steps with: a span of one is no span)
        assert spawns[0] > 0 and spawns[3] > 0
        s.call(dts, spawns)
        s.check(f"call {call}")
    st = ctx.step_stats()
    assert st["frames"] == 32 and st["fused_frames"] == 0 and st["update_launches"] == 32, st
    ctx.close()


def test_a_spawning_step_cuts_the_span_in_front_of_it():
    """Half a burst, a bound published, then ONE call of 7 steps whose step 3 spawns into the free half: steps 0 .. 2 are one launch, step 3 and the
    quiet tail behind it are single frames (only a bound computed after the spawn covers them, and none can be visible inside the call)."""
    cap = 1 << 19
    ctx = _ctx()
    s = Stepper(effects.firework_trails(cap), ctx)
    s.single(1 / 60, cap // 2)
    s.single(1 / 60)
    s.single(1 / 60)
    ctx.synchronize()
    before = ctx.step_stats()
    s.call([1 / 60] * 7, [0, 0, 0, cap // 4, 0, 0, 0])
    d = _delta(ctx.step_stats(), before)
    assert d["frames"] == 7 and d["fused_frames"] == 3 and d["fused_launches"] == 1 and d["update_launches"] == 5, d
    s.check("spawn in step 3 of 7")
    assert s.g.fx.metadata()["alive_count"] == cap // 2 + cap // 4
    ctx.close()


@pytest.mark.parametrize("mode", ["default", "off"])
def test_bounds_published_behind_even_and_odd_spans_carry_the_die_off(mode):
    """The no-death bound rows are double-buffered by LAUNCH: a launch re-arms the row of the launch before it and writes the other, whatever the
    number of frames it covers. 2,097,152 particles (512 chunks, two rounds of the publisher's loop), spans of 2, 3, 4, 5 and 8 frames one after the other
    - each proven from the bound the launch before it left -, then calls of 2 and 3 steps through the complete die-off: every proof there rests on a
    bound published behind a fused launch, and a bound that forgot a chunk shows as a fault and as lists that differ from the oracle's."""
    cap = 1 << 21
    ctx = _ctx(age_cohort=COHORT[mode])
    s = Stepper(effects.firework_trails(cap), ctx)
    s.single(1 / 240, cap)
    s.single(1 / 240)
    s.single(1 / 240)
    ctx.synchronize()
    before = ctx.step_stats()
    for span in (2, 3, 4, 5, 8, 2, 4, 3):
        s.call([1 / 240] * span)
        ctx.synchronize()
    d = _delta(ctx.step_stats(), before)
    assert d["frames"] == 31 and d["fused_frames"] == 31 and d["fused_launches"] == 8 and d["list_launches"] == 0, d
    s.check("behind the spans")
    fused_before = ctx.step_stats()["fused_frames"]
    call = 0
    while s.g.fx.alive_count() > 0:
        s.call([1 / 60] * (2 if call % 2 else 3))
        call += 1
        if call % 6 == 0:
            s.check(f"die-off, call {call}")
        assert call < 60
    s.check("after the die-off")
    assert ctx.step_stats()["fused_frames"] > fused_before + 20       # (the flight up to the first death: about 45 frames of 1/60)
    c = s.g.fx.check()
    assert c["ok"] == 1 and c["fault"] == 0, c
    ctx.close()


# ---- 5. several instances, a frozen one, inputs through the per-program range form ----------------------------------------------------------
def test_eight_instances_per_program_inputs_and_a_frozen_one():
    n, cap = 8, 65536
    asset = effects.instancing(cap)
    ctx = _ctx()
    prog = ctx.create_program(bh.lower(asset))
    fxs = [prog.create_effect() for _ in range(n)]
    orcs = [OracleRunner(asset, omp=True) for _ in range(n)]
    xfs = [translation(float(i), 0.5 * i, -float(i)) for i in range(n)]
    frozen = set()
    f, t = [0], [0.0]

    def seeds_of(frame):
        return [frame_seed(frame, base=0xABC000 + 977 * i) for i in range(n)]

    def call(dts, spawn_first=0):
        k = len(dts)
        spawns = np.zeros((k, n), dtype=np.uint32)
        spawns[0, :] = spawn_first
        seeds = np.array([seeds_of(f[0] + j) for j in range(k)], dtype=np.uint32)
        prog.set_frames_ahead(spawns, seeds, np.array([xfs] * k, dtype=np.float32))
        params = []
        for j, dt in enumerate(dts):
            params.append((dt, t[0]))
            for i in range(n):
                if i not in frozen:
                    orcs[i].step(Frame(dt, int(spawns[j, i]), int(seeds[j, i]), transform=xfs[i], time=t[0]))
            t[0] += dt
        f[0] += k
        ctx.simulate_steps(params)

    def check(what):
        keys = ["capacity", "alive_count", "max_update", "max_spawn", "indirect_write_index", "particle_counter", "instance_count", "dead_count"]
        for i, (fx, orc) in enumerate(zip(fxs, orcs)):
            m = fx.metadata()
            got = {"counters": {k: m[k] for k in keys}, "alive": fx.alive_list(), "dead": fx.dead_list(),
                   "attrs": {a.name: fx.read_attr(a.id).view(np.uint32) for a in asset.particle_layout() if a.id >= 2}}
            assert_same_state(orc.state(), got, f"{what}, instance {i}")

    call([1 / 60] * 3, spawn_first=cap // 2)     # spawns in step 0: a single frame, then a bound has to be published first
    check("call 0")
    before = ctx.step_stats()
    call([1 / 60, 1 / 30, 1 / 60, 1 / 60])
    check("call 1")
    call([1 / 60] * 4)
    check("call 2")
    d = _delta(ctx.step_stats(), before)
    assert d["fused_frames"] == 8 and d["fused_launches"] == 2 and d["list_launches"] == 0, d     # lifetime 12 s: nobody dies
    fxs[3].set_simulated(False)
    frozen.add(3)
    call([1 / 60] * 4)
    check("instance 3 frozen")
    fxs[3].set_simulated(True)
    frozen.discard(3)
    call([1 / 60] * 4)
    check("instance 3 thawed")
    call([1 / 60] * 4)
    check("one call later")
    ctx.close()


# ---- 6. a system of linked effects next to a fusable effect ---------------------------------------------------------------------------------
def test_firework_system_runs_single_frames_beside_a_fused_effect():
    specs = [EffectSpec(effects.firework_rocket(64, 5, 200)),
             EffectSpec(effects.firework_sparkle_trail(20000), parent=0, channel=0, event_capacity=2048),
             EffectSpec(effects.firework_trails_child(60000), parent=0, channel=1, event_capacity=32768)]
    cap = 150_000
    ctx = _ctx()
    gs, os_ = GpuSystem(specs, ctx), OracleSystem(specs, omp=True)
    s = Stepper(effects.firework_trails(cap), ctx)
    sp, rng = bh.EffectSpawner(specs[0].asset.spawner), bh.Pcg32()
    f = 0
    for call in range(6):
        dts = [1 / 60] * 4
        rockets = [sp.tick(dt, rng) + (3 if (f + j) % 2 == 0 else 0) for j, dt in enumerate(dts)]
        frames = [[Frame(dt, rockets[j], frame_seed(f + j), time=(f + j) / 60), Frame(dt, 0, frame_seed(1000 + f + j), time=(f + j) / 60),
                   Frame(dt, 0, frame_seed(2000 + f + j), time=(f + j) / 60)] for j, dt in enumerate(dts)]
        for e, fx in enumerate(gs.fx):
            fx.set_frames_ahead([fr[e].spawn for fr in frames], [fr[e].seed for fr in frames])
        for fr in frames:
            os_.step(fr)
        f += 4
        s.call(dts, [cap, 0, 0, 0] if call == 0 else None)      # ONE hnb_simulate_steps for the whole context (the system's inputs were set above)
        s.check(f"call {call}: the burst effect")
        assert_same_system_state(os_.state(), gs.state(), f"call {call}: the system")
    st = ctx.step_stats()
    assert st["frames"] == 24 and st["fused_frames"] >= 12 and st["fused_launches"] >= 3, st
    # the system ran single frames: beside the burst effect's launches (one per fused span, one per frame it ran alone) every one of the 24 frames
    # launched at least one update for the three linked programs, and their lists were maintained
    own = st["fused_launches"] + (st["frames"] - st["fused_frames"])
    assert st["update_launches"] - own >= st["frames"] and st["list_launches"] >= st["frames"], st
    assert any(fx.metadata()["particle_counter"] > 0 for fx in gs.fx[1:]), "no spawn event reached a child: the system did not run"
    ctx.close()


# ---- 7. fallbacks are exact ---------------------------------------------------------------------------------------------------------------------
def test_a_ribbon_effect_runs_single_frames_inside_the_call():
    cap = 1 << 17
    asset = effects.ribbon(cap)
    ctx = _ctx()
    s = Stepper(asset, ctx)
    sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
    for call in range(10):
        dts = [1 / 60, 1 / 30, 1 / 60, 1 / 60]
        spawns = [sp.tick(dt, rng) if (call < 6 or j == 0) else 0 for j, dt in enumerate(dts)]
        s.call(dts, spawns)
        s.check(f"ribbon, call {call}")
    assert ctx.step_stats()["fused_frames"] == 0
    ctx.close()


def test_a_generic_kernel_effect_runs_single_frames_inside_the_call():
    """examples/expr.rs ("whirlwind"): the acceleration reads the particle's position, so the update runs on the generic kernel."""
    from bevy_hanabi_amd import reference_examples
    asset = reference_examples.example_expr()
    ctx = _ctx()
    s = Stepper(asset, ctx)
    assert "generic" in s.g.prog.kernel_info(), s.g.prog.kernel_info()
    sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
    for call in range(6):
        dts = [1 / 60, 1 / 30, 1 / 60, 0.5]
        s.call(dts, [sp.tick(dt, rng) if call < 4 else 0 for dt in dts])
        s.check(f"whirlwind, call {call}")
    assert ctx.step_stats()["fused_frames"] == 0 and ctx.step_stats()["frames"] == 24
    ctx.close()


def test_the_scene_of_small_effects_equals_its_single_frame_replay():
    """The 26 single-entity example effects in one context (tests/test_scene_merge.py): merged launches, set kernels, programs that are frozen, spawn
    by bursts or take new property values - 3 calls of 4 steps against a second context that replays the same script one hnb_simulate at a time.
    Properties and visibility hold for a whole call (include/hanabi_amd.h): both sides take them from the call's first step."""
    from test_reference_examples import Player
    from test_scene_merge import SceneRunner, _scene_entries
    entries = _scene_entries()
    assert len(entries) >= 20
    a, b = SceneRunner([e for _, _, e in entries], merge=True), SceneRunner([e for _, _, e in entries], merge=True)
    players = [Player(e, i) for _, i, e in entries]
    f = 0
    for _ in range(48):                                  # a prelude of single frames on both sides: the scene is populated when the calls begin
        frames = [p.frame(f) for p in players]
        f += 1
        if any(fr is not None for fr in frames):
            a.step(frames)
            b.step(frames)
    before = b.ctx.step_stats()
    for call in range(3):
        raw = [[p.frame(f + j) for p in players] for j in range(4)]
        f += 4
        shown = [fr is not None for fr in raw[0]]
        script = []
        for j in range(4):
            row = []
            for i, fr in enumerate(raw[j]):
                if not shown[i]:
                    row.append(None)
                elif fr is None:
                    row.append(Frame(raw[0][i].dt, 0, frame_seed(7000 + f + j), raw[0][i].transform, time=(f - 4 + j) * raw[0][i].dt))
                else:
                    row.append(Frame(fr.dt, fr.spawn, fr.seed, fr.transform, time=fr.time, props=fr.props if j == 0 else {}))
            script.append(row)
        if not any(shown):
            continue
        dt = next(fr.dt for fr in script[0] if fr is not None)
        for row in script:                               # the replay: one frame at a time
            a.step(row)
        for i, r in enumerate(b.runners):                # the same through ONE call
            r.fx.set_simulated(shown[i])
            if not shown[i]:
                continue
            for k, v in script[0][i].props.items():
                r.fx.set_property(k, v)
            xfs = [row[i].transform for row in script]
            r.fx.set_frames_ahead([row[i].spawn for row in script], [row[i].seed for row in script],
                                  None if xfs[0] is None else np.array(xfs, dtype=np.float32))
        b.ctx.simulate_steps([(dt, next(fr.time for fr in row if fr is not None)) for row in script])
        for (name, index, _), ra, rb in zip(entries, a.runners, b.runners):
            assert_same_state(ra.state(), rb.state(), f"scene {name}[{index}], call {call}")
    d = _delta(b.ctx.step_stats(), before)
    assert d["frames"] == 12 and d["fused_frames"] == 0, d          # every program of the scene is small: single frames, shared launches
    assert sum("merged launch" in r.prog.kernel_info() for r in b.runners) >= len(entries) // 2
    assert sum(r.fx.alive_count() for r in b.runners) > 1000
    a.ctx.close()
    b.ctx.close()


# ---- 8. HNB_OPT_FUSE_STEPS = 0 --------------------------------------------------------------------------------------------------------------
def test_fuse_steps_off_gives_the_same_state():
    cap = 1 << 19
    asset = effects.firework_trails(cap)
    on, off = _ctx(), _ctx(fuse_steps=0)
    a, b = GpuRunner(asset, ctx=on), GpuRunner(asset, ctx=off)
    o = OracleRunner(asset, omp=True)
    f = 0
    for call in range(5):
        frames = [Frame(1 / 60, cap if f + j == 0 else 0, frame_seed(f + j), time=(f + j) / 60) for j in range(6)]
        f += 6
        for r, ctx in ((a, on), (b, off)):
            r.fx.set_frames_ahead([fr.spawn for fr in frames], [fr.seed for fr in frames])
            ctx.simulate_steps([(fr.dt, fr.time) for fr in frames])
        for fr in frames:
            o.step(fr)
        d = a.fx.compare(b.fx)
        assert d["equal"] == 1, (call, d)
    assert on.step_stats()["fused_frames"] > 0 and off.step_stats()["fused_frames"] == 0 and off.step_stats()["frames"] == 30
    assert_same_state(o.state(), a.state(), "fused")
    assert_same_state(o.state(), b.state(), "single frames")
    on.close()
    off.close()


# ---- 9. the verification still notices ------------------------------------------------------------------------------------------------------
def test_the_broken_proof_hook_is_never_fused_and_still_raises_the_fault(monkeypatch):
    """HNB_OPT_TEST_BREAK_PROOF claims "nothing can die" without evidence: such frames are not fused (fused_frames stays 0 while it is set), and a
    particle that dies in one sets the metadata flag as it does under hnb_simulate. Nothing faults on the device."""
    monkeypatch.setenv("HNB_ENABLE_TEST_HOOKS", "1")
    cap = 1 << 17
    ctx = _ctx(test_break_proof=1)
    g = GpuRunner(effects.firework_trails(cap), ctx=ctx)
    f = 0
    for call in range(20):      # 80 frames at 1/60: the whole die-off
        g.fx.set_frames_ahead([cap if f + j == 0 else 0 for j in range(4)], [frame_seed(f + j) for j in range(4)])
        ctx.simulate_steps([(1 / 60, (f + j) / 60) for j in range(4)])
        f += 4
        ctx.synchronize()
    st = ctx.step_stats()
    assert st["frames"] == 80 and st["fused_frames"] == 0, st
    assert g.fx.metadata()["fault"] == 1
    assert g.fx.check()["ok"] == 0
    ctx.close()


# ---- 10. BASELINE size ----------------------------------------------------------------------------------------------------------------------
def test_c2_at_baseline_size_in_calls_of_four_steps():
    """C2 at 16,777,216 under the library defaults: burst, two frames, then 7 calls of 4 steps - the FULL state (counters, both lists, every plane of
    every slot) against the OpenMP oracle stepped frame by frame, as tests/test_gpu_scale.py does for single frames."""
    cap = 1 << 24
    ctx = _ctx()
    s = Stepper(effects.firework_trails(cap), ctx)
    s.single(1 / 60, cap)
    s.single(1 / 60)
    s.single(1 / 60)
    ctx.synchronize()
    for call in range(7):
        s.call([1 / 60] * 4)
        if call in (0, 3):
            s.check(f"c2 16.7M, call {call}")
        else:
            ctx.synchronize()
    s.check("c2 16.7M, 31 frames")
    st = ctx.step_stats()
    assert st["frames"] == 31 and st["fused_frames"] == 28 and st["fused_launches"] == 7, st
    c = s.g.fx.check()
    assert c["ok"] == 1 and c["alive_count"] == cap, c
    ctx.close()
