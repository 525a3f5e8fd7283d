"""The staging ring of the frames' parameter blocks on the device (hanabi_amd.hip ensure_stage / simulate_frame; the bookkeeping: plan::StageRing,
tests/test_stage_ring_plan.py): sixteen slots, one completion event per four staged frames. Every run here is 53 frames - three laps of the ring and
five frames - of an effect whose update reads a parameter block that differs in EVERY frame (a property set through hnb_effect_set_property times a
function of `time`, alternating ticks, a spawn count and a seed of its own), read back only at the end so that the host runs as far ahead of the
device as the ring lets it; a stale or torn block leaves a wrong velocity behind for good. Bit for bit against the oracle stepped frame by frame."""
import numpy as np
import pytest

import bevy_hanabi_amd as bh
from helpers import Frame, GpuRunner, OracleRunner, assert_same_state, frame_seed, stored_attrs

pytestmark = pytest.mark.gpu
A = bh.Attribute
CAP = 8192
FRAMES = 3 * 16 + 5
KEYS = ["capacity", "alive_count", "max_update", "max_spawn", "indirect_write_index", "particle_counter", "instance_count", "dead_count"]


def ring_asset(cap):
    """Lifetime uniform(2, 3) s (nobody dies in 53 frames); AccelModifier((k sin t, -9 t, k + t t)) with the property k and t = `time`: the
    whole operand is the host's uniform stream, evaluated once per frame into the frame's parameter block."""
    w = bh.ExprWriter()
    t, k = w.time(), w.prop(w.add_property("k", 1.0))
    accel = bh.AccelModifier((k * t.sin()).vec3(t * w.lit(-9.0), k + t * t).expr())
    init = [bh.SetAttributeModifier(A.POSITION, w.lit((0.0, 0.0, 0.0)).expr()),
            bh.SetAttributeModifier(A.VELOCITY, ((w.rand(bh.VectorType.VEC3F) * w.lit(2.0) - w.lit(1.0)) * w.lit(5.0)).expr()),
            bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr()),
            bh.SetAttributeModifier(A.LIFETIME, w.lit(2.0).uniform(w.lit(3.0)).expr())]
    asset = bh.EffectAsset(cap, bh.SpawnerSettings.once(float(cap)), w.finish())
    for m in init:
        asset = asset.init(m)
    return asset.update(accel)


def frame_of(f, cap=CAP, first=0, base=0xC0FFEE, spawns=True):
    """frame f of a script whose effect was created in frame `first`: a burst of half the capacity, then a few spawns in most frames"""
    spawn = cap // 2 if f == first else ((f * 13) % 97 if spawns else 0)
    return Frame(1 / 60 if f % 3 else 1 / 45, spawn, frame_seed(f, base), time=f / 60.0, props={"k": 0.5 + 0.25 * f})


@pytest.fixture(scope="module")
def asset():
    return ring_asset(CAP)


@pytest.fixture(scope="module")
def reference(asset):
    """the oracle's state after the 53 frames of frame_of(): computed once, never changed"""
    orc = OracleRunner(asset)
    for f in range(FRAMES):
        orc.step(frame_of(f))
    return orc.state()


@pytest.mark.parametrize("upload", ["direct", "copied", "switched"])
def test_three_laps_and_five_frames_equal_the_oracle(asset, reference, upload):
    ctx = bh.Context(0)
    if upload == "copied":
        ctx.set_option("direct_upload", 0)
    g = GpuRunner(asset, ctx=ctx)
    for f in range(FRAMES):
        if upload == "switched" and f == 26:          # in the middle of a group of slots: the slots are re-created between two frames
            ctx.set_option("direct_upload", 0)
        g.step(frame_of(f))
    assert_same_state(reference, g.state(), f"{upload}: 53 frames")
    assert g.fx.check()["ok"] == 1
    ctx.close()


def test_a_program_without_effects_and_frames_without_any(asset):
    """Two programs in one context. A loses its only effect for ten frames (20 .. 29: its program takes no part in the frame); B loses its own for
    the frames 24 .. 26, in which the context has nothing to enqueue at all: such frames take no slot, wait for nothing and record nothing."""
    ctx = bh.Context(0)
    blob = bh.lower(asset)
    progs = [ctx.create_program(blob), ctx.create_program(blob)]
    gone = [(20, 30), (24, 27)]
    base = [0xA11CE, 0xB0B]
    fx = [p.create_effect() for p in progs]
    orc = [OracleRunner(asset), OracleRunner(asset)]
    first = [0, 0]

    def state(e):
        m = e.metadata()
        return {"counters": {k: m[k] for k in KEYS}, "alive": e.alive_list(), "dead": e.dead_list(),
                "attrs": {a.name: e.read_attr(a.id).view(np.uint32) for a in stored_attrs(asset)}}

    for f in range(FRAMES):
        for i in range(2):
            if f == gone[i][0]:
                assert_same_state(orc[i].state(), state(fx[i]), f"program {i} before its effect goes, frame {f}")
                fx[i].destroy()
                fx[i] = None
            elif f == gone[i][1]:
                fx[i], orc[i], first[i] = progs[i].create_effect(), OracleRunner(asset), f
        ctx.frame_begin(1 / 60 if f % 3 else 1 / 45, f / 60.0)
        for i in range(2):
            if fx[i] is None:
                continue
            fr = frame_of(f, first=first[i], base=base[i])
            fx[i].set_property("k", fr.props["k"])
            fx[i].set_frame(fr.spawn, fr.seed)
            orc[i].step(fr)
        ctx.simulate()
    for i in range(2):
        assert_same_state(orc[i].state(), state(fx[i]), f"program {i} after 53 frames")
    ctx.close()


@pytest.mark.parametrize("programs", ["alone", "beside_a_small_one"])
def test_calls_of_three_and_five_steps(programs):
    """The same 53 frames through hnb_simulate_steps in calls of 3 and 5. The 8,192-slot effect never fuses (its frames are single frames inside the
    calls); a 70,001-slot effect without spawns does: its span is ONE staged frame whose launch reads the S blocks of that frame's slot - alone in
    its context the frames it covers enqueue nothing, beside the small effect they are the small effect's staged frames."""
    big_cap = 70_001
    caps = [CAP, big_cap] if programs == "beside_a_small_one" else [big_cap]
    assets = [ring_asset(c) for c in caps]
    ctx = bh.Context(0)
    runners = [GpuRunner(a, ctx=ctx) for a in assets]
    oracles = [OracleRunner(a, omp=True) for a in assets]
    # (the small effect goes on spawning a few particles per frame; the large one only bursts: nothing ends its spans but their length)
    frames_of = lambda f: [frame_of(f, cap=c, base=0x5EED + 31 * i, spawns=(c == CAP)) for i, c in enumerate(caps)]
    f = 0
    for _ in range(3):                                  # the burst and two quiet frames as single frames: the no-death bound is published
        ctx.frame_begin(frames_of(f)[0].dt, frames_of(f)[0].time)
        for g, o, fr in zip(runners, oracles, frames_of(f)):
            g.fx.set_property("k", fr.props["k"])
            g.fx.set_frame(fr.spawn, fr.seed)
            o.step(fr)
        ctx.simulate()
        f += 1
    ctx.synchronize()
    for n in [3, 5] * 6 + [2]:                          # 3 + 50 = 53 frames
        per = [frames_of(f + j) for j in range(n)]
        k = 0.5 + 0.25 * f
        for i, (g, o) in enumerate(zip(runners, oracles)):
            g.fx.set_property("k", k)
            g.fx.set_frames_ahead([per[j][i].spawn for j in range(n)], [per[j][i].seed for j in range(n)])
            for j in range(n):
                per[j][i].props = {"k": k}
                o.step(per[j][i])
        ctx.simulate_steps([(per[j][0].dt, per[j][0].time) for j in range(n)])
        f += n
    assert f == FRAMES
    for i, (g, o) in enumerate(zip(runners, oracles)):
        assert_same_state(o.state(), g.state(), f"{programs}: effect {i} after 53 frames")
        assert g.fx.check()["ok"] == 1
    st = ctx.step_stats()
    assert st["frames"] == FRAMES and st["fused_frames"] > 0, st      # spans were launched (their length depends on when the bound arrives)
    ctx.close()


def test_more_instances_in_frame_twenty_re_create_the_slots():
    """A program of four instances gets 500 more in frame 20: the block outgrows the slots (64 KiB at least), which are re-created between two
    frames, in the middle of a group - everything outstanding is waited for, nothing of the old ring is waited for again. The first four and two
    of the new instances against the oracle; every instance's block differs in every frame."""
    cap, grow_at, more = 256, 20, 500
    asset = ring_asset(cap)
    ctx = bh.Context(0)
    prog = ctx.create_program(bh.lower(asset))
    fxs = [prog.create_effect() for _ in range(4)]
    watched = {i: (OracleRunner(asset), 0) for i in range(4)}
    for f in range(FRAMES):
        if f == grow_at:
            fxs += [prog.create_effect() for _ in range(more)]
            watched[4] = (OracleRunner(asset), f)
            watched[len(fxs) - 1] = (OracleRunner(asset), f)
        frames = [frame_of(f, cap=cap, first=(0 if i < 4 else grow_at), base=0x1000 + 7 * i) for i in range(len(fxs))]
        ctx.frame_begin(frames[0].dt, frames[0].time)
        for i, (e, fr) in enumerate(zip(fxs, frames)):
            kk = fr.props["k"] + i
            e.set_property("k", kk)
            if i in watched:
                fr.props = {"k": kk}
                watched[i][0].step(fr)
        prog.set_frames([fr.spawn for fr in frames], [fr.seed for fr in frames])
        ctx.simulate()
    for i, (o, _) in watched.items():
        e = fxs[i]
        m = e.metadata()
        got = {"counters": {k: m[k] for k in KEYS}, "alive": e.alive_list(), "dead": e.dead_list(),
               "attrs": {a.name: e.read_attr(a.id).view(np.uint32) for a in stored_attrs(asset)}}
        assert_same_state(o.state(), got, f"instance {i} after 53 frames")
    ctx.close()
