"""Every simulation modifier at its edge operands (tests/modifier_lattice.py) ON THE GPU, the full state - planes, alive and dead lists, counters -
bit for bit against the oracle, on every path that evaluates a modifier:

  * each table with its parameters as effect properties ("props": one instance per parameter row; the streaming kernels, the pre-built sequences
    aot-stream:<name> where the stack matches one, interp-stream / jit-stream otherwise) and read from per-particle planes ("planes": interp-generic /
    jit-generic), under HNB_JIT=0 and HNB_JIT=1 (a hiprtc compile of the same headers; init=jit);
  * the force field's modifiers in another order, which has no pre-built sequence;
  * the position and velocity modifiers in the INIT context (SetPositionSphere / Circle / Cone3d, SetVelocitySphere / Circle / Tangent, the emitter
    transform with a zero row and with infinite entries): one spawning frame per parameter row, init=interp and init=jit, list-major and slot-major init;
  * the shared launches that small programs of one context take: every table, both forms, cut to a few hundred rows, one context per dt;
  * the component-wise sequences over 2 * 4096 + 300 particles, all alive, the lattice rows at slots 0.., across 4095 | 4096 and in the partial chunk,
    with `transpose` on and off: with the burst's common age and lifetime left alone the two whole chunks stream FLAT and the partial one does not (the
    conditions are argued, and the cohort state asserted, at the tests), with ages and lifetimes written per row none does; the same through
    hnb_simulate_steps in calls of four frames, `fuse_steps` on and off, fused frames asserted;
  * ages and lifetimes at their edges (NaN, +-inf, -0, subnormals, age + dt one ulp either side of the lifetime) written by the host under the proofs the
    frames are planned from: twelve frames with ticks of 1/60, 0, 1e-6, -1/120 ... and a re-spawn, under the default options and with cull_lifetime,
    skip_lists, age_cohort and horizon flipped, and through hnb_simulate_steps.

Every case asserts from Program.kernel_info() that the path it names ran. That the oracle itself is right at these operands is
tests/test_modifier_lattice.py's half (no GPU). The GPU-only copies of the semantics (apply_static, the flat path, the hiprtc compiles) are reached
through these path assertions."""
import numpy as np
import pytest

import bevy_hanabi_amd as bh
import helpers
import modifier_lattice as mdl
from helpers import A, Frame, GpuGroup, GpuRunner, OracleRunner, RunnerGroup, assert_same_state, modifier_probe_asset, run_modifier_table
from test_modifier_lattice import age_frames, age_oracle_states, oracle_states, start_age_lattice

pytestmark = pytest.mark.gpu


def expected_kernels(t, form, jit):
    """the first line of Program.kernel_info() for a table's probe"""
    streams = t.streamable and (form == "props" or not t.ops)
    aot = mdl.prebuilt_sequence(t) if streams else None
    update = f"aot-stream:{aot}" if aot else (("jit-" if jit else "interp-") + ("stream" if streams else "generic"))
    return ("init=jit" if jit else "init=interp") + " update=" + update


def _cases():
    out = []
    for name, t in mdl.tables().items():
        for form in ("props", "planes"):
            for jit in (0, 1):
                out.append(pytest.param(name, form, jit, id=f"{name}-{form}-HNB_JIT={jit}-{expected_kernels(t, form, jit).replace(' ', '-')}"))
    return out


def _first_line(prog):
    return prog.kernel_info().split("\n")[0]


@pytest.mark.parametrize("name, form, jit", _cases())
def test_table_on_the_gpu(name, form, jit, monkeypatch):
    monkeypatch.setenv("HNB_JIT", str(jit))
    t = mdl.tables()[name]
    asset, operands = modifier_probe_asset(t, form)
    ctx = bh.Context(0)
    try:
        g = GpuGroup(asset, 1 if form == "planes" else t.P, ctx)
        got = run_modifier_table(g, t, form, operands)
        line = _first_line(g.prog)
        assert expected_kernels(t, form, jit) in line and "merged launch" not in g.prog.kernel_info(), g.prog.kernel_info()
        for i, (r, s) in enumerate(zip(oracle_states(name, form), got)):
            assert_same_state(r, s, f"{name} [{form}] HNB_JIT={jit} [{line}], instance {i}")
        assert all(fx.metadata()["fault"] == 0 for fx in g.fx)
        print(f"{name} [{form}] ({t.P} x {t.Q}): {line}")
    finally:
        ctx.close()


@pytest.mark.parametrize("jit", [0, 1], ids=["interp-stream", "jit-stream"])
def test_another_order_of_a_prebuilt_stack(jit, monkeypatch):
    """KillSphere, KillAabb, Conform, Conform: the force field's modifiers backwards match no pre-built sequence"""
    monkeypatch.setenv("HNB_JIT", str(jit))
    t = mdl.tables()["force_field"]
    order = list(range(len(t.ops)))[::-1]
    asset, operands = modifier_probe_asset(t, "props", order=order)
    ref = run_modifier_table(RunnerGroup(OracleRunner, lambda: modifier_probe_asset(t, "props", order=order)[0], t.P), t, "props", operands)
    ctx = bh.Context(0)
    try:
        g = GpuGroup(asset, t.P, ctx)
        got = run_modifier_table(g, t, "props", operands)
        assert ("init=jit update=jit-stream" if jit else "init=interp update=interp-stream") in _first_line(g.prog), g.prog.kernel_info()
        for i, (r, s) in enumerate(zip(ref, got)):
            assert_same_state(r, s, f"force field backwards HNB_JIT={jit}, instance {i}")
    finally:
        ctx.close()


def _shared_groups():
    """{dt: [table names]}: one hnb_simulate has one dt, so the tables of each dt share a context of their own"""
    out = {}
    for name, t in mdl.tables().items():
        out.setdefault(float(t.dt), []).append(name)
    return out


@pytest.mark.parametrize("dt", list(_shared_groups()), ids=lambda d: f"dt={d:.6g}")
def test_tables_through_the_shared_launches_of_small_programs(dt):
    """Small independent programs of one context share the frame's job-table launches (hnb_plan.h plan_merged_launches): interpreter instantiations of
    their own - streaming, generic and generic with the wide register file -, behind another kernel entry than the per-program launches. Every table,
    both forms, cut to a few hundred rows; EVERY program must report both frames as served by a merged launch. The wide-file family (Conform read from
    planes: 36 .. 44 update registers) merges only from two such programs on, the streaming and narrow generic ones from two in all: where a dt has
    Conform alone, the force field's two probes run beside it."""
    tables = [mdl.tables()[n] for n in _shared_groups()[dt]]
    if any(t.name.startswith("conform") for t in tables) and not any(t.name == "force_field" for t in tables):
        beside = mdl.cut(mdl.tables()["force_field"], 384)
        beside.name, beside.dt = "force_field_beside", np.float32(dt)
        tables.append(beside)
    runs = []
    ctx = bh.Context(0)
    ctx.set_option("scene_merge", 1)
    try:
        for full in tables:
            for form in ("props", "planes"):
                t = mdl.cut(full, 384, params=2 if form == "props" else None)
                asset, operands = modifier_probe_asset(t, form)
                count = 1 if form == "planes" else t.P
                ref = run_modifier_table(RunnerGroup(OracleRunner, lambda: modifier_probe_asset(t, form)[0], count), t, form, operands)
                runs.append((t, form, operands, GpuGroup(asset, count, ctx), ref))
        assert len(runs) >= 2
        # the two frames of run_modifier_table, every program in the same hnb_simulate
        ctx.frame_begin(1 / 60, 0.0)
        for t, form, operands, g, _ in runs:
            for fx in g.fx:
                fx.set_frame(t.n if form == "planes" else t.Q, 1, None)
        ctx.simulate()
        for t, form, operands, g, _ in runs:
            for i in range(len(g.fx)):
                get = (lambda what: t.particle(what)) if form == "planes" else (lambda what: getattr(t, what))
                if not t.no_motion:
                    g.write_attr(i, A.POSITION, np.ascontiguousarray(get("pos")))
                    g.write_attr(i, A.VELOCITY, np.ascontiguousarray(get("vel")))
                g.write_attr(i, A.AGE, np.ascontiguousarray(get("age")))
                g.write_attr(i, A.LIFETIME, np.ascontiguousarray(get("lifetime")))
                for attr, plane in (operands.planes.items() if form == "planes" else ()):
                    g.write_attr(i, attr, plane)
                for k, v in (operands.props[i].items() if form == "props" else ()):
                    g.fx[i].set_property(k, v)
        ctx.frame_begin(dt, 1 / 60)
        for t, form, operands, g, _ in runs:
            for fx in g.fx:
                fx.set_frame(0, t.seed, None)
        ctx.simulate()
        wide = 0
        for t, form, operands, g, ref in runs:
            info = g.prog.kernel_info()
            wide += "wide-file" in info.split("\n")[0]
            line = [l for l in info.split("\n") if l.startswith("update served by a merged launch")]
            assert line and line[0].endswith(": 2 frames"), (t.name, form, info)
            for i, (r, s) in enumerate(zip(ref, g.states())):
                assert_same_state(r, s, f"{t.name} [{form}] in the shared launch, instance {i}")
        assert wide >= 2 or not any(t.name.startswith(("conform", "force_field")) for t, *_ in runs), wide
        print(f"shared launches at dt {dt}: {len(runs)} programs ({wide} wide-file), {sum(len(r[3].fx) for r in runs)} instances: update served by a merged launch in both frames")
    finally:
        ctx.close()


# ---- the position and velocity modifiers in the init context --------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot_init", [0, 2], ids=["slot_init=0", "slot_init=2"])
@pytest.mark.parametrize("jit", [0, 1], ids=["init=interp", "init=jit"])
@pytest.mark.parametrize("name", list(mdl.init_tables()))
def test_init_modifiers_on_the_gpu(name, jit, slot_init, monkeypatch):
    """one spawning frame per parameter row (its properties, its emitter transform), list-major and slot-major init: the full state against the oracle"""
    from test_modifier_lattice import init_oracle_states
    monkeypatch.setenv("HNB_JIT", str(jit))
    t = mdl.init_tables()[name]
    asset, props = helpers.init_probe_asset(t)
    ctx = bh.Context(0)
    ctx.set_option("slot_init", slot_init)
    try:
        g = GpuGroup(asset, t.P, ctx)
        got = helpers.run_init_table(g, t, props)
        assert ("init=jit" if jit else "init=interp") in _first_line(g.prog), g.prog.kernel_info()
        for i, (r, s) in enumerate(zip(init_oracle_states(name), got)):
            assert_same_state(r, s, f"{name} HNB_JIT={jit} slot_init={slot_init}, instance {i}")
    finally:
        ctx.close()


# ---- the component-wise sequences over whole and partial chunks: the flat path of the streaming kernel ------------------------------------------------
# update_stream_chunk (csrc/hnb_kernels.hip.h) streams a chunk FLAT - position and velocity as plain float arrays, the component of a vec3 operand
# picked by a rotation (apply_static_flat) - where
#     flat = chunk_full && ast == 1 && cull && Lm > 0 && age_after(A) < Lm && position and velocity are loaded && LIFETIME is not stored
# in the cohort instantiation of a component-wise program. The "burst" runs below meet every term in the two whole chunks from the second frame on:
#   * the burst fills the effect, and the update of the spawning frame counts 4096 alive slots and no casualty per whole chunk: chunk_full;
#   * the init gives every particle age 0 and lifetime 1e9, and nobody writes AGE or LIFETIME afterwards, so the survivors of a chunk share one age: the
#     chunk's cohort state is 1 (asserted below from kernel_info's "age cohorts: N of M chunks", which reads the state words), age_cohort being on by
#     default for an asset whose render modifiers do not read AGE; lifetime culling is on by default;
#   * the host writes POSITION and VELOCITY only. hnb_effect_write_attr zeroes the chunks' lifetime bounds (Lm), keeps the completely-alive flags and,
#     AGE not being written, the cohort states; the first frame behind the write loads the lifetimes in every step and republishes Lm = 1e9;
#   * age_after(A) is a few ticks, far below 1e9: from the second frame behind the write on, chunks 0 and 1 stream flat. Chunk 2 has 300 slots: never full.
# The lattice rows sit at slots 0.., across 4095 | 4096 and in the partial chunk, every edge in ONE of x, y, z: a wrong rotation moves it to another
# component. The "written" runs write AGE and LIFETIME per row as well (rows that die, mixed ages): no chunk is a cohort, none streams flat.
BIG_TABLES = [stack + tag for stack in mdl.BIG_STACKS for tag in ("", "_dt4", "_dtfma")]


def run_big(group, t, operands, count, frames, ages):
    """the burst, the host's write, `frames` update frames: the states after each. ages "written": AGE and LIFETIME are written per row too"""
    group.step([Frame(1 / 60, t.Q, 1) for _ in range(count)])
    for i in range(count):
        group.write_attr(i, A.POSITION, np.ascontiguousarray(t.pos))
        group.write_attr(i, A.VELOCITY, np.ascontiguousarray(t.vel))
        if ages == "written":
            group.write_attr(i, A.AGE, np.ascontiguousarray(t.age))
            group.write_attr(i, A.LIFETIME, np.ascontiguousarray(t.lifetime))
    out = []
    for f in range(frames):
        group.step(big_frames(t, operands, count, f))
        out.append(group.states())
    return out


def big_frames(t, operands, count, f):
    return [Frame(float(t.dt), 0, t.seed + f, time=(1 + f) / 60, props=operands.props[i % t.P]) for i in range(count)]


_BIG_REF = {}


def big_reference(name, ages):
    """(table, asset, operands, {frame: the oracle's states after it} for the frames the tests compare), computed once"""
    if (name, ages) not in _BIG_REF:
        t = mdl.big_table(name)
        asset, operands = modifier_probe_asset(t, "props")
        o = RunnerGroup(OracleRunner, lambda: modifier_probe_asset(t, "props")[0], t.P)
        states = run_big(o, t, operands, t.P, 6, ages)
        _BIG_REF[name, ages] = (t, asset, operands, {f: states[f] for f in (0, 1, 2, 5)})
    return _BIG_REF[name, ages]


def _cohort_chunks(prog):
    line = [l for l in prog.kernel_info().split("\n") if l.startswith("age cohorts: ")]
    assert line and " of " in line[0], prog.kernel_info()
    return int(line[0].split()[2])


def _instances(t):
    return max(t.P, 6)      # instances x 3 chunks above the 16 chunks up to which a program counts as small and never runs fused spans


@pytest.mark.parametrize("transpose", [1, 0], ids=["transpose=1", "transpose=0"])
@pytest.mark.parametrize("ages", ["burst", "written"])
@pytest.mark.parametrize("name", BIG_TABLES)
def test_componentwise_sequences_over_whole_and_partial_chunks(name, ages, transpose):
    """three frames behind the host's write, each against the oracle. "burst": the second and third stream chunks 0 and 1 flat (see above)"""
    t, asset, operands, ref = big_reference(name, ages)
    count = _instances(t)
    ctx = bh.Context(0)
    ctx.set_option("transpose", transpose)
    try:
        g = GpuGroup(asset, count, ctx)
        got = run_big(g, t, operands, count, 3, ages)
        assert f"update=aot-stream:{mdl.prebuilt_sequence(t)}" in _first_line(g.prog), g.prog.kernel_info()
        for f in range(3):
            for i, s in enumerate(got[f]):
                assert_same_state(ref[f][i % t.P], s, f"{name} [{ages}] over {mdl.BIG_CAPACITY} slots transpose={transpose}, frame {f}, instance {i}")
        if ages == "burst":
            assert _cohort_chunks(g.prog) >= 2 * count, g.prog.kernel_info()      # the two whole chunks of every instance keep one age in a word
            assert all(s["counters"]["alive_count"] == mdl.BIG_CAPACITY for s in got[2])
    finally:
        ctx.close()


@pytest.mark.parametrize("fuse", [1, 0], ids=["fuse_steps=1", "fuse_steps=0"])
@pytest.mark.parametrize("ages", ["burst", "written"])
@pytest.mark.parametrize("name", mdl.BIG_STACKS)
def test_componentwise_sequences_through_simulate_steps(name, ages, fuse):
    """Two single frames behind the host's write (the device publishes the bound the spans are proven from), then four frames in ONE call: with fuse_steps
    on, frames of it run in the fused instantiation of the pre-built kernel - "burst": flat in chunks 0 and 1."""
    t, asset, operands, ref = big_reference(name, ages)
    count = _instances(t)
    ctx = bh.Context(0)
    ctx.set_option("fuse_steps", fuse)
    try:
        g = GpuGroup(asset, count, ctx)
        run_big(g, t, operands, count, 2, ages)
        ctx.synchronize()
        before = ctx.step_stats()["fused_frames"]
        for fx in g.fx:
            fx.set_frames_ahead([0, 0, 0, 0], [t.seed + f for f in range(2, 6)])
        ctx.simulate_steps([(float(t.dt), (1 + f) / 60) for f in range(2, 6)])
        assert f"update=aot-stream:{mdl.prebuilt_sequence(t)}" in _first_line(g.prog), g.prog.kernel_info()
        for i, s in enumerate(g.states()):
            assert_same_state(ref[5][i % t.P], s, f"{name} [{ages}] six frames, the last four in one call, fuse_steps={fuse}, instance {i}")
        st = ctx.step_stats()
        print(f"{name} [{ages}] fuse_steps={fuse}: {st}")
        assert st["frames"] == 7 and ((st["fused_frames"] - before >= 2) if fuse else st["fused_frames"] == 0), st
        if ages == "burst":
            assert _cohort_chunks(g.prog) >= 2 * count, g.prog.kernel_info()
    finally:
        ctx.close()


# ---- ages and lifetimes at their edges under the host's proofs --------------------------------------------------------------------------------
AGE_OPTIONS = [{}, {"cull_lifetime": 0}, {"skip_lists": 0}, {"age_cohort": 0}, {"age_cohort": 2}, {"horizon": 0}]


@pytest.mark.parametrize("options", AGE_OPTIONS, ids=lambda o: "defaults" if not o else ",".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("which", helpers.AGE_LATTICE_ASSETS)
def test_age_lattice_frame_by_frame(which, options):
    want = age_oracle_states(which)
    ctx = bh.Context(0)
    for k, v in options.items():
        ctx.set_option(k, v)
    try:
        g = GpuRunner(helpers.age_lattice_asset(which, mdl.AGE_CAPACITY), ctx=ctx)
        start_age_lattice(g)
        for f, fr in enumerate(age_frames()):
            g.step(fr)
            assert_same_state(want[f], g.state(), f"{which} {options} frame {f} (dt {fr.dt})")
            assert g.fx.metadata()["fault"] == 0, (which, options, f)
        info = g.prog.kernel_info().split("\n")
        print(f"{which} {options}: {info[0]}; " + "; ".join(l for l in info if l.startswith(("lists skipped", "death horizons", "age cohorts"))))
    finally:
        ctx.close()


class _Instances:
    """start_age_lattice's runner interface over the instances of a GpuGroup"""

    def __init__(self, group):
        self.g = group

    def step(self, fr):
        self.g.step([fr for _ in self.g.fx])

    def write_attr(self, attr_id, plane):
        for fx in self.g.fx:
            fx.write_attr(attr_id, plane)


@pytest.mark.parametrize("which", helpers.AGE_LATTICE_ASSETS)
def test_age_lattice_through_simulate_steps(which):
    """Five instances (20 chunks: above the 16 up to which a program never runs fused spans). Four single frames behind the host's write - the device
    publishes bounds computed from the written planes -, then two calls of four frames; the re-spawn is the last step of the first call."""
    want = age_oracle_states(which)
    frames = age_frames()
    ctx = bh.Context(0)
    try:
        g = GpuGroup(helpers.age_lattice_asset(which, mdl.AGE_CAPACITY), 5, ctx)
        r = _Instances(g)
        start_age_lattice(r)
        for f in range(4):
            r.step(frames[f])
            for i, s in enumerate(g.states()):
                assert_same_state(want[f], s, f"{which} frame {f}, instance {i}")
        ctx.synchronize()
        for first in (4, 8):
            call = frames[first:first + 4]
            for fx in g.fx:
                fx.set_frames_ahead([fr.spawn for fr in call], [fr.seed for fr in call])
            ctx.simulate_steps([(fr.dt, fr.time) for fr in call])
            for i, s in enumerate(g.states()):
                assert_same_state(want[first + 3], s, f"{which} frames {first} .. {first + 3} in one call, instance {i}")
            assert all(fx.metadata()["fault"] == 0 for fx in g.fx), (which, first)
        print(f"{which}: {ctx.step_stats()}\n{g.prog.kernel_info()}")
    finally:
        ctx.close()
