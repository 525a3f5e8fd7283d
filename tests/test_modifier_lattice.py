"""Every simulation modifier at its edge operands (tests/modifier_lattice.py), on the CPU: the oracle against an independent numpy
reference written from the reference's WGSL text, and the product's copy of the arithmetic (hnb_vm.h compiled for the host,
CpuVmRunner) against the oracle, bit for bit, through the streaming and the generic interpreter.

Each table runs in two forms (helpers.modifier_probe_asset): "props", every parameter an effect property - uniform operands, a streamable
program, one effect per parameter row -, and "planes", every parameter read from a per-particle attribute plane - the generic interpreter,
one effect over all P * Q rows. Float planes are compared by bits (NaN as a class), the alive set exactly.
tests/test_gpu_modifier_lattice.py runs the same tables on the GPU.
"""
import functools

import numpy as np
import pytest

import helpers
import math_lattice as ml
import modifier_lattice as mdl
import oracle
from helpers import A, CpuVmRunner, OracleRunner, RunnerGroup, assert_same_state, modifier_probe_asset, program_mnemonics, run_modifier_table

f32, u32 = np.float32, np.uint32
TABLES = list(mdl.tables())
FORMS = ["props", "planes"]


def _each(fn):
    return lambda x: np.array([fn(float(v)) for v in np.asarray(x, f32)], f32)


# the transcendental builtins inside the drawing shapes are taken from the oracle, element by element (tests/math_lattice.py pins them)
BUILTINS = {"sin": _each(lambda v: oracle.math1(0, v)), "cos": _each(lambda v: oracle.math1(1, v)), "acos": _each(lambda v: oracle.math1(8, v)),
            "sqrt": _each(lambda v: oracle.math1(10, v)), "cbrt": _each(lambda v: oracle.math2(0, v, float(f32(1.0 / 3.0))))}


@functools.lru_cache(None)
def reference(name, form):
    """the numpy reference over the P * Q rows; the particle index of a row is its slot in its effect"""
    t = mdl.tables()[name]
    return mdl.ref_update(t, BUILTINS, index=np.arange(t.n) if form == "planes" else t.qrow())


def flatten(t, states):
    """the states of a run (one effect, or one per parameter row) as planes over the P * Q rows: {"pos", "vel", "age": float32, "alive": bool}"""
    m = len(states[0]["attrs"]["age"])
    out = {"age": np.concatenate([s["attrs"]["age"][:, 0] for s in states]).view(f32)}
    if not t.no_motion:
        out["pos"] = np.concatenate([s["attrs"]["position"] for s in states]).view(f32)
        out["vel"] = np.concatenate([s["attrs"]["velocity"] for s in states]).view(f32)
    alive = np.zeros(m * len(states), bool)
    for i, s in enumerate(states):
        alive[i * m + s["alive"].astype(np.int64)] = True
    out["alive"] = alive
    assert len(alive) == t.n
    return out


@functools.lru_cache(None)
def oracle_states(name, form):
    """the oracle's states of a table: computed once, shared by the tests of this module and by the GPU tests"""
    t = mdl.tables()[name]
    asset, operands = modifier_probe_asset(t, form)
    count = 1 if form == "planes" else t.P
    return run_modifier_table(RunnerGroup(OracleRunner, lambda: modifier_probe_asset(t, form)[0], count), t, form, operands)


def check_against_reference(t, got, want, what):
    for k in ("pos", "vel", "age"):
        if k in got:
            ops = [t.prow(), t.qrow()]
            ml.check_bits(f"{what} {k} (parameter row, particle row)", got[k], want[k], *ops)
    bad = np.flatnonzero(got["alive"] != want["alive"])
    assert not len(bad), f"{what}: alive differs at rows {bad[:8]} (parameter row {t.prow()[bad[:8]]}, particle {t.qrow()[bad[:8]]}): want {want['alive'][bad[:8]]}"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", TABLES)
def test_oracle_against_the_reference(name, form):
    t = mdl.tables()[name]
    got, want = flatten(t, oracle_states(name, form)), reference(name, form)
    check_against_reference(t, got, want, f"{name} [{form}] oracle")
    cols = [want[k].reshape(t.n, -1) for k in ("pos", "vel", "age") if k in got]
    share = min(float((~np.isnan(c)).mean()) for c in np.concatenate(cols, axis=1).T)
    print(f"{name} [{form}]: {t.n} rows ({t.P} parameter rows x {t.Q} particles), least non-NaN share of a column {share:.2f}, {int((~want['alive']).sum())} dead")


@pytest.mark.parametrize("force_generic", [False, True], ids=["as-lowered", "force-generic"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", TABLES)
def test_host_build_of_the_product_against_the_oracle(name, form, force_generic):
    t = mdl.tables()[name]
    asset, operands = modifier_probe_asset(t, form)
    count = 1 if form == "planes" else t.P
    g = RunnerGroup(CpuVmRunner, lambda: modifier_probe_asset(t, form)[0], count, force_generic=force_generic)
    got = run_modifier_table(g, t, form, operands)
    for i, (r, s) in enumerate(zip(oracle_states(name, form), got)):
        assert_same_state(r, s, f"{name} [{form}] cpu_vm force_generic={force_generic}, effect {i}")


# ---- the conditions on the tables, asserted on the reference alone -------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLES)
def test_the_table_is_not_mostly_nan_and_reaches_its_edges(name):
    t = mdl.tables()[name]
    want = reference(name, "planes")
    keys = ("age",) if t.no_motion else ("pos", "vel", "age")
    planes = np.concatenate([want[k].reshape(t.n, -1) for k in keys], axis=1)
    for c, col in enumerate(planes.T):
        assert (~np.isnan(col)).mean() >= 0.5, f"{name}: output column {c} is NaN in {int(np.isnan(col).sum())} of {t.n} rows"
    clean = ~np.isnan(planes).any(axis=1)
    edges = t.edges()
    for kind, mask in edges.items():
        assert mask.shape == (t.n,) and mask.any(), f"{name}: no row has the edge '{kind}'"
        if kind in t.nan_is_the_point:
            assert np.isnan(planes[mask]).any(), f"{name}: '{kind}' is listed as a NaN by design, and no row of it is NaN"
        else:
            assert (mask & clean).any(), f"{name}: every row with the edge '{kind}' is NaN"
    assert set(t.nan_is_the_point) <= set(edges), name
    if name in mdl.KILL_TABLES:
        dead = float((~want["alive"]).mean())
        assert 0.1 <= dead <= 0.9, f"{name}: {dead:.2f} of the rows are killed"
    print(f"{name}: {t.n} rows, non-NaN share {float((~np.isnan(planes)).mean()):.2f}, {int((~want['alive']).sum())} killed, edges: {', '.join(f'{k} ({int(m.sum())})' for k, m in edges.items())}")


def test_the_draws_are_the_pinned_ones():
    """modifier_lattice's numpy pcg_hash / to_float01 / frand against the oracle's, which are pinned to the reference's vectors"""
    xs = np.array([0, 1, 2, 0x5EED, 0xC0FFEE, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 123456789, 0xDEADBEEF], u32)
    assert [int(v) for v in mdl.pcg_hash(xs)] == [oracle.pcg_hash(int(v)) for v in xs]
    assert [float(v) for v in mdl.to_float01(xs)] == [oracle.to_float01(int(v)) for v in xs]
    for x in xs:
        state, vals = oracle.frand_kat(int(x), 1)
        seed, v = mdl.frand(np.array([x], u32))
        assert (int(seed[0]), float(v[0])) == (state, vals[0])


# ---- what the probes lower to --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TABLES)
def test_the_probes_lower_to_the_intended_macro_ops(name):
    t = mdl.tables()[name]
    want = ["M_AGE_TICK"] + [op.mnemonic() for op in t.ops] + ([] if t.no_motion else ["M_EULER"])
    asset, _ = modifier_probe_asset(t, "props")
    got = program_mnemonics(helpers.bh.lower(asset))["update"]
    assert got == want, (name, got)
    assert CpuVmRunner(asset).streamable == t.streamable, name
    asset, _ = modifier_probe_asset(t, "planes")
    ops = program_mnemonics(helpers.bh.lower(asset))["update"]
    assert [o for o in ops if o.startswith("M_") and o != "M_PIN_SET"] == want, (name, ops)
    assert not CpuVmRunner(asset).streamable or not t.ops, name


def test_transform_users_are_rejected_in_update():
    """SetPositionCone3d, SetVelocityCircle and SetVelocityTangent read the emitter transform, which the update pass does not have. Lowering refuses each
    with a message that names it; the oracle, which evaluates, refuses each at the first particle it updates."""
    bh = helpers.bh
    builders = {"SetPositionCone3dModifier": lambda w: bh.SetPositionCone3dModifier(w.lit(1.0).expr(), w.lit(1.0).expr(), w.lit(0.5).expr(), bh.ShapeDimension.Volume),
                "SetVelocityCircleModifier": lambda w: bh.SetVelocityCircleModifier(w.lit((0.0, 0.0, 0.0)).expr(), w.lit((0.0, 1.0, 0.0)).expr(), w.lit(1.0).expr()),
                "SetVelocityTangentModifier": lambda w: bh.SetVelocityTangentModifier(w.lit((0.0, 0.0, 0.0)).expr(), w.lit((0.0, 1.0, 0.0)).expr(), w.lit(1.0).expr())}
    for who, build in builders.items():
        w = bh.ExprWriter()
        m = build(w)
        inits = [bh.SetAttributeModifier(a, w.lit((0.0, 0.0, 0.0)).expr()) for a in (A.POSITION, A.VELOCITY)]
        asset = bh.EffectAsset(16, bh.SpawnerSettings.once(16.0), w.finish())
        for i in inits:
            asset.init(i)
        asset.update(m)
        with pytest.raises(bh.ShaderGenerateError) as err:
            bh.lower(asset)
        assert str(err.value) == f"{who} uses the emitter transform, which is only defined in the init context", (who, str(err.value))
        fx = oracle.OracleEffect(bh.serialize_asset(asset))
        with pytest.raises(oracle.OracleError) as err:
            fx.step(1 / 60, 16, 1)
        assert "transform is not defined in the update shader" in str(err.value), (who, str(err.value))


# ---- ages and lifetimes at their edges, through twelve frames ------------------------------------------------------------------------------
def age_frames():
    """the twelve frames of the age lattice: ticks of 1/60, 0, 1e-6, -1/120 ..., a re-spawn of 300 in frame 8"""
    out, time = [], 2 / 60
    for f, dt in enumerate(mdl.AGE_TICKS):
        out.append(helpers.Frame(dt, mdl.AGE_RESPAWN[1] if f == mdl.AGE_RESPAWN[0] else 0, helpers.frame_seed(10 + f), time=time))
        time += dt
    return out


def start_age_lattice(runner):
    """a burst that fills the effect, one ordinary frame (the bounds of the host's proofs exist), then AGE and LIFETIME written by the host"""
    runner.step(helpers.Frame(1 / 60, mdl.AGE_CAPACITY, helpers.frame_seed(0)))
    runner.step(helpers.Frame(1 / 60, 0, helpers.frame_seed(1), time=1 / 60))
    age, life, _ = mdl.age_lifetime_planes()
    write = runner.write_attr if hasattr(runner, "write_attr") else runner.fx.write_attr
    write(A.AGE.id, age)
    write(A.LIFETIME.id, life)


@functools.lru_cache(None)
def age_oracle_states(which):
    """the oracle's state after each of the twelve frames: computed once, shared with the GPU tests"""
    o = OracleRunner(helpers.age_lattice_asset(which, mdl.AGE_CAPACITY))
    start_age_lattice(o)
    out = []
    for fr in age_frames():
        o.step(fr)
        out.append(o.state())
    return out


@pytest.mark.parametrize("which", helpers.AGE_LATTICE_ASSETS)
def test_age_lattice_on_the_host(which):
    """The alive set after the first frame is (age + dt) < lifetime in numpy binary32 over the written planes, and the oracle has it; the host build of the
    product follows the oracle through all twelve frames, as lowered and through the generic interpreter."""
    states = age_oracle_states(which)
    age, life, where = mdl.age_lifetime_planes()
    want = mdl.ref_alive_after_tick(age, life, mdl.AGE_TICKS[0])
    got = np.zeros(mdl.AGE_CAPACITY, bool)
    got[states[0]["alive"].astype(np.int64)] = True
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"{which}: alive after the first frame differs at slots {bad[:8]}: age {age[bad[:8]]} lifetime {life[bad[:8]]}"
    assert 0 < want[where].sum() < len(where)                      # the edge rows fall on both sides
    assert states[-1]["counters"]["alive_count"] < states[mdl.AGE_RESPAWN[0] - 1]["counters"]["alive_count"] + mdl.AGE_RESPAWN[1]   # deaths go on after the re-spawn
    assert states[mdl.AGE_RESPAWN[0]]["counters"]["alive_count"] > states[mdl.AGE_RESPAWN[0] - 1]["counters"]["alive_count"]     # ... which found free slots
    for force_generic in (False, True):
        v = CpuVmRunner(helpers.age_lattice_asset(which, mdl.AGE_CAPACITY), force_generic=force_generic)
        start_age_lattice(v)
        for f, fr in enumerate(age_frames()):
            v.step(fr)
            assert_same_state(states[f], v.state(), f"{which} cpu_vm force_generic={force_generic} frame {f}")
    print(f"{which}: {int(want.sum())} of {mdl.AGE_CAPACITY} alive after the first frame ({int(want[where].sum())} of {len(where)} edge rows), "
          f"{states[-1]['counters']['alive_count']} after the twelfth")


# ---- the position and velocity modifiers in the init context ---------------------------------------------------------------------------------
INIT_TABLES = list(mdl.init_tables())


@functools.lru_cache(None)
def init_oracle_states(name):
    t = mdl.init_tables()[name]
    asset, props = helpers.init_probe_asset(t)
    return helpers.run_init_table(RunnerGroup(OracleRunner, lambda: helpers.init_probe_asset(t)[0], t.P), t, props)


@pytest.mark.parametrize("name", INIT_TABLES)
def test_init_modifiers_against_the_reference(name):
    """what the init stores right behind the position and the velocity modifier (F32X3_0, F32X3_1): the oracle against the numpy reference by bits, the host
    build of the product against the oracle's full state"""
    t = mdl.init_tables()[name]
    states = init_oracle_states(name)
    want = mdl.ref_init(t, BUILTINS)
    rows = [np.repeat(np.arange(t.P), t.Q), np.tile(np.arange(t.Q), t.P)]
    for key, attr in (("pos", "f32x3_0"), ("vel", "f32x3_1")):
        got = np.concatenate([s["attrs"][attr] for s in states]).view(f32)
        ml.check_bits(f"{name} oracle {key} (parameter row, slot)", got, want[key], *rows)
        for c in range(3):
            assert (~np.isnan(want[key][:, c])).mean() >= 0.5, (name, key, c)
    assert all(s["counters"]["alive_count"] == t.Q for s in states)
    # every named edge is reached by a row whose stored position and velocity are not NaN, or is listed as a NaN by design (and is one)
    planes = np.concatenate([want["pos"], want["vel"]], axis=1)
    clean = ~np.isnan(planes).any(axis=1)
    edges = t.edges()
    assert edges and set(t.nan_is_the_point) <= set(edges), name
    for kind, mask in edges.items():
        assert mask.any(), f"{name}: no row has the edge '{kind}'"
        if kind in t.nan_is_the_point:
            assert np.isnan(planes[mask]).any(), f"{name}: '{kind}' is listed as a NaN by design, and no row of it is NaN"
        else:
            assert (mask & clean).any(), f"{name}: every row with the edge '{kind}' is NaN"
    _, props = helpers.init_probe_asset(t)
    for force_generic in (False, True):
        got = helpers.run_init_table(RunnerGroup(CpuVmRunner, lambda: helpers.init_probe_asset(t)[0], t.P, force_generic=force_generic), t, props)
        for i, (r, s) in enumerate(zip(states, got)):
            assert_same_state(r, s, f"{name} cpu_vm force_generic={force_generic}, effect {i}")
    print(f"{name}: {t.n} rows ({t.P} parameter rows x {t.Q} spawns), non-NaN share {float((~np.isnan(np.concatenate([want['pos'], want['vel']], axis=1))).mean()):.2f}")
