"""include/hanabi_amd.h promises "same results bit for bit with either value" for the switches of hnb_ctx_set_option. Here every creation-time and
per-frame option (tests/option_scripts.py: CLASSES) meets the oracle: flipped singly from the defaults and from the all-off PLAIN set, crossed in
full where the options pick the update kernel's template (age_cohort x cull_lifetime x horizon, specialised and ahead-of-time kernels), switched
BETWEEN frames of one effect (the per-chunk state words - lmin, cfull, the cohort state - survive the switch), inside merged launches, and on random
programs at capacities that fill chunks. Of `stream_hints` and `overlap_updates` only the plumbing runs at these sizes (tests/option_scripts.py);
`fuse_steps` has its own case at 17 chunks, the smallest size at which a span can fuse.

Every run compares the whole state - counters, both lists, every plane - with the oracle after EVERY frame (a stale chunk word can heal within a few
frames), and runs hnb_effect_check at the frames where the oracle's chunks change state. The scripts' preconditions are asserted without a GPU in
tests/test_option_scripts.py. A flip that never reaches its code tests nothing: where hnb_program_kernel_info carries a counter it is asserted in
both directions (expected_engagement). Three options have no counter; what gates them and why the assets reach it:

  transpose      hnb_kernels.hip.h, update_stream_chunk's step_body: `xp = args.transpose != 0 && ... step_first + kStepRows <= capacity && at least 32
                 quads of the step hold a live particle` - the per-particle path of every streamable program with vec3 planes. The force field (a
                 non-flat stack: ConformToSphere) takes it in every frame with enough particles; the firework takes it whenever a chunk is not on
                 the flat path (cohorts off, or a chunk that is not completely alive), and falls back to the direct path late in its die-off.
  alternate      hanabi_amd.hip, the update launch: `cb.xcd_remap = ... (ctx->alternate && !(p->frames_run & 1u) ? 2u : 0u)` - every second frame of
                 every program with more than one chunk walks the chunks downwards (all scripts here have at least two chunks).
  cull_lifetime  hnb_program.h cull_eligible (fixed at creation): `cull = args.cull_lifetime != 0` in update_stream_chunk gates the per-chunk lifetime
                 bound lmin[j], the skipped LIFETIME loads (`need_life`), and - through the facts derived from it - cohorts, death horizons and
                 list-free frames. Firework and force field both have AGE + LIFETIME and a streamable update: eligible.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import option_scripts as S
from bevy_hanabi_amd import runtime
from helpers import A, Frame, GpuRunner, OracleRunner, assert_same_state, frame_seed, stored_attrs
from test_fuzz import _run, _run_typed
from test_lowering_cpu import ZOO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

BASES = {"defaults": {}, "plain": S.PLAIN}
RECHECKED_BY = 87   # the chunks hold one age again from frame 71 on; a chunk found mixed is looked at again in one frame of sixteen: frames 71 .. 86


def expected_engagement(name, options):
    """{counter: bool} - must the counter of hnb_program_kernel_info be > 0 (True) or == 0 (False) after the whole script under these options?
    From the creation-time facts of hnb_program.h and the frame proofs of hnb_plan.h: list-free frames, cohorts and horizons all need lifetime
    culling; AUTO keeps per-particle ages for an AGE-reading asset below 65,536 slots; the force field kills (no horizons, no list-free frames) and is not lean (cohorts only with ALL);
    a ribbon has neither cohorts nor horizons. Only the facts this module is sure of are listed."""
    o = lambda k: S.base_value(options, k)
    cull = o("cull_lifetime") == 1
    out = {}
    if name == "firework":
        out["lists_skipped"] = bool(o("skip_lists") and cull)
        out["horizon_frames"] = bool(o("horizon") and cull)
        out["cohort_chunks"] = bool(cull and o("age_cohort") in (1, 2))
        out["slot_init_frames"] = o("slot_init") == 2      # (1, "where it pays", asks for 17 chunks or more: plan::kSlotInitMinChunks)
    elif name == "force_field":
        out["lists_skipped"] = False
        out["horizon_frames"] = False
        out["cohort_chunks"] = bool(cull and o("age_cohort") == 2)
    elif name == "ribbon":
        out["cohort_chunks"] = False
        out["horizon_frames"] = False
        out["slot_init_frames"] = False
        if not o("suffix_proof") or not o("skip_lists"):    # (plan::prove_ribbon_order: both proofs stand on the sorted head, which skip_lists keeps)
            out["suffix_frames"] = out["ring_frames"] = False
        if not o("ring_lists"):
            out["ring_frames"] = False
        if options.keys() <= {"suffix_proof", "ring_lists", "skip_lists", "alternate"} and o("suffix_proof") and o("ring_lists") and o("skip_lists"):
            out["suffix_frames"] = out["ring_frames"] = True      # (from the defaults: the trail of examples/ribbon.rs is what both proofs were made for)
    return out


def run_life_cycle(name, cap, options, before_frame=None, flight_cohorts=True):
    """One script on the GPU under `options`, against the oracle's trace after every frame; hnb_effect_check at the transition frames;
    the engagement counters at the end. `before_frame(ctx, f)`: option switches between frames."""
    tr = S.trace(name, cap)
    ctx = S.make_context(options)
    try:
        g = GpuRunner(tr.asset, ctx=ctx)
        want = expected_engagement(name, options)
        checks = set(tr.transition_frames())
        flight = tr.flight_frame()
        for f, fr in enumerate(tr.frames):
            if before_frame is not None:
                before_frame(ctx, f)
            g.step(fr)
            tr.assert_frame(f, g.state(), f"{options}")
            if f in checks:
                c = g.fx.check()
                assert c["ok"] == 1 and c["alive_count"] == tr.alive_counts[f], (f, c)
            if flight_cohorts and "cohort_chunks" in want and f in (flight, RECHECKED_BY):
                i = S.parse_kernel_info(g.prog.kernel_info())
                print(f"{name}@{cap} {options} frame {f}: age cohorts {i['cohort_chunks']} of {i['cohort_total']}")
                if want["cohort_chunks"] and (f == flight or name == "firework"):   # state 1 exactly where the oracle's chunk holds one age (0: empty, 4: mixed)
                    assert i["cohort_chunks"] == sum(tr.uniform(f, j) for j in range(tr.n_chunks())) > 0, (f, i)
                if not want["cohort_chunks"]:
                    assert i["cohort_chunks"] == 0, (f, i)
        text = g.prog.kernel_info()
        info = S.parse_kernel_info(text)
        print(f"{name}@{cap} {options}: {info}")
        assert info["frames_run"] == len(tr.frames), text
        assert g.fx.metadata()["fault"] == 0
        if before_frame is None:   # HNB_OPT_DIRECT_UPLOAD: every frame's parameter block went the way the option says (where the device has a large BAR)
            direct = S.base_value(options, "direct_upload") == 1 and info["large_bar"]
            assert (info["direct_frames"], info["copied_frames"]) == ((len(tr.frames), 0) if direct else (0, len(tr.frames))), text
        return text, info, want
    finally:
        ctx.close()


def assert_engagement(info, want, skip=()):
    for k, engaged in want.items():
        if k in skip or k == "cohort_chunks":    # (the cohort count is a state, asserted at the flight frames)
            continue
        assert (info[k] > 0) == engaged, (k, info[k], "expected > 0" if engaged else "expected == 0")


# ---- one flip from the defaults, one flip from PLAIN --------------------------------------------------------------------------------------------
def _flip_cases(options=None):
    return [pytest.param(base, flip, id=f"{base}-{S.flip_id(flip)}") for base in BASES for flip in S.single_flips(BASES[base], options)]


def _base_cases():
    return [pytest.param(base, None, id=f"{base}-as-is") for base in BASES]


def _options(base, flip):
    o = dict(BASES[base])
    if flip is not None:
        o[flip[0]] = flip[1]
    return o


@pytest.mark.parametrize("base, flip", _base_cases() + _flip_cases())
def test_firework_life_cycle_with_one_option_flipped(base, flip):
    _, info, want = run_life_cycle("firework", S.FIREWORK_CAP, _options(base, flip))
    assert_engagement(info, want)


@pytest.mark.parametrize("cap", [4095, 4096, 4097])
@pytest.mark.parametrize("cohort", [1, 2])
def test_firework_life_cycle_around_one_chunk_with_cohorts(cap, cohort):
    """4095: cfull is never set; 4096: one chunk, exactly; 4097: a second chunk of one slot"""
    _, info, want = run_life_cycle("firework", cap, {"age_cohort": cohort})
    assert_engagement(info, want)


@pytest.mark.parametrize("base, flip", _base_cases() + _flip_cases(("transpose", "alternate", "cull_lifetime", "age_cohort", "skip_lists")))
def test_force_field_life_cycle_with_one_option_flipped(base, flip):
    _, info, want = run_life_cycle("force_field", S.FORCE_FIELD_CAP, _options(base, flip))
    assert_engagement(info, want)


@pytest.mark.parametrize("base, flip", _base_cases() + _flip_cases(("suffix_proof", "ring_lists", "skip_lists", "alternate")))
def test_ribbon_life_cycle_with_one_option_flipped(base, flip):
    _, info, want = run_life_cycle("ribbon", S.RIBBON_CAP, _options(base, flip))
    assert_engagement(info, want)


# ---- the AGE plane as a device-side reader sees it, on both sides of AUTO's threshold --------------------------------------------------------------
def _consumer():
    lib = C.CDLL(os.path.join(ROOT, "tests", "device_view", "libconsumer.so"))
    lib.consumer_gather.argtypes = [C.POINTER(runtime.DeviceView), C.c_uint32, C.c_void_p, C.c_void_p]
    return lib


def _age_cases():
    flips = [("age_cohort", v) for v in (3, 0, 1, 2)] + [("transpose", 0), ("cull_lifetime", 0)]
    return [pytest.param(cap, flip, id=f"{cap}-{S.flip_id(flip)}") for cap in (S.AUTO_THRESHOLD - 1, S.AUTO_THRESHOLD) for flip in flips]


@pytest.mark.parametrize("cap, flip", _age_cases())
def test_age_reading_asset_on_both_sides_of_the_auto_threshold(cap, flip):
    """firework_trails (ColorOverLifetime / SizeOverLifetime read AGE) at 65,535 and 65,536 slots. The header (HNB_OPT_AGE_COHORT, "Device-side
    output"): the AGE plane is current after every frame with OFF, with AUTO below 65,536 slots (per-particle ages) and with AUTO from 65,536 slots on
    (cohorts, the update writes the common age as it goes) - read here through hnb_effect_device_view WITHOUT materialise, right behind
    hnb_simulate; with LEAN / ALL it is stale (stale_attr_mask) until hnb_effect_materialise - read with it. Without lifetime culling there are no
    cohorts and nothing is stale. The ages of the alive rows, then the whole state, against the oracle after every frame. The flips start from the
    defaults only: from PLAIN lifetime culling is off, no cohort code is reachable and the plane is simply current - the cull_lifetime=0 id is that
    case. (The host read of the state materialises too; the next frame's update rewrites the age of every alive slot before the next device-side read.)"""
    import torch
    cons = _consumer()
    options = {flip[0]: flip[1]}
    mode, cull = S.base_value(options, "age_cohort"), S.base_value(options, "cull_lifetime")
    stale = bool(cull and mode in (1, 2))
    tr = S.trace("firework_short", cap)
    ctx = S.make_context(options)
    try:
        g = GpuRunner(tr.asset, ctx=ctx)
        assert g.fx.device_view().stale_attr_mask == ((1 << A.AGE.id) if stale else 0)
        checks = set(tr.transition_frames())
        out = torch.zeros(cap, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for f, fr in enumerate(tr.frames):
            g.step(fr)
            if stale:
                g.fx.materialise([A.AGE.id])
            v = g.fx.device_view()
            assert cons.consumer_gather(C.byref(v), int(A.AGE.id), out.data_ptr(), cnt.data_ptr()) == 0     # enqueued behind the frame; nothing has synchronised
            ctx.synchronize()
            n = int(cnt.item())
            assert n == tr.alive_counts[f], (f, n, tr.alive_counts[f])
            rows = out.cpu().numpy().view(np.uint32)[:n]
            if hashlib.blake2b(np.ascontiguousarray(rows).tobytes(), digest_size=16).digest() != tr.row_ages[f]:
                ref = tr.oracle_state(f)
                np.testing.assert_array_equal(rows, ref["attrs"]["age"].reshape(-1)[ref["alive"]], err_msg=f"{options} frame {f}: ages of the alive rows as a device-side reader sees them")
            tr.assert_frame(f, g.state(), f"{options}")
            if f in checks:
                assert g.fx.check()["ok"] == 1, f
            if f == tr.flight_frame():
                assert S.parse_kernel_info(g.prog.kernel_info())["cohort_chunks"] == (tr.n_chunks() if cull and mode != 0 and (mode != 3 or cap >= S.AUTO_THRESHOLD) else 0)
        i = S.parse_kernel_info(g.prog.kernel_info())
        print(f"firework_short@{cap} {options}: {i}")
        auto_cohorts = cull and mode == 3 and cap >= S.AUTO_THRESHOLD
        assert i["cohort_plane_current"] == bool(auto_cohorts) and i["cohort_auto_off"] == bool(cull and mode == 3 and cap < S.AUTO_THRESHOLD), g.prog.kernel_info()
        assert (i["cohort_total"] > 0) == bool(stale or auto_cohorts)
    finally:
        ctx.close()


# ---- the options that pick the update kernel's template, crossed in full ---------------------------------------------------------------------------
@pytest.mark.parametrize("jit", ["1", "0"])
@pytest.mark.parametrize("horizon", [0, 1])
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("cohort", [0, 1, 2, 3])
def test_creation_time_options_crossed(cohort, cull, horizon, jit, monkeypatch):
    monkeypatch.setenv("HNB_JIT", jit)
    text, info, want = run_life_cycle("firework", S.FIREWORK_CAP, {"age_cohort": cohort, "cull_lifetime": cull, "horizon": horizon})
    assert_engagement(info, want)
    first = text.split("\n")[0]
    assert ("jit" in first) == (jit == "1"), first


# ---- hnb_simulate_steps, fused and not -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cohort", [3, 1])
@pytest.mark.parametrize("fuse", [1, 0])
def test_firework_through_simulate_steps_at_seventeen_chunks(fuse, cohort):
    """HNB_OPT_FUSE_STEPS acts on hnb_simulate_steps alone, and only on a program of more than 16 chunks (hanabi_amd.hip fuse_candidate: never a
    candidate for the merged launches) - the other cases of this module, at 4 chunks, run single frames whatever the option says. Here: the short
    firework script at 17 chunks in calls of four frames. Calls in which provably nothing spawns or dies run as one fused launch with fuse_steps=1
    (hnb_ctx_step_stats: fused_frames > 0) and as single frames with 0 (== 0); compared with the oracle after every call - a fused span has no
    state in between. Cohort AUTO keeps the AGE plane current at this size (the flat path's age store inside a fused launch), LEAN does not.
    tests/test_gpu_simulate_steps.py holds the fused kernel itself against the oracle at larger sizes."""
    tr = S.trace("firework_short", S.FUSE_CAP)
    ctx = S.make_context({"fuse_steps": fuse, "age_cohort": cohort})
    try:
        g = GpuRunner(tr.asset, ctx=ctx)
        for first in range(0, len(tr.frames), 4):
            span = tr.frames[first:first + 4]
            g.fx.set_frames_ahead([fr.spawn for fr in span], [fr.seed for fr in span])
            ctx.simulate_steps([(fr.dt, fr.time) for fr in span])
            last = first + len(span) - 1
            tr.assert_frame(last, g.state(), f"fuse_steps={fuse}")
            if any(f in tr.transition_frames() for f in range(first, last + 1)):
                assert g.fx.check()["ok"] == 1, last
        st = ctx.step_stats()
        print(f"fuse_steps={fuse} age_cohort={cohort}: {st}")
        assert st["frames"] == len(tr.frames) and g.fx.metadata()["fault"] == 0
        if fuse:
            assert st["fused_frames"] >= 8 and st["fused_launches"] >= 2, st     # (the flight before the first deaths alone is ten quiet calls)
        else:
            assert st["fused_frames"] == 0 and st["fused_launches"] == 0, st
    finally:
        ctx.close()


# ---- switching between frames ----------------------------------------------------------------------------------------------------------------------
SWITCH_CASES = [("firework", S.FIREWORK_CAP, cohort) for cohort in (3, 1, 2, 0)] + [("ribbon", S.RIBBON_CAP, 3)]


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("name", ["firework", "ribbon"])
def test_a_random_option_switched_before_every_frame(name, seed):
    """Most options "apply from the next hnb_simulate on", and the chunk words the previous frames left stay: one random frame-class option is set to a
    random legal value before every frame. (The firework's cohort mode, fixed at creation, goes round with the seed: AUTO, LEAN, ALL, OFF.)"""
    rng = np.random.default_rng(1000 + seed)
    cap = S.FIREWORK_CAP if name == "firework" else S.RIBBON_CAP
    creation = {"age_cohort": (3, 1, 2, 0)[seed % 4]} if name == "firework" else {}
    log = []

    def switch(ctx, f):
        k = S.FRAME[int(rng.integers(len(S.FRAME)))]
        v = S.values_of(k)[int(rng.integers(len(S.values_of(k))))]
        log.append((f, k, v))
        ctx.set_option(k, v)

    try:
        run_life_cycle(name, cap, creation, before_frame=switch, flight_cohorts=False)
    except AssertionError:
        print("switches:", log[-12:])
        raise


@pytest.mark.parametrize("name, cap, cohort", SWITCH_CASES, ids=[f"{n}-cohort{c}" for n, _, c in SWITCH_CASES])
def test_transpose_alternate_and_skip_lists_switched_every_frame(name, cap, cohort):
    """frame f runs with transpose = bit 0, alternate = bit 1, skip_lists = bit 2 of f: every transition frame of the script (and its neighbours)
    meets a switch of at least one of them, and all eight combinations follow each other"""
    def switch(ctx, f):
        ctx.set_option("transpose", f & 1)
        ctx.set_option("alternate", f >> 1 & 1)
        ctx.set_option("skip_lists", f >> 2 & 1)

    run_life_cycle(name, cap, {"age_cohort": cohort} if name == "firework" else {}, before_frame=switch, flight_cohorts=False)


# ---- merged launches -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_module", [runtime.SET_MODULE_OFF, runtime.SET_MODULE_CACHED], ids=["set-off", "set-cached"])
@pytest.mark.parametrize("merge", [1, 0])
def test_a_program_that_lives_in_merged_launches(merge, set_module):
    """Two small programs in one context share their launches (HNB_OPT_SCENE_MERGE): the firework at 4097 slots - burst, completely alive, die-off,
    partial respawn, re-burst, died out, burst - never runs a launch of its own, so whatever the quartered merged kernels do not maintain of the
    chunk words (lmin, cfull) must not show. A second instance of it is frozen for frames 40 - 60 and lags behind from then on; its oracle is
    stepped only when it is simulated. All three effects against their oracles after every frame."""
    cap = S.CHUNK + 1
    tr = S.trace("firework", cap)
    zoo_asset = ZOO["update_all_macros"]()
    ctx = S.make_context({"scene_merge": merge, "set_module": set_module})
    try:
        g = GpuRunner(tr.asset, ctx=ctx)
        lag_fx, lag_orc = g.prog.create_effect(), OracleRunner(tr.asset)
        z, z_orc = GpuRunner(zoo_asset, ctx=ctx), OracleRunner(zoo_asset)
        zcap = zoo_asset.capacity
        keys = ["capacity", "alive_count", "max_update", "max_spawn", "indirect_write_index", "particle_counter", "instance_count", "dead_count"]
        checks = set(tr.transition_frames())
        for f, fr in enumerate(tr.frames):
            frozen = 40 <= f <= 60
            zfr = Frame(fr.dt, zcap // 2 if f == 0 else (zcap // 9 if f % 11 == 0 else 0), frame_seed(5000 + f), time=fr.time)
            lfr = Frame(fr.dt, fr.spawn, frame_seed(9000 + f), time=fr.time)
            ctx.frame_begin(fr.dt, fr.time)
            g.fx.set_frame(fr.spawn, fr.seed)
            lag_fx.set_simulated(not frozen)
            if not frozen:
                lag_fx.set_frame(lfr.spawn, lfr.seed)
                lag_orc.step(lfr)
            z.fx.set_frame(zfr.spawn, zfr.seed)
            z_orc.step(zfr)
            ctx.simulate()
            tr.assert_frame(f, g.state(), f"merge={merge}")
            m = lag_fx.metadata()
            lag_state = {"counters": {k: m[k] for k in keys}, "alive": lag_fx.alive_list(), "dead": lag_fx.dead_list(),
                         "attrs": {a.name: lag_fx.read_attr(a.id).view(np.uint32) for a in stored_attrs(tr.asset)}}
            assert_same_state(lag_orc.state(), lag_state, f"merge={merge} frame {f}: the instance that was frozen")
            assert_same_state(z_orc.state(), z.state(), f"merge={merge} frame {f}: the zoo program")
            if f in checks:
                assert g.fx.check()["ok"] == 1 and lag_fx.check()["ok"] == 1, f
        i = S.parse_kernel_info(g.prog.kernel_info())
        print(f"merge={merge} set_module={set_module}: {i}")
        assert (i["merged_frames"] > 0) == bool(merge), g.prog.kernel_info()
        if merge:
            assert i["merged_frames"] >= len(tr.frames) - 2, g.prog.kernel_info()     # the program lives in the merged launches
    finally:
        ctx.close()


# ---- random programs at capacities that fill chunks ------------------------------------------------------------------------------------------------
def _fuzz(seed, profile, run, every=1):
    ctx = S.make_context(S.FUZZ_PROFILES[profile])
    holder = {}

    def mk(a):
        holder["g"] = GpuRunner(a, ctx=ctx)
        return holder["g"]

    try:
        run(seed, mk, capacity=S.fuzz_capacity(seed), frames=S.full_chunk_frames, every=every)
        assert holder["g"].fx.check()["ok"] == 1
    finally:
        ctx.close()


@pytest.mark.parametrize("profile", sorted(S.FUZZ_PROFILES))
@pytest.mark.parametrize("seed", S.FUZZ_FLOAT_SEEDS)
def test_fuzz_with_completely_alive_chunks(seed, profile):
    _fuzz(seed, profile, _run)


@pytest.mark.parametrize("profile", sorted(S.FUZZ_PROFILES))
@pytest.mark.parametrize("seed", S.FUZZ_TYPED_SEEDS)
def test_fuzz_typed_with_completely_alive_chunks(seed, profile):
    _fuzz(seed, profile, _run_typed)
