"""tests/option_scripts.py without a GPU: every option classified, every script's preconditions asserted on the oracle alone (the chunk states the
GPU tests of tests/test_gpu_option_matrix.py are meant to go through), the fuzz seeds' share of completely alive chunks, the kernel_info parser."""
import ast
import os

import numpy as np
import pytest

import bevy_hanabi_amd as bh
import option_scripts as S
from bevy_hanabi_amd import runtime
from fuzz_assets import random_asset, random_typed_asset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- classification ------------------------------------------------------------------------------------------------------------------------
def test_every_option_has_exactly_one_class():
    unclassified = sorted(set(runtime.OPTIONS) - set(S.CLASSES))
    assert not unclassified, f"classify {unclassified} in tests/option_scripts.py: creation, frame or excluded (with a reason)"
    assert not set(S.CLASSES) - set(runtime.OPTIONS), "option_scripts.CLASSES names options the runtime does not have"
    assert all(v[0] in ("creation", "frame", "excluded") for v in S.CLASSES.values())
    assert set(S.CREATION) == {"age_cohort", "cull_lifetime", "horizon"}
    assert set(S.FRAME) == {"alternate", "skip_lists", "transpose", "scene_merge", "suffix_proof", "ring_lists", "slot_init", "overlap_updates", "stream_hints",
                            "direct_upload", "fuse_steps"}
    assert set(S.EXCLUDED) == {"test_break_proof", "jit_async", "set_module", "list_order"}
    assert all(isinstance(r, str) and len(r) > 20 for r in S.EXCLUDED.values())
    assert len(S.CREATION) + len(S.FRAME) + len(S.EXCLUDED) == len(runtime.OPTIONS)
    assert S.values_of("age_cohort") == (3, 0, 1, 2) and set(S.values_of("slot_init")) == {0, 1, 2}
    assert "256 MiB" in S.__doc__ and "use_streaming_hints" in S.__doc__ and "do not claim to cover" in S.__doc__


def test_plain_restates_the_bench_dictionary():
    """bench.py is not imported (it initialises the device plumbing): its PLAIN_OPTIONS literal is read from the source"""
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    lit = next(n.value for n in tree.body if isinstance(n, ast.Assign) and any(getattr(t, "id", None) == "PLAIN_OPTIONS" for t in n.targets))
    assert ast.literal_eval(lit) == S.PLAIN
    assert set(S.PLAIN) <= set(S.CREATION + S.FRAME) and all(v == 0 for v in S.PLAIN.values())


def test_single_flips_cover_every_value_from_both_bases():
    for base in ({}, S.PLAIN):
        flips = S.single_flips(base)
        assert len(set(flips)) == len(flips)
        for k in S.CREATION + S.FRAME:
            assert {v for o, v in flips if o == k} == set(S.values_of(k)) - {S.base_value(base, k)}
    assert ("slot_init", 0) in S.single_flips({}) and ("slot_init", 2) in S.single_flips({}) and ("slot_init", 1) in S.single_flips(S.PLAIN)
    assert {v for o, v in S.single_flips({}) if o == "age_cohort"} == {0, 1, 2} and {v for o, v in S.single_flips(S.PLAIN) if o == "age_cohort"} == {1, 2, 3}


# ---- the firework life cycle ---------------------------------------------------------------------------------------------------------------
def test_firework_life_cycle_at_three_chunks_and_a_ragged_one():
    """The chunk states of the script, frame by frame, from the oracle's alive list and AGE plane."""
    cap = S.FIREWORK_CAP
    tr = S.trace("firework", cap)
    n = tr.n_chunks()
    assert n == 4 and len(tr.frames) == S.FIREWORK_TIGHT + 3
    chunks = range(n)
    for f in range(0, 48):                                                                  # flight: all 4 chunks completely alive, one age each
        assert all(tr.full(f, j) and tr.uniform(f, j) for j in chunks), f
    assert all(tr.kernel_full(47, j) for j in range(3)) and not tr.kernel_full(47, 3)
    assert all(tr.full(47, j) and not tr.full(48, j) for j in chunks)                       # full -> not full: the first deaths, frame 48
    assert all(tr.uniform(69, j) and tr.mixed(70, j) for j in chunks)                       # uniform -> mixed: the 900 spawns land in every chunk
    for f in range(71, 104):                                                                # mixed -> uniform, held for 33 frames: two re-check periods of 16
        assert all(tr.uniform(f, j) and not tr.full(f, j) for j in chunks), f
    assert tr.frames[90].dt == 1 / 24 and tr.frames[91].dt == 0.0                          # (... one with another tick, one with none)
    assert all(tr.full(104, j) and tr.mixed(104, j) for j in chunks)                        # completely alive AND mixed: the re-burst beside the 900
    assert all(tr.full(116, j) for j in chunks) and not all(tr.full(117, j) for j in chunks)   # the 900 older particles die from frame 117 on
    assert tr.alive_counts[S.FIREWORK_EMPTY_BY] == 0 and tr.alive_counts[124] > 0           # all dead
    assert all(tr.facts[S.FIREWORK_EMPTY_BY][j][1] == 0 and tr.full(S.FIREWORK_EMPTY_BY + 1, j) and tr.uniform(S.FIREWORK_EMPTY_BY + 1, j) for j in chunks)   # empty -> full, uniform
    assert all(tr.alive_counts[f] == cap for f in range(S.FIREWORK_EMPTY_BY + 1, S.FIREWORK_TIGHT)) and S.FIREWORK_TIGHT - (S.FIREWORK_EMPTY_BY + 1) > 20   # 20 more frames of flight, and on
    # the tight frame: the first deaths of that burst come within 2^-9 (relative) of the smallest lifetime - a death horizon that is late by more is wrong here
    st = tr.oracle_state(S.FIREWORK_TIGHT)
    age, life = (st["attrs"][k].view(np.float32).reshape(-1) for k in ("age", "lifetime"))
    assert 0 < cap - tr.alive_counts[S.FIREWORK_TIGHT] < 100 and len(np.unique(age[st["alive"]])) == 1
    assert 0 < (age[st["alive"]][0] - life.min()) / life.min() < 2.0 ** -9
    t = tr.transitions()
    assert (t["full_to_not_full"], t["uniform_to_mixed"], t["mixed_to_uniform"], t["full_and_mixed"], t["empty_to_full"]) == (48, 70, 71, 104, S.FIREWORK_EMPTY_BY + 1)
    assert t["refilled_to_not_full"] == S.FIREWORK_TIGHT
    assert t["all_dead"] is not None and 124 < t["all_dead"] <= S.FIREWORK_EMPTY_BY and t["uniform_run"] >= 33
    assert set(tr.transition_frames()) >= {0, 48, 70, 71, 104, t["all_dead"], S.FIREWORK_EMPTY_BY + 1, S.FIREWORK_TIGHT, len(tr.frames) - 1}
    assert tr.flight_frame() < 47


@pytest.mark.parametrize("cap", [4095, 4096, 4097])
def test_firework_life_cycle_around_one_chunk(cap):
    tr = S.trace("firework", cap)
    t = tr.transitions()
    assert tr.frames[70].spawn == cap // 14 and tr.n_chunks() == (1 if cap <= 4096 else 2)
    assert t["full_to_not_full"] is not None and t["uniform_to_mixed"] == 70 and t["mixed_to_uniform"] is not None
    assert t["uniform_run"] >= 17, t                                # mixed -> uniform, held over a whole re-check period
    assert t["full_and_mixed"] == 104 and t["all_dead"] is not None and t["all_dead"] <= S.FIREWORK_EMPTY_BY
    assert t["empty_to_full"] is not None and tr.alive_counts[S.FIREWORK_EMPTY_BY + 21] == cap and 0 < tr.alive_counts[S.FIREWORK_TIGHT] < cap
    assert tr.full(S.FIREWORK_EMPTY_BY + 1, 0) and tr.uniform(S.FIREWORK_EMPTY_BY + 1, 0) and tr.facts[S.FIREWORK_EMPTY_BY][0][1] == 0
    assert any(tr.kernel_full(f, 0) for f in range(len(tr.frames))) == (cap >= 4096)     # 4095: the one size at which cfull is never set


# ---- the three other assets ----------------------------------------------------------------------------------------------------------------
def test_force_field_script_kills_by_modifier_and_fills_and_empties():
    tr = S.trace("force_field", S.FORCE_FIELD_CAP)
    t = tr.transitions()
    assert tr.kill_deaths > 100, "no particle died of a kill modifier (age < lifetime)"
    assert tr.n_chunks() == 2 and tr.kernel_full(30, 0)
    assert t["full_to_not_full"] is not None and t["uniform_to_mixed"] == 70 and t["mixed_to_uniform"] is not None
    assert t["all_dead"] is not None and t["empty_to_full"] is not None and tr.alive_counts[-1] == S.FORCE_FIELD_CAP
    blob = bh.lower(tr.asset)
    bh.validate_program(blob)
    # what the transpose flips on this asset rely on: the update runs on the streaming kernel, and not on its flat path (component-wise ops only)
    from helpers import CpuVmRunner, program_mnemonics
    assert CpuVmRunner(tr.asset).streamable
    assert set(program_mnemonics(blob)["update"]) - {"M_AGE_TICK", "M_VEL_SCALE", "M_VEL_ADD", "M_EULER"} >= {"M_CONFORM_SPHERE", "M_KILL_AABB", "M_KILL_SPHERE"}
    assert set(program_mnemonics(bh.lower(S.trace("firework", 4096).asset))["update"]) == {"M_AGE_TICK", "M_VEL_SCALE", "M_VEL_ADD", "M_EULER"}   # (the flat one)


def test_ribbon_script_churns_dies_out_and_restarts():
    tr = S.trace("ribbon", S.RIBBON_CAP)
    t = tr.transitions()
    assert max(tr.alive_counts) > S.RIBBON_CAP * 0.95                         # the rate spawner fills the trail ...
    churn = [f for f in range(1, 110) if tr.frames[f].spawn > 0 and tr.alive_counts[f] < tr.alive_counts[f - 1] + tr.frames[f].spawn]
    assert len(churn) >= 15, churn                                           # ... and then rows die in frames that also spawn
    assert t["full_and_mixed"] is not None and t["all_dead"] is not None and tr.alive_counts[-1] > 1000
    assert all(fr.spawn == 0 for fr in tr.frames[110:205]) and tr.frames[206].spawn > 0


@pytest.mark.parametrize("cap", [S.AUTO_THRESHOLD - 1, S.AUTO_THRESHOLD])
def test_age_reading_asset_on_both_sides_of_the_auto_threshold(cap):
    tr = S.trace("firework_short", cap)
    hdr = np.frombuffer(bh.lower(tr.asset)[:96], dtype=np.uint32)   # HnbProgramHeader: the last two words are render_reads_lo / _hi
    assert (int(hdr[-2]) | int(hdr[-1]) << 32) >> S.A.AGE.id & 1, "the asset's render modifiers do not read AGE"
    t = tr.transitions()
    assert t["full_to_not_full"] == 48 and t["uniform_to_mixed"] == 60 and t["mixed_to_uniform"] is not None and t["full_and_mixed"] == 80
    assert all(tr.kernel_full(20, j) for j in range(cap // S.CHUNK))


def test_fuse_script_has_quiet_spans_at_seventeen_chunks():
    """tests/test_gpu_option_matrix.py steps this script in calls of four frames: more than 16 chunks (a fused launch is never a small program's), and
    whole calls in which nothing spawns and nothing dies, before the first deaths and between the respawn and the re-burst"""
    tr = S.trace("firework_short", S.FUSE_CAP)
    assert tr.n_chunks() == 17
    quiet = [f for f in range(0, len(tr.frames), 4) if f and all(fr.spawn == 0 for fr in tr.frames[f:f + 4]) and len(set(tr.alive_counts[f - 1:f + 4])) == 1]
    assert len(quiet) >= 8 and tr.transitions()["full_to_not_full"] == 48, quiet


# ---- fuzz seeds ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make, seeds", [(random_asset, S.FUZZ_FLOAT_SEEDS), (random_typed_asset, S.FUZZ_TYPED_SEEDS)], ids=["float", "typed"])
def test_at_least_half_of_the_fuzz_seeds_hold_a_completely_alive_chunk(make, seeds):
    assert len(seeds) == 8 and {S.fuzz_capacity(s) for s in seeds} == set(S.FUZZ_CAPS) == {4096, 4097, 2 * 4096 + 5}
    full = 0
    for seed in seeds:
        cap = S.fuzz_capacity(seed)
        asset = make(seed, cap)
        bh.validate_program(bh.lower(asset))          # every committed seed lowers: none of the GPU ids is a skip
        frames = S.full_chunk_frames(seed, cap)
        assert frames[0].spawn == cap and frames[len(frames) // 2].spawn == 2 * cap + 1
        full += S.holds_a_full_chunk(asset, frames)
    assert 2 * full >= len(seeds), full


def test_fuzz_frames_follow_random_frames_elsewhere():
    from fuzz_assets import random_frames
    a, b = S.full_chunk_frames(7, 4097), random_frames(7, 4097)
    for f, (x, y) in enumerate(zip(a, b)):
        assert (x.dt, x.seed, x.time) == (y.dt, y.seed, y.time) and (x.transform == y.transform).all()
        assert x.spawn == y.spawn or f in (0, 18)


# ---- kernel_info -----------------------------------------------------------------------------------------------------------------------------
SAMPLE = """init=jit update=jit-stream
steps kernel: not requested
age cohorts: 3 of 4 chunks (HNB_AGE_COHORT_AUTO: the asset's render modifiers read AGE, the update keeps the plane current)
slot-major init (large spawns): 3 frames
casualties proven to be the list's last rows (no k_count_rows): 61 frames
list kept as a ring (no row rewritten): 58 frames
ribbon sorts skipped in list-free frames: 7 frames
ribbon sorts by rotation: 180 of 230 frames
ribbon sorts by path: one-tile 1, one-workgroup 2, multi-launch 3 frames
update served by a merged launch (small programs of the context share one): 150 frames
... by the context's set module (the program's specialised code behind the shared launch): 140 frames
death horizons in use: 44 frames
lists skipped: 47 of 202 frames
frame parameters (context): written by the host into device memory in 202 frames, copied in 0
hnb_simulate waited for the device (the frame 5 before still running) in 0 of 202 frames, 0 us in all"""


def test_kernel_info_parser_reads_the_sample():
    i = S.parse_kernel_info(SAMPLE)
    assert (i["lists_skipped"], i["frames_run"], i["lists_eligible"]) == (47, 202, True)
    assert i["horizon_frames"] == 44 and (i["cohort_chunks"], i["cohort_total"], i["cohort_plane_current"]) == (3, 4, True)
    assert i["slot_init_frames"] == 3 and i["merged_frames"] == 150 and i["set_module_frames"] == 140
    assert (i["suffix_frames"], i["ring_frames"], i["sort_skipped_frames"], i["sort_rotated_frames"]) == (61, 58, 7, 180)
    assert not i["cohort_auto_off"] and (i["direct_frames"], i["copied_frames"], i["large_bar"]) == (202, 0, True)
    k = S.parse_kernel_info("lists skipped: 0 of 9 frames\nframe parameters (context): written by the host into device memory in 0 frames, copied in 9 (the device memory is not host-visible: no large BAR)")
    assert (k["direct_frames"], k["copied_frames"], k["large_bar"]) == (0, 9, False)
    j = S.parse_kernel_info("init=jit update=jit-stream\nage cohorts: off (HNB_AGE_COHORT_AUTO: the asset's render modifiers read AGE after every frame)\n"
                            "lists skipped: 0 of 12 frames (not eligible)")
    assert j["cohort_auto_off"] and j["cohort_chunks"] == 0 and j["lists_skipped"] == 0 and j["frames_run"] == 12 and not j["lists_eligible"]
    assert all(j[k] == 0 for k in ("horizon_frames", "slot_init_frames", "merged_frames", "suffix_frames", "ring_frames", "sort_skipped_frames"))
