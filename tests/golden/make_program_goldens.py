"""Generates the two records that hold program validation and the creation-time proofs (csrc/hnb_program.h) to what the library
computed before they moved there:

  python tests/golden/make_program_goldens.py verdicts      -> validator_verdicts.json      (CPU)
  python tests/golden/make_program_goldens.py kernel-info   -> program_kernel_info.json     (needs the GPU)

verdicts: (return code, hnb_last_error text) of hnb_program_validate for the exact mutant corpus of tests/test_validator_fuzz.py (its
_bases(), _mutate, seeds 1 and 2, 6,000 mutants each) and for the unmutated bases: per seed the accepted / rejected counts, a SHA-256
over the "index rc text" lines, and a histogram of the messages with their digits replaced (a mismatch then points at a rule).

kernel-info: what hnb_program_kernel_info says statically about one program of every kind the proofs tell apart, one instance, two
frames; numbers replaced, run-dependent lines dropped (normalise_kernel_info).
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import bevy_hanabi_amd as bh  # noqa: E402
from bevy_hanabi_amd import _hanabi_host as h  # noqa: E402
from bevy_hanabi_amd import effects, runtime  # noqa: E402

VERDICTS_PATH = os.path.join(HERE, "validator_verdicts.json")
KERNEL_INFO_PATH = os.path.join(HERE, "program_kernel_info.json")
SEEDS = (1, 2)
MUTANTS = 6000


# ---- validator verdicts ---------------------------------------------------------------------------------------------------
def verdict(blob):
    """(rc, text) of hnb_program_validate; text is "" for an accepted blob"""
    lib = runtime.load_library()
    rc = lib.hnb_program_validate(blob, len(blob))
    return rc, ("" if rc == 0 else lib.hnb_last_error().decode("utf-8", "replace"))


def corpus(seed, bases):
    """the mutants of test_accepted_mutants_stay_in_bounds(seed), in its order"""
    from test_validator_fuzz import _mutate
    rng = np.random.default_rng(seed)
    return [_mutate(rng, bases[int(rng.integers(len(bases)))]) for _ in range(MUTANTS)]


def summarise(verdicts):
    lines = [f"{i} {rc} {text}" for i, (rc, text) in enumerate(verdicts)]
    hist = {}
    for rc, text in verdicts:
        key = f"{rc} " + re.sub(r"[0-9]+", "#", text)
        hist[key] = hist.get(key, 0) + 1
    return {"accepted": sum(1 for rc, _ in verdicts if rc == 0), "rejected": sum(1 for rc, _ in verdicts if rc != 0),
            "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest(), "messages": hist}


def verdict_record(verdict_of=verdict):
    from test_validator_fuzz import _bases
    bases = _bases()
    out = {"bases": summarise([verdict_of(b) for b in bases])}
    for seed in SEEDS:
        out[f"seed{seed}"] = summarise([verdict_of(m) for m in corpus(seed, bases)])
    return out


# ---- hnb_program_kernel_info ---------------------------------------------------------------------------------------------
A = h.Attribute


def _stream_asset(capacity, render_reads_age):
    w = h.ExprWriter()
    init = [h.SetAttributeModifier(A.POSITION, w.lit((0.0, 0.0, 0.0)).expr()), h.SetAttributeModifier(A.VELOCITY, w.lit((0.0, 1.0, 0.0)).expr()),
            h.SetAttributeModifier(A.AGE, w.lit(0.0).expr()), h.SetAttributeModifier(A.LIFETIME, w.lit(0.8).uniform(w.lit(1.2)).expr())]
    accel = h.AccelModifier(w.lit((-0.0, -16.0, -0.0)).expr())
    asset = h.EffectAsset(capacity, h.SpawnerSettings.once(float(capacity)), w.finish()).with_name("stream")
    for m in init:
        asset = asset.init(m)
    asset = asset.update(accel)
    return asset.render(h.ColorOverLifetimeModifier()) if render_reads_age else asset.render(h.OrientModifier(h.OrientMode.AlongVelocity))


def _generic_asset(capacity):
    """an acceleration that is an expression of the position: the update is no macro-op stream"""
    w = h.ExprWriter()
    init = [h.SetAttributeModifier(A.POSITION, w.lit((1.0, 0.0, 0.0)).expr()), h.SetAttributeModifier(A.VELOCITY, w.lit((0.0, 1.0, 0.0)).expr()),
            h.SetAttributeModifier(A.AGE, w.lit(0.0).expr()), h.SetAttributeModifier(A.LIFETIME, w.lit(3.0).expr())]
    accel = h.AccelModifier(((w.attr(A.POSITION) - w.lit((0.0, 0.0, 0.0))).normalized() * w.lit(-6.0)).expr())
    asset = h.EffectAsset(capacity, h.SpawnerSettings.rate(500.0), w.finish()).with_name("generic")
    for m in init:
        asset = asset.init(m)
    return asset.update(accel).render(h.ColorOverLifetimeModifier())


def _ribbon_random_lifetime(capacity):
    """effects.ribbon with a per-particle LIFETIME: the head stays sorted (provable), the spawns' place in front is not static"""
    w = h.ExprWriter()
    init = [h.SetAttributeModifier(A.POSITION, w.lit((0.0, 0.0, 0.0)).expr()), h.SetAttributeModifier(A.AGE, w.lit(0.0).expr()),
            h.SetAttributeModifier(A.LIFETIME, w.lit(1.0).uniform(w.lit(2.0)).expr()), h.SetAttributeModifier(A.SIZE, w.lit(0.5).expr()),
            h.SetAttributeModifier(A.RIBBON_ID, w.lit(h.Value.u32(0)).expr())]
    asset = (h.EffectAsset(capacity, h.SpawnerSettings.rate(100.0), w.finish()).with_name("ribbon_random_lifetime")
             .with_motion_integration(h.MotionIntegration.None_).with_simulation_space(h.SimulationSpace.Global))
    for m in init:
        asset = asset.init(m)
    return asset.render(h.SizeOverLifetimeModifier())


def kernel_info_cases():
    """name -> (asset, parent case or None): every kind of program the creation-time proofs tell apart"""
    return {
        "firework_streaming_cohort_off_by_auto": (effects.firework_trails(4096), None),   # render reads AGE, 4,096 slots: AUTO keeps the plane
        "age_euler": (effects.instancing(4096), None),
        "generic_update": (_generic_asset(4096), None),
        "one_age_tick_ribbon_front_static": (effects.ribbon(4096, rate=100.0), None),
        "ribbon_not_front_static": (_ribbon_random_lifetime(4096), None),
        "kill_modifier": (effects.force_field(4096), None),
        "event_parent": (effects.firework_rocket(4096), None),
        "event_child": (effects.firework_sparkle_trail(4096), "event_parent"),
        "cohort_on_render_ignores_age": (_stream_asset(4096, False), None),
        "cohort_on_auto_65536": (_stream_asset(65536, True), None),                       # the smallest size AUTO keeps cohorts for
        "cohort_off_by_auto_4096": (_stream_asset(4096, True), None),
    }


def normalise_kernel_info(text):
    keep = []
    for line in text.replace(" (jit cache hit)", "").splitlines():
        if line.startswith("frame parameters (context):") or line.startswith("hnb_simulate waited for the device"):
            continue
        keep.append(re.sub(r"[0-9]+", "#", line))
    return keep


def kernel_info_record():
    cases = kernel_info_cases()
    ctx = bh.Context(0)
    fx = {}
    progs = {}
    for name, (asset, parent) in cases.items():
        progs[name] = ctx.create_program(bh.lower(asset))
        fx[name] = progs[name].create_effect()
        if parent is not None:
            fx[name].set_parent(fx[parent], 0)
    for f in range(2):
        ctx.frame_begin(1 / 60, f / 60)
        for name, (asset, parent) in cases.items():
            fx[name].set_frame(0 if parent is not None or f else 16, 0xC0FFEE + f)
        ctx.simulate()
    ctx.synchronize()
    out = {name: normalise_kernel_info(progs[name].kernel_info()) for name in cases}
    ctx.close()
    return out


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "verdicts":
        data, path = verdict_record(), VERDICTS_PATH
    elif what == "kernel-info":
        data, path = kernel_info_record(), KERNEL_INFO_PATH
    else:
        sys.exit(__doc__)
    if len(sys.argv) > 2:
        path = sys.argv[2]
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
