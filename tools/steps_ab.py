#!/usr/bin/env python3
"""A/B of hnb_simulate_steps against single frames: c2 (effects.firework_trails, burst) at 16,777,216 particles under the library defaults,
or with --asset tangent_drag a stack without a pre-built kernel (update=jit-stream: burst, lifetime uniform(2, 3), TangentAccel + LinearDrag),
whose fused spans run on the steps kernel hiprtc builds for it.

Per mode a fresh context plays the same script: the burst and 5 warm-up frames (not timed), then `--windows` windows of 32 simulated frames at a
small dt (nobody dies: the c2 metric is defined on complete bursts), each window submitted as
    a  32 x hnb_simulate            (only the old entry points: this mode also runs on a checkout that has no hnb_simulate_steps)
    b  16 x hnb_simulate_steps(2)      c  8 x hnb_simulate_steps(4)      d  4 x hnb_simulate_steps(8)
and timed on the host from the first submission to the end of hnb_ctx_synchronize (a window is 32 frames of >= 0.1 ms: the 10 us of the
synchronisation are < 0.5 %). Reported per mode: median, min and max over the windows of ms per simulated frame, and updates per second.
After the timed windows a slab of the effect is compared bit for bit with an oracle effect fed the same frames (the comparison bench.py makes
for burst configurations: a burst gives slot i the PRNG stream of particle slot_base + i, and nothing a particle does depends on another slot).

    python tools/steps_ab.py --modes a,b,c,d --windows 12 --json out.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS = {"a": (32, 1), "b": (16, 2), "c": (8, 4), "d": (4, 8)}
WARM = 5


def frame_seed(f):
    import oracle
    return oracle.pcg_hash(0xC0FFEE + f)


def tangent_drag(cap):
    """Burst on a sphere surface, tangential acceleration around Z and drag: the update of examples/portal.rs on a burst that lives 2 .. 3 s."""
    import bevy_hanabi_amd as bh
    A, w = bh.Attribute, bh.ExprWriter()
    init = [bh.SetPositionSphereModifier(w.lit((0.0, 0.0, 0.0)).expr(), w.lit(4.0).expr(), bh.ShapeDimension.Surface),
            bh.SetAttributeModifier(A.VELOCITY, ((w.rand(bh.VectorType.VEC3F) * w.lit(2.0) - w.lit(1.0)) * w.lit(3.0)).expr()),
            bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr()),
            bh.SetAttributeModifier(A.LIFETIME, w.lit(2.0).uniform(w.lit(3.0)).expr())]
    update = [bh.TangentAccelModifier(w.lit((0.0, 0.0, 0.0)).expr(), w.lit((0.0, 0.0, 1.0)).expr(), w.lit(30.0).expr()), bh.LinearDragModifier(w.lit(2.0).expr())]
    asset = bh.EffectAsset(cap, bh.SpawnerSettings.once(float(cap)), w.finish())
    for m in init:
        asset = asset.init(m)
    for m in update:
        asset = asset.update(m)
    return asset


def make_asset(name, cap):
    from bevy_hanabi_amd import effects
    return {"c2": effects.firework_trails, "tangent_drag": tangent_drag}[name](cap)


def run_mode(mode, cap, windows, check, marker, asset_name="c2"):
    import bevy_hanabi_amd as bh
    total = 1 + WARM + 32 * windows
    dt = min(1 / 60, 0.5 / total)                 # 0.5 s of the 0.8 s the youngest particle lives: every span stays provable to the end
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(make_asset(asset_name, cap))).create_effect()
    f = 0
    for _ in range(1 + WARM):
        ctx.frame_begin(dt, f * dt)
        fx.set_frame(cap if f == 0 else 0, frame_seed(f))
        ctx.simulate()
        f += 1
    ctx.synchronize()
    calls, steps = CALLS[mode]
    ms = []
    for w in range(windows):
        if marker:
            ctx.profile_marker(marker)
        t0 = time.perf_counter()
        for _ in range(calls):
            if steps == 1:
                ctx.frame_begin(dt, f * dt)
                fx.set_frame(0, frame_seed(f))
                ctx.simulate()
            else:
                fx.set_frames_ahead([0] * steps, [frame_seed(f + s) for s in range(steps)])
                ctx.simulate_steps([(dt, (f + s) * dt) for s in range(steps)])
            f += steps
        ctx.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / 32)
    out = {"mode": mode, "calls_per_window": calls, "steps_per_call": steps, "windows": windows, "frames": f, "dt": dt,
           "ms_per_frame_median": statistics.median(ms), "ms_per_frame_min": min(ms), "ms_per_frame_max": max(ms), "ms_per_frame": ms,
           "updates_per_s": cap / (statistics.median(ms) * 1e-3), "kernel": fx._prog.kernel_info().split("\n")[0]}
    if hasattr(ctx, "step_stats"):
        out["step_stats"] = ctx.step_stats()
    if check:
        out["slab"] = slab_check(fx, cap, f, dt, asset_name=asset_name)
    out["device_check"] = fx.check()
    ctx.close()
    return out


def slab_check(fx, cap, frames, dt, slots=16384, asset_name="c2"):
    """Slots [B, B + S) of the effect against an oracle effect of capacity S and slot_base B fed the same frames: every stored plane and the set of
    alive slots, bit for bit (NaN == NaN)."""
    import bevy_hanabi_amd as bh
    import oracle
    S = min(slots, cap)
    B = min(cap // 2 // 4096 * 4096, cap - S)
    asset = make_asset(asset_name, S)
    o = oracle.OracleEffect(bh.serialize_asset(asset), B, omp=True)
    for f in range(frames):
        o.step(dt, S if f == 0 else 0, frame_seed(f), time=f * dt)
    problems = []
    for a in (a for a in asset.particle_layout() if a.id >= 2):
        ref, got = o.read_attr(a.id).view(np.uint32), fx.read_attr(a.id).view(np.uint32)[B:B + S]
        bad = ref != got
        if a.value_type.elem == bh.ScalarType.Float:
            nan = lambda x: (x & 0x7F800000 == 0x7F800000) & (x & 0x007FFFFF != 0)
            bad &= ~(nan(ref) & nan(got))
        if bad.any():
            problems.append(f"{a.name}: {int(bad.sum())} words differ, first at slot {B + int(np.argwhere(bad)[0][0])}")
    alive = fx.alive_list()
    mine = np.sort(alive[(alive >= B) & (alive < B + S)] - B)
    if not np.array_equal(mine, np.sort(o.alive_list())):
        problems.append(f"alive slots of the slab: device {len(mine)}, oracle {o.alive_count()}")
    return {"slots": [B, B + S], "frames": frames, "alive_in_slab": o.alive_count(), "ok": not problems, "problems": problems}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="a,b,c,d")
    ap.add_argument("--asset", default="c2", choices=["c2", "tangent_drag"], help="c2: a pre-built stream kernel; tangent_drag: update=jit-stream")
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=1, help="repeat the whole list of modes (alternation inside one process)")
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--markers", action="store_true", help="bracket every timed window with k_marker (grid = 100 + index of the mode): for counter runs")
    ap.add_argument("--label", default="")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    rows = []
    for r in range(args.rounds):
        for i, m in enumerate(args.modes.split(",")):
            row = run_mode(m, args.capacity, args.windows, not args.no_check, 100 + i if args.markers else 0, args.asset)
            row["round"], row["label"] = r, args.label
            rows.append(row)
            ok = "slab ok" if row.get("slab", {}).get("ok") else ("slab NOT CHECKED" if "slab" not in row else "SLAB DIFFERS " + "; ".join(row["slab"]["problems"]))
            print(f"{args.label} round {r} mode {m}: {row['ms_per_frame_median']:.4f} ms/frame (min {row['ms_per_frame_min']:.4f}, max {row['ms_per_frame_max']:.4f}), "
                  f"{row['updates_per_s'] / 1e9:.1f} G updates/s, {ok}, fault {row['device_check']['fault']}, stats {row.get('step_stats')}", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    bad = [r for r in rows if ("slab" in r and not r["slab"]["ok"]) or r["device_check"]["ok"] != 1]
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
