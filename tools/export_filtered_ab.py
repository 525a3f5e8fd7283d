#!/usr/bin/env python3
"""A/B of the filtered export (hnb_effect_export_filtered, HNB_FILTER_SPHERE) on one effect of 16,777,216 firework particles, in the two states of
tools/export_ab.py (burst: identity list, everything alive; churn: 240 frames of the c2_mixed rate spawner, a permuted list). The sphere sits at
the origin; its squared radii are chosen on the host from the state so that about 100 %, 25 % and 1 % of the alive rows are kept (the realised
fractions are printed). Sides that alternate window by window in ONE process on ONE device:

    plain          hnb_effect_export of {POSITION @0, AGE @12, LIFETIME @16} at stride 32: what the filtered export replaces at 100 %
    filtered_F     hnb_effect_export_filtered of the same records with the sphere that keeps fraction F, the whole call
    torch_F        what a user has without it: the plain export, the same predicate in torch on the exported records (one torch op per
                   operation of the header's formula) and records[mask], on the same device (the export's stream is synchronised in front of
                   torch's: two streams)

A window is `--reps` calls between two synchronisations, timed on the host. Reported: median / min / max ms per call, the bytes the design moves
(DESIGN.md "Filtered export": 16 B per alive row and 64 B per kept row) as a fraction of 8 TB/s, filtered / torch per fraction against the
same-run spread of the windows, and filtered / plain at 100 %. Then the one-launch path: an effect of 4096 slots, plain against filtered.

    python tools/export_filtered_ab.py --windows 10 --reps 20 --log profiles/export_filtered_ab.log
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PEAK = 8e12
FRACTIONS = (1.0, 0.25, 0.01)
ROW_BYTES, KEPT_BYTES, PLAIN_BYTES = 16, 64, 56    # mark: list 4 + POSITION 12; kept: list 4 + order 4 written, order 4 + fields 20 read, record 32 written


def windows(sides, sync, n_windows, reps):
    ms = {k: [] for k in sides}
    for fn in sides.values():           # warm-up: module load, scratch allocation, TLBs
        fn()
    sync()
    for _ in range(n_windows):
        for k, fn in sides.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            sync()
            ms[k].append((time.perf_counter() - t0) * 1e3 / reps)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--states", default="burst,churn")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects
    from export_ab import frame_seed, prepare
    A = bh.Attribute
    fields = [(A.POSITION.id, 0), (A.AGE.id, 12), (A.LIFETIME.id, 16)]
    lines = [f"export_filtered_ab: capacity {args.capacity}, {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
    verdicts = []
    for state in [s for s in args.states.split(",") if s]:
        ctx, fx = prepare(state, args.capacity)
        alive = fx.alive_count()
        cap = args.capacity
        # squared radii from the state, with the header's own arithmetic: d = (x*x + y*y) + z*z in binary32
        p = fx.read_attr(A.POSITION.id).reshape(-1, 3)[fx.alive_list()]
        d = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
        assert d.dtype == np.float32 and np.isfinite(d).all()
        radii = {}
        for frac in FRACTIONS:
            k = max(int(round(frac * alive)), 1) - 1
            r2 = float(np.partition(d, k)[k])
            radii[frac] = (r2, int((d <= np.float32(r2)).sum()))
        del p, d
        dst = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
        dst2 = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        result = {}

        def torch_side(r2):
            r2t = torch.tensor(r2, dtype=torch.float32, device="cuda")

            def run():
                fx.export(fields, dst.data_ptr(), 32, cap, cnt.data_ptr())
                ctx.synchronize()
                rec = dst[:alive]
                e = rec[:, 0:3].view(torch.float32)                      # the centre is the origin: e = p - 0 = p
                dd = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                result["torch"] = rec[dd <= r2t]
                torch.cuda.synchronize()
            return run

        def filtered_side(r2):
            return lambda: fx.export_filtered(fields, dst2.data_ptr(), 32, cap, cnt.data_ptr(), kind="sphere", sphere=(0.0, 0.0, 0.0, r2))

        sides = {"plain": lambda: fx.export(fields, dst.data_ptr(), 32, cap, cnt.data_ptr())}
        for frac in FRACTIONS:
            sides[f"filtered_{frac:g}"] = filtered_side(radii[frac][0])
            sides[f"torch_{frac:g}"] = torch_side(radii[frac][0])
        ms = windows(sides, ctx.synchronize, args.windows, args.reps)
        med = {k: statistics.median(x) for k, x in ms.items()}
        spread = max(max(x) / min(x) - 1 for x in ms.values())
        lines.append(f"state {state}: alive {alive} of {cap}; same-box spread of the windows (largest max / min - 1 over the sides): {spread * 100:.1f} %")
        lines.append(f"  plain          {med['plain']:.4f} ms (min {min(ms['plain']):.4f}, max {max(ms['plain']):.4f}); {PLAIN_BYTES} B per row = {alive * PLAIN_BYTES / 1e6:.0f} MB -> "
                     f"{alive * PLAIN_BYTES / (med['plain'] * 1e-3) / 1e12:.2f} TB/s = {alive * PLAIN_BYTES / (med['plain'] * 1e-3) / PEAK:.2f} of 8 TB/s")
        for frac in FRACTIONS:
            r2, kept = radii[frac]
            fk, tk = f"filtered_{frac:g}", f"torch_{frac:g}"
            sides[tk](); sides[fk](); ctx.synchronize()                      # (the filtered export last: the count words are its own)
            counts = [int(x) for x in cnt.cpu().numpy().view(np.uint32)]
            same = counts == [kept, kept] and len(result["torch"]) == kept and bool((dst2[:kept] == result["torch"]).all())
            moved = alive * ROW_BYTES + kept * KEPT_BYTES
            ratio = med[fk] / med[tk]
            ok = ratio <= 1 + spread
            verdicts.append(ok)
            lines.append(f"  target {frac * 100:g} %: squared radius {r2:.9g}, kept {kept} = {kept / max(alive, 1) * 100:.3f} % of the alive rows; filtered and torch outputs identical: {same}")
            lines.append(f"    {fk:14s} {med[fk]:.4f} ms (min {min(ms[fk]):.4f}, max {max(ms[fk]):.4f}); {ROW_BYTES} B per alive row + {KEPT_BYTES} B per kept row = {moved / 1e6:.0f} MB -> "
                         f"{moved / (med[fk] * 1e-3) / 1e12:.2f} TB/s = {moved / (med[fk] * 1e-3) / PEAK:.2f} of 8 TB/s")
            lines.append(f"    {tk:14s} {med[tk]:.4f} ms (min {min(ms[tk]):.4f}, max {max(ms[tk]):.4f})")
            lines.append(f"    filtered / torch = {ratio:.3f}; filtered / plain = {med[fk] / med['plain']:.3f}; bar (filtered <= torch within the spread): {'met' if ok else 'MISSED'}")
        del dst, dst2
        ctx.close()
    # the one-launch path: 4096 slots, everything alive, the sphere that keeps about a quarter
    small = 4096
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(small))).create_effect()
    for f in range(6):
        ctx.frame_begin(1 / 600, f / 600)
        fx.set_frame(small if f == 0 else 0, frame_seed(f))
        ctx.simulate()
    p = fx.read_attr(A.POSITION.id).reshape(-1, 3)[fx.alive_list()]
    d = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    r2 = float(np.partition(d, small // 4)[small // 4])
    dst = torch.zeros((small, 8), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sides = {"plain": lambda: fx.export(fields, dst.data_ptr(), 32, small, cnt.data_ptr()),
             "filtered": lambda: fx.export_filtered(fields, dst.data_ptr(), 32, small, cnt.data_ptr(), kind="sphere", sphere=(0.0, 0.0, 0.0, r2))}
    ms = windows(sides, ctx.synchronize, args.windows, 10 * args.reps)
    lines.append(f"one-launch path: {small} slots, all alive, {int((d <= np.float32(r2)).sum())} kept, {10 * args.reps} calls per window")
    for k in sides:
        lines.append(f"  {k:8s} {statistics.median(ms[k]) * 1e3:.2f} us per call (min {min(ms[k]) * 1e3:.2f}, max {max(ms[k]) * 1e3:.2f})")
    ctx.close()
    lines.append(f"the bar at every fraction and state: {'met' if all(verdicts) else 'MISSED'}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
