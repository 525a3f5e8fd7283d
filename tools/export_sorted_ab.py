#!/usr/bin/env python3
"""A/B of the sorted export (hnb_effect_export_sorted, key DEPTH) on one effect of 16,777,216 firework particles, in the two states of
tools/export_ab.py (burst: identity list, everything alive; churn: 240 frames of the c2_mixed rate spawner, a permuted list), three sides that
alternate window by window in ONE process on ONE device:

    plain    hnb_effect_export of {POSITION @0, AGE @12, LIFETIME @16} at stride 32: the floor - the sorted export ends in the same gather
    sorted   hnb_effect_export_sorted of the same records, depth along (0.3, -0.5, 0.8), the whole call
    torch    what a user has without it: the plain export, then keys from the records, torch.sort(keys, stable=True) and index_select of the
             32-byte records, all in torch on the same device (the export's stream is synchronised in front of torch's: two streams)

and `sortonly`, the sorted export into a destination of 0 records: every gather workgroup leaves after its scalar loads, so the call is the key
and sort stages alone and sorted - sortonly is the gather behind a sort. A window is `--reps` calls between two synchronisations, timed on the
host. Reported: median / min / max ms per call, and the bytes the design moves per alive row (DESIGN.md "Sorted export") as a fraction of 8 TB/s.
Then the one-launch path: an effect of 4096 slots, plain against sorted.

    python tools/export_sorted_ab.py --windows 10 --reps 20 --log profiles/export_sorted_ab.log
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
DIR = (0.3, -0.5, 0.8)
BYTES = {"plain": 56, "sorted": 156, "sortonly": 100}    # per alive row: keys 16 + 8, four passes of 8 + 8 and three recounts of 4, gather 4 + 20 + 32


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
    ap.add_argument("--only", default="", help="comma-separated sides to run (plain, sorted, sortonly, torch)")
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects
    from export_ab import frame_seed, prepare
    A = bh.Attribute
    fields = [(A.POSITION.id, 0), (A.AGE.id, 12), (A.LIFETIME.id, 16)]
    lines = [f"export_sorted_ab: capacity {args.capacity}, {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
    for state in [s for s in args.states.split(",") if s]:
        ctx, fx = prepare(state, args.capacity)
        alive = fx.alive_count()
        cap = args.capacity
        dst = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
        dst2 = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        v = torch.tensor(DIR, dtype=torch.float32, device="cuda")
        result = {}

        def torch_side():
            fx.export(fields, dst.data_ptr(), 32, cap, cnt.data_ptr())
            ctx.synchronize()
            rec = dst[:alive]
            p = rec[:, 0:3].view(torch.float32)
            d = (p[:, 0] * v[0] + p[:, 1] * v[1]) + p[:, 2] * v[2]
            order = torch.sort(d, stable=True).indices
            result["torch"] = rec.index_select(0, order)
            torch.cuda.synchronize()

        sides = {"plain": lambda: fx.export(fields, dst.data_ptr(), 32, cap, cnt.data_ptr()),
                 "sorted": lambda: fx.export_sorted(fields, dst2.data_ptr(), 32, cap, cnt.data_ptr(), key="depth", v=DIR),
                 "sortonly": lambda: fx.export_sorted(fields, dst2.data_ptr(), 32, 0, None, key="depth", v=DIR),
                 "torch": torch_side}
        if args.only:
            sides = {k: sides[k] for k in args.only.split(",")}
        ms = windows(sides, ctx.synchronize, args.windows, args.reps)
        lines.append(f"state {state}: alive {alive} of {cap}")
        if "sorted" in sides and "torch" in sides:       # the two ends are the same records (no NaN keys here: torch's order of floats is the key order, except -0 == +0)
            sides["sorted"](); ctx.synchronize(); torch_side()
            same = bool((dst2[:alive] == result["torch"]).all())
            lines.append(f"  sorted and torch outputs identical: {same}")
        for k in sides:
            med = statistics.median(ms[k])
            per = BYTES.get(k)
            bw = f"; {per} B per row = {alive * per / 1e6:.0f} MB -> {alive * per / (med * 1e-3) / 1e12:.2f} TB/s = {alive * per / (med * 1e-3) / PEAK:.2f} of 8 TB/s" if per else ""
            lines.append(f"  {k:8s} {med:.4f} ms (min {min(ms[k]):.4f}, max {max(ms[k]):.4f}){bw}")
        med = {k: statistics.median(x) for k, x in ms.items()}
        spread = max(max(x) / min(x) - 1 for x in ms.values())
        if "sorted" in med and "sortonly" in med:
            lines.append(f"  gather behind the sort (sorted - sortonly) = {med['sorted'] - med['sortonly']:.4f} ms")
        if "sorted" in med and "torch" in med:
            lines.append(f"  sorted / torch = {med['sorted'] / med['torch']:.3f}, sorted / plain = {med['sorted'] / med['plain']:.2f} (same-box spread of the windows: {spread * 100:.1f} %)"
                         if "plain" in med else f"  sorted / torch = {med['sorted'] / med['torch']:.3f}")
        del dst, dst2
        ctx.close()
    # the one-launch path: 4096 slots, everything alive
    if not args.only:
        small = 4096
        ctx = bh.Context(0)
        fx = ctx.create_program(bh.lower(effects.firework_trails(small))).create_effect()
        for f in range(6):
            ctx.frame_begin(1 / 600, f / 600)
            fx.set_frame(small if f == 0 else 0, frame_seed(f))
            ctx.simulate()
        dst = torch.zeros((small, 8), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        sides = {"plain": lambda: fx.export(fields, dst.data_ptr(), 32, small, cnt.data_ptr()),
                 "sorted": lambda: fx.export_sorted(fields, dst.data_ptr(), 32, small, cnt.data_ptr(), key="depth", v=DIR)}
        ms = windows(sides, ctx.synchronize, args.windows, 10 * args.reps)
        lines.append(f"one-launch path: {small} slots, all alive, {10 * args.reps} calls per window")
        for k in sides:
            lines.append(f"  {k:8s} {statistics.median(ms[k]) * 1e3:.2f} us per call (min {min(ms[k]) * 1e3:.2f}, max {max(ms[k]) * 1e3:.2f})")
        ctx.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
