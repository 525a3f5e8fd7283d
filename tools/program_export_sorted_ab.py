#!/usr/bin/env python3
"""A/B of the sorted program export (hnb_program_export_sorted, key DEPTH) against what a user has without it, sides alternating window by window
in ONE process on ONE device (the method of tools/export_sorted_ab.py). Per workload, all particles alive, records {POSITION @0, AGE @12, ID @16}
at stride 32:

    inst       hnb_program_export_sorted, HNB_SORT_SCOPE_INSTANCE, the whole call
    loop       its baseline: hnb_effect_export_sorted instance by instance into the segments of one buffer (offsets known to the host here)
    prog       hnb_program_export_sorted, HNB_SORT_SCOPE_PROGRAM, the whole call
    torch      its baseline: hnb_program_export, then keys from the records, torch.sort(keys, stable=True) and index_select of the records, on the
               same device (the export's stream is synchronised in front of torch's)

Workloads: 512 instances x 4096 slots (the one-launch path), 512 x 65,536 (C4; the multi-tile path), one instance of 16,777,216 (C2's size, a
sanity row against the effect form). The two ends' buffers are compared for identity. Reported: median / min / max ms per call, the window spread,
and the bytes the design moves per row (DESIGN.md "Sorted export, program form") as TB/s.

    python tools/program_export_sorted_ab.py --windows 10 --reps 20 --log profiles/program_export_sorted_ab.log
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
DIR = (0.3, -0.5, 0.8)
# per alive row. inst, multi-tile: the effect form's 156 (keys 16 + 8, four passes of 8 + 8 and three recounts of 4, gather 4 + 20 + 32);
# inst, one launch: keys 16 + 8, four passes of (4 + 8 + 8) inside one workgroup, gather 4 + 20 + 32; prog: fill 16 + 8, four passes of 4 + 8 + 8, gather 4 + 20 + 32
BYTES = {"inst": {True: 160, False: 156}, "prog": {True: 160, False: 160}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="512x4096,512x65536,1x16777216")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects
    from export_ab import frame_seed
    from export_sorted_ab import windows
    A = bh.Attribute
    fields = [(A.POSITION.id, 0), (A.AGE.id, 12), (A.ID.id, 16)]
    lines = [f"program_export_sorted_ab: {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
    for w in [x for x in args.workloads.split(",") if x]:
        n_inst, cap = (int(x) for x in w.split("x"))
        ctx = bh.Context(0)
        prog = ctx.create_program(bh.lower(effects.firework_trails(cap)))
        fxs = [prog.create_effect(slot_base=k * cap) for k in range(n_inst)]
        for f in range(6):
            ctx.frame_begin(1 / 600, f / 600)
            for k, fx in enumerate(fxs):
                fx.set_frame(cap if f == 0 else 0, frame_seed(f * 7 + k))
            ctx.simulate()
        ctx.synchronize()
        counts = [fx.alive_count() for fx in fxs]
        total = sum(counts)
        offs = [0]
        for c in counts:
            offs.append(offs[-1] + c)
        rows = n_inst * cap
        bufs = {k: torch.zeros((rows, 8), dtype=torch.int32, device="cuda") for k in ("inst", "loop", "prog", "plain")}
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        v = torch.tensor(DIR, dtype=torch.float32, device="cuda")
        result = {}

        def loop_side():
            base = bufs["loop"].data_ptr()
            for k, fx in enumerate(fxs):
                fx.export_sorted(fields, base + offs[k] * 32, 32, counts[k], None, key="depth", v=DIR)

        def torch_side():
            prog.export(fields, bufs["plain"].data_ptr(), 32, rows, cnt.data_ptr())
            ctx.synchronize()
            rec = bufs["plain"][:total]
            p = rec[:, 0:3].view(torch.float32)
            d = (p[:, 0] * v[0] + p[:, 1] * v[1]) + p[:, 2] * v[2]
            order = torch.sort(d, stable=True).indices
            result["torch"] = rec.index_select(0, order)
            torch.cuda.synchronize()

        sides = {"inst": lambda: prog.export_sorted(fields, bufs["inst"].data_ptr(), 32, rows, cnt.data_ptr(), scope="instance", key="depth", v=DIR),
                 "loop": loop_side,
                 "prog": lambda: prog.export_sorted(fields, bufs["prog"].data_ptr(), 32, rows, cnt.data_ptr(), scope="program", key="depth", v=DIR),
                 "torch": torch_side}
        ms = windows(sides, ctx.synchronize, args.windows, args.reps)
        lines.append(f"workload {n_inst} instances x {cap} slots: alive {total} of {rows}")
        for k in ("inst", "loop", "prog"):
            sides[k]()
        ctx.synchronize(); torch_side()
        lines.append(f"  inst and loop outputs identical: {bool((bufs['inst'][:total] == bufs['loop'][:total]).all())}")
        lines.append(f"  prog and torch outputs identical: {bool((bufs['prog'][:total] == result['torch']).all())}")
        med = {k: statistics.median(x) for k, x in ms.items()}
        spread = {k: max(x) / min(x) - 1 for k, x in ms.items()}
        for k in sides:
            per = BYTES.get(k, {}).get(cap <= 4096)
            bw = f"; {per} B per row = {total * per / 1e6:.0f} MB -> {total * per / (med[k] * 1e-3) / 1e12:.3f} TB/s" if per else ""
            lines.append(f"  {k:6s} {med[k]:.4f} ms (min {min(ms[k]):.4f}, max {max(ms[k]):.4f}, spread {spread[k] * 100:.1f} %){bw}")
        lines.append(f"  inst / loop = {med['inst'] / med['loop']:.3f}; prog / torch = {med['prog'] / med['torch']:.3f} (largest window spread of the four sides: {max(spread.values()) * 100:.1f} %)")
        del bufs, result
        ctx.close()
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
