#!/usr/bin/env python3
"""A/B of the filtered program export (hnb_program_export_filtered, one shared HNB_FILTER_SPHERE) against what a user has without it, sides
alternating window by window in ONE process on ONE device (the method of tools/program_export_sorted_ab.py). Firework particles, all alive, records
{POSITION @0, AGE @12, ID @16} at stride 32. The sphere sits at the origin; its squared radii are taken from the state (the header's own
arithmetic, d = (x*x + y*y) + z*z in binary32, over the records of a plain program export) so that about 100 %, 25 % and 1 % of the rows are kept.
Per fraction F:

    new_F      hnb_program_export_filtered, the whole call
    loop_F     hnb_effect_export_filtered instance by instance into one buffer; the kept count of an instance is read back before the next call,
               because the next segment's first record is not known before - what a user must do today
    torch_F    hnb_program_export, then the same predicate in torch on the exported records (one torch op per operation of the header's formula)
               and records[mask], on the same device (the export's stream is synchronised in front of torch's)
    plain      hnb_program_export alone: what the filtered call replaces at 100 %

Workloads: 512 instances x 4096 slots (three launches), 512 x 65,536 (C4; five launches), and one instance of 16,777,216 against
hnb_effect_export_filtered itself (effect_F) as a sanity row. Every side's output is compared with the new call's and must be identical. Bars,
each against existing code of the same run: at 25 % and 1 % the new call is no slower than the faster of loop and torch by more than the same-run
spread of the windows (max / min - 1 of a side); the one-instance rows are within that spread of the effect form. The 100 % rows and new / plain
are reported as measured.

    python tools/program_export_filtered_ab.py --windows 10 --reps 20 --log profiles/program_export_filtered_ab.log
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FRACTIONS = (1.0, 0.25, 0.01)
ROW_BYTES, KEPT_BYTES = 16, 64          # mark: list 4 + POSITION 12 per alive row; per kept row: list 4 + order 4 written, order 4 + fields 20 read, record 32 written


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
    lines = [f"program_export_filtered_ab: {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
    verdicts = []
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
        rows = n_inst * cap
        bufs = {k: torch.zeros((rows, 8), dtype=torch.int32, device="cuda") for k in ("new", "other", "plain")}
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        cnt1 = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        prog.export(fields, bufs["plain"].data_ptr(), 32, rows, cnt.data_ptr())
        ctx.synchronize()
        total = int(cnt.cpu()[1])
        e = bufs["plain"][:total, 0:3].view(torch.float32)
        d = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        assert d.dtype == torch.float32 and bool(torch.isfinite(d).all())
        radii = {}
        for frac in FRACTIONS:
            k = max(int(round(frac * total)), 1)
            r2 = float(torch.kthvalue(d, k).values)
            radii[frac] = (r2, int((d <= r2).sum()))
        del e, d
        result = {}

        def new_side(r2):
            flt = dict(kind="sphere", sphere=(0.0, 0.0, 0.0, r2))
            return lambda: prog.export_filtered(fields, bufs["new"].data_ptr(), 32, rows, cnt.data_ptr(), filter=flt)

        def loop_side(r2):
            def run():
                base, off = bufs["other"].data_ptr(), 0
                for fx in fxs:
                    fx.export_filtered(fields, base + off * 32, 32, rows - off, cnt1.data_ptr(), kind="sphere", sphere=(0.0, 0.0, 0.0, r2))
                    ctx.synchronize()
                    off += int(cnt1[1].item())                           # the next segment starts behind what this instance kept
                result["loop"] = off
            return run

        def torch_side(r2):
            r2t = torch.tensor(r2, dtype=torch.float32, device="cuda")

            def run():
                prog.export(fields, bufs["plain"].data_ptr(), 32, rows, cnt1.data_ptr())
                ctx.synchronize()
                rec = bufs["plain"][:total]
                p = rec[:, 0:3].view(torch.float32)                      # the centre is the origin: e = p - 0 = p
                dd = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
                result["torch"] = rec[dd <= r2t]
                torch.cuda.synchronize()
            return run

        def effect_side(r2):
            return lambda: fxs[0].export_filtered(fields, bufs["other"].data_ptr(), 32, rows, cnt1.data_ptr(), kind="sphere", sphere=(0.0, 0.0, 0.0, r2))

        sides = {"plain": lambda: prog.export(fields, bufs["plain"].data_ptr(), 32, rows, cnt1.data_ptr())}
        for frac in FRACTIONS:
            r2 = radii[frac][0]
            sides[f"new_{frac:g}"] = new_side(r2)
            if n_inst == 1:
                sides[f"effect_{frac:g}"] = effect_side(r2)
            else:
                sides[f"loop_{frac:g}"] = loop_side(r2)
                sides[f"torch_{frac:g}"] = torch_side(r2)
        ms = windows(sides, ctx.synchronize, args.windows, args.reps)
        med = {k: statistics.median(x) for k, x in ms.items()}
        spread = max(max(x) / min(x) - 1 for x in ms.values())
        launches = 3 if cap <= 4096 else 5
        lines.append(f"workload {n_inst} instances x {cap} slots ({launches} launches): alive {total} of {rows}; same-run spread of the windows (largest max / min - 1 over the sides): {spread * 100:.1f} %")
        lines.append(f"  plain        {med['plain']:.4f} ms (min {min(ms['plain']):.4f}, max {max(ms['plain']):.4f})")
        for frac in FRACTIONS:
            r2, kept = radii[frac]
            nk = f"new_{frac:g}"
            sides[nk](); ctx.synchronize()
            counts = [int(x) for x in cnt.cpu().numpy().view("uint32")]
            same = [counts == [kept, kept]]
            others = [f"effect_{frac:g}"] if n_inst == 1 else [f"loop_{frac:g}", f"torch_{frac:g}"]
            for ok in others:
                sides[ok](); ctx.synchronize()
                if ok.startswith("torch"):
                    same.append(len(result["torch"]) == kept and bool((bufs["new"][:kept] == result["torch"]).all()))
                else:
                    same.append((n_inst == 1 or result["loop"] == kept) and bool((bufs["new"][:kept] == bufs["other"][:kept]).all()))
            moved = total * ROW_BYTES + kept * KEPT_BYTES
            best = min(others, key=lambda k: med[k])
            ratio = med[nk] / med[best]
            lines.append(f"  target {frac * 100:g} %: squared radius {r2:.9g}, kept {kept} = {kept / max(total, 1) * 100:.3f} % of the alive rows; every side's output identical to the new call's: {all(same)}")
            lines.append(f"    {nk:12s} {med[nk]:.4f} ms (min {min(ms[nk]):.4f}, max {max(ms[nk]):.4f}); {ROW_BYTES} B per alive row + {KEPT_BYTES} B per kept row = {moved / 1e6:.0f} MB -> "
                         f"{moved / (med[nk] * 1e-3) / 1e12:.2f} TB/s")
            for ok in others:
                lines.append(f"    {ok:12s} {med[ok]:.4f} ms (min {min(ms[ok]):.4f}, max {max(ms[ok]):.4f}); new / {ok.split('_')[0]} = {med[nk] / med[ok]:.3f}")
            if frac == 1.0:
                lines.append(f"    new / plain = {med[nk] / med['plain']:.3f} (reported, no bar)")
            else:
                met = ratio <= 1 + spread and all(same)
                verdicts.append(met)
                what = "within the spread of the effect form" if n_inst == 1 else "no slower than the faster of loop and torch by more than the spread"
                lines.append(f"    new / {best.split('_')[0]} = {ratio:.3f}; bar ({what}): {'met' if met else 'MISSED'}")
        del bufs, result
        ctx.close()
        torch.cuda.empty_cache()
    lines.append(f"the bars of every workload and fraction: {'met' if all(verdicts) else 'MISSED'}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
