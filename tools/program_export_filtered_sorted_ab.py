#!/usr/bin/env python3
"""A/B of the filtered, then sorted program export (an HnbExportSortFiltered through hnb_program_export_sorted, instance scope; one shared
HNB_FILTER_SPHERE, HNB_SORT_KEY_DEPTH) against what a user has without it, sides alternating window by window in ONE process on ONE device (the
method of tools/bounds_ab.py). Firework particles, all alive, records {POSITION @0, COLOR @12} at stride 16. The sphere sits at the origin; its
squared radii are taken from the state (the header's own arithmetic, d = (x*x + y*y) + z*z in binary32, over the records of a plain program
export) so that about 100 %, 25 % and 1 % of the rows are kept. Per fraction F:

    new_F      the new call, whole
    loop_F     hnb_effect_export_filtered_sorted instance by instance into one buffer; the kept count of an instance is read back before the next
               call, because the next segment's first record is not known before - the host loop a user writes today
    sorted     hnb_program_export_sorted (instance scope) of ALL rows, which does not depend on F: what a user sorts today, before the consumer
               discards what is outside the sphere (the discarding is not timed)

Workloads: 512 instances x 4096 slots (3 launches), 512 x 65,536 (13 launches and a memset), and one instance of 16,777,216 against
hnb_effect_export_filtered_sorted itself (effect_F), reported and not barred. Every side's output is compared with the new call's: the loop's
buffer is identical, and the sorted side's records with the predicate applied in torch, in their order, are the new call's. The bar, against the
alternatives of the same run and never against the code under test: in every 512-instance row the new call is no slower than the faster of loop
and sorted by more than the same-run spread of the windows (largest max / min - 1 over the sides).

    python tools/program_export_filtered_sorted_ab.py --windows 10 --reps 20 --log profiles/program_export_filtered_sorted_ab.log
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FRACTIONS = (1.0, 0.25, 0.01)
DIR = (0.3, -0.5, 0.8)


def windows(sides, sync, n_windows, reps):
    """-> ms per call of every side, a list per side with one entry per window; the sides alternate inside a window"""
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
    ap.add_argument("--workloads", default="512x4096,512x65536,1x16777216")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects
    from export_ab import frame_seed
    A = bh.Attribute
    fields = [(A.POSITION.id, 0), (A.COLOR.id, 12)]
    sort = dict(key="depth", v=DIR)
    lines = [f"program_export_filtered_sorted_ab: {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
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
        bufs = {k: torch.zeros((rows, 4), dtype=torch.int32, device="cuda") for k in ("new", "loop", "sorted")}
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        cnt1 = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        prog.export(fields, bufs["sorted"].data_ptr(), 16, rows, cnt.data_ptr())
        ctx.synchronize()
        total = int(cnt.cpu()[1])
        e = bufs["sorted"][:total, 0:3].view(torch.float32)
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
            return lambda: prog.export_filtered_sorted(fields, bufs["new"].data_ptr(), 16, rows, cnt.data_ptr(), filter=flt, sort=sort)

        def loop_side(r2):
            flt = dict(kind="sphere", sphere=(0.0, 0.0, 0.0, r2))

            def run():
                base, off = bufs["loop"].data_ptr(), 0
                for fx in fxs:
                    fx.export_filtered_sorted(fields, base + off * 16, 16, rows - off, cnt1.data_ptr(), filter=flt, sort=sort)
                    ctx.synchronize()
                    off += int(cnt1[1].item())                           # the next segment starts behind what this instance kept
                result["loop"] = off
            return run

        def effect_side(r2):
            flt = dict(kind="sphere", sphere=(0.0, 0.0, 0.0, r2))
            return lambda: fxs[0].export_filtered_sorted(fields, bufs["loop"].data_ptr(), 16, rows, cnt1.data_ptr(), filter=flt, sort=sort)

        sides = {"sorted": lambda: prog.export_sorted(fields, bufs["sorted"].data_ptr(), 16, rows, cnt1.data_ptr(), scope="instance", **sort)}
        for frac in FRACTIONS:
            r2 = radii[frac][0]
            sides[f"new_{frac:g}"] = new_side(r2)
            sides[(f"effect_{frac:g}" if n_inst == 1 else f"loop_{frac:g}")] = effect_side(r2) if n_inst == 1 else loop_side(r2)
        ms = windows(sides, ctx.synchronize, args.windows, args.reps)
        med = {k: statistics.median(x) for k, x in ms.items()}
        spread = max(max(x) / min(x) - 1 for x in ms.values())
        launches = "3 launches" if cap <= 4096 else "13 launches and a memset"
        lines.append(f"workload {n_inst} instances x {cap} slots ({launches}): alive {total} of {rows}; same-run spread of the windows (largest max / min - 1 over the sides): {spread * 100:.1f} %")
        lines.append(f"  sorted       {med['sorted']:.4f} ms (min {min(ms['sorted']):.4f}, max {max(ms['sorted']):.4f}): every alive row, whatever the fraction")
        sides["sorted"](); ctx.synchronize()
        srec = bufs["sorted"][:total]
        sp = srec[:, 0:3].view(torch.float32)
        sd = (sp[:, 0] * sp[:, 0] + sp[:, 1] * sp[:, 1]) + sp[:, 2] * sp[:, 2]
        for frac in FRACTIONS:
            r2, kept = radii[frac]
            nk, ok = f"new_{frac:g}", (f"effect_{frac:g}" if n_inst == 1 else f"loop_{frac:g}")
            sides[nk](); ctx.synchronize()
            counts = [int(x) for x in cnt.cpu().numpy().view("uint32")]
            same = [counts == [kept, kept]]
            sides[ok](); ctx.synchronize()
            same.append((n_inst == 1 or result["loop"] == kept) and bool((bufs["new"][:kept] == bufs["loop"][:kept]).all()))
            same.append(bool((srec[sd <= r2] == bufs["new"][:kept]).all()))       # the sorted side, what is outside the sphere discarded
            lines.append(f"  target {frac * 100:g} %: squared radius {r2:.9g}, kept {kept} = {kept / max(total, 1) * 100:.3f} % of the alive rows; every side's output identical to the new call's: {all(same)}")
            lines.append(f"    {nk:12s} {med[nk]:.4f} ms (min {min(ms[nk]):.4f}, max {max(ms[nk]):.4f}); new / sorted = {med[nk] / med['sorted']:.3f}")
            lines.append(f"    {ok:12s} {med[ok]:.4f} ms (min {min(ms[ok]):.4f}, max {max(ms[ok]):.4f}); new / {ok.split('_')[0]} = {med[nk] / med[ok]:.3f}")
            if n_inst == 1:
                lines.append("    (one instance: reported against the effect form, no bar)")
            else:
                best = min((ok, "sorted"), key=lambda k: med[k])
                ratio = med[nk] / med[best]
                met = ratio <= 1 + spread and all(same)
                verdicts.append(met)
                lines.append(f"    new / {best.split('_')[0]} = {ratio:.3f}; bar (no slower than the faster of loop and sorted by more than the spread): {'met' if met else 'MISSED'}")
        del bufs, result, srec, sp, sd
        ctx.close()
        torch.cuda.empty_cache()
    lines.append(f"the bars of every 512-instance row: {'met' if all(verdicts) else 'MISSED'}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
