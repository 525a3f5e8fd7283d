#!/usr/bin/env python3
"""A/B of the filtered, then sorted export (hnb_effect_export_filtered_sorted: HNB_FILTER_SPHERE, HNB_SORT_KEY_DEPTH) on one effect of 16,777,216
firework particles, in the two states of tools/export_ab.py (burst: identity list, everything alive; churn: 240 frames of the c2_mixed rate spawner, a
permuted list). The sphere sits at the origin; its squared radii are chosen on the host from the state so that about 100 %, 25 % and 1 % of the alive
rows are kept (the realised fractions are printed). Records {POSITION @0, AGE @12, LIFETIME @16} at stride 32. Sides that alternate window by window
in ONE process on ONE device:

    sorted         hnb_effect_export_sorted of everything: what the new call is measured against at 100 %
    cull_F         hnb_effect_export_filtered_sorted with the sphere that keeps fraction F, the whole call
    A_F            what a user has without it, culling first: hnb_effect_export_filtered, then in torch the depth of every kept record (one op per
                   operation of the header's formula), the key transform, torch.sort(stable=True) and index_select on the records
    B_F            ... sorting first: hnb_effect_export_sorted of everything, then the predicate in torch on the sorted records and records[mask]
    (A and B synchronise the export's stream in front of torch's: two streams.)  cull_F alone is also run at 90 %, 75 % and 50 % to place the
    break-even with the sorted export.

A window is `--reps` calls between two synchronisations, timed on the host. Reported: median / min / max ms per call, the outputs of the three sides
compared, cull / min(A, B) per fraction against the same-run spread of the windows (the bar, at 25 % and 1 %), cull / sorted, the bytes of the
design's model (DESIGN.md "Filtered, then sorted": 16 B per alive row + 164 B per kept row; the sorted export: 156 B per alive row) and where cull =
sorted lies by linear interpolation between the measured fractions.

    python tools/export_filtered_sorted_ab.py --windows 10 --reps 20 --log profiles/export_filtered_sorted_ab.log
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PEAK = 8e12
FRACTIONS = (1.0, 0.25, 0.01)           # all three sides
BAR_FRACTIONS = (0.25, 0.01)
MORE_FRACTIONS = (0.9, 0.75, 0.5)       # the new call alone
ROW_BYTES, KEPT_BYTES, SORTED_BYTES = 16, 164, 156
DIR = (0.3, -0.5, 0.8)


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
    from export_ab import prepare
    from export_filtered_ab import windows
    A = bh.Attribute
    fields = [(A.POSITION.id, 0), (A.AGE.id, 12), (A.LIFETIME.id, 16)]
    sort = dict(key="depth", v=DIR)
    lines = [f"export_filtered_sorted_ab: capacity {args.capacity}, {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
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
        for frac in FRACTIONS + MORE_FRACTIONS:
            k = max(int(round(frac * alive)), 1) - 1
            r2 = float(np.partition(d, k)[k])
            radii[frac] = (r2, int((d <= np.float32(r2)).sum()))
        del p, d
        dst_a = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
        dst_b = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
        dst_c = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
        cnt, cnt_c = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
        v = [torch.tensor(c, dtype=torch.float32, device="cuda") for c in DIR]
        torch.cuda.synchronize()
        result = {}

        def flt(r2):
            return dict(kind="sphere", sphere=(0.0, 0.0, 0.0, r2))

        def side_a(r2, kept):            # cull on the device, sort in the user's own code
            def run():
                fx.export_filtered(fields, dst_a.data_ptr(), 32, cap, cnt.data_ptr(), **flt(r2))
                ctx.synchronize()
                rec = dst_a[:kept]
                q = rec[:, 0:3].view(torch.float32)
                depth = (q[:, 0] * v[0] + q[:, 1] * v[1]) + q[:, 2] * v[2]
                b = depth.view(torch.int32)
                key = torch.where(b < 0, b ^ 0x7FFFFFFF, b)              # the header's key, as a signed number of the same order
                order = torch.sort(key, stable=True).indices
                result["A"] = rec.index_select(0, order)
                torch.cuda.synchronize()
            return run

        def side_b(r2):                  # sort everything on the device, cull in the user's own code
            r2t = torch.tensor(r2, dtype=torch.float32, device="cuda")

            def run():
                fx.export_sorted(fields, dst_b.data_ptr(), 32, cap, cnt.data_ptr(), **sort)
                ctx.synchronize()
                rec = dst_b[:alive]
                e = rec[:, 0:3].view(torch.float32)                      # the centre is the origin: e = p - 0 = p
                dd = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
                result["B"] = rec[dd <= r2t]
                torch.cuda.synchronize()
            return run

        def side_cull(r2):
            return lambda: fx.export_filtered_sorted(fields, dst_c.data_ptr(), 32, cap, cnt_c.data_ptr(), filter=flt(r2), sort=sort)

        sides = {"sorted": lambda: fx.export_sorted(fields, dst_b.data_ptr(), 32, cap, cnt.data_ptr(), **sort)}
        for frac in FRACTIONS:
            sides[f"cull_{frac:g}"] = side_cull(radii[frac][0])
            sides[f"A_{frac:g}"] = side_a(*radii[frac])
            sides[f"B_{frac:g}"] = side_b(radii[frac][0])
        for frac in MORE_FRACTIONS:
            sides[f"cull_{frac:g}"] = side_cull(radii[frac][0])
        ms = windows(sides, ctx.synchronize, args.windows, args.reps)
        med = {k: statistics.median(x) for k, x in ms.items()}
        spread = max(max(x) / min(x) - 1 for x in ms.values())
        row = lambda k: f"{k:10s} {med[k]:.4f} ms (min {min(ms[k]):.4f}, max {max(ms[k]):.4f})"
        lines.append(f"state {state}: alive {alive} of {cap}; same-box spread of the windows (largest max / min - 1 over the sides): {spread * 100:.1f} %")
        lines.append(f"  {row('sorted')}; {SORTED_BYTES} B per alive row = {alive * SORTED_BYTES / 1e6:.0f} MB -> {alive * SORTED_BYTES / (med['sorted'] * 1e-3) / PEAK:.2f} of 8 TB/s")
        for frac in FRACTIONS:
            r2, kept = radii[frac]
            ck, ak, bk = f"cull_{frac:g}", f"A_{frac:g}", f"B_{frac:g}"
            sides[ak](); sides[bk](); sides[ck](); ctx.synchronize()
            counts = [int(x) for x in cnt_c.cpu().numpy().view(np.uint32)]
            same = (counts == [kept, kept] and len(result["A"]) == kept and len(result["B"]) == kept and bool((dst_c[:kept] == result["A"]).all())
                    and bool((dst_c[:kept] == result["B"]).all()))
            moved = alive * ROW_BYTES + kept * KEPT_BYTES
            best = min(med[ak], med[bk])
            ratio = med[ck] / best
            lines.append(f"  target {frac * 100:g} %: squared radius {r2:.9g}, kept {kept} = {kept / max(alive, 1) * 100:.3f} % of the alive rows; the three outputs identical: {same}")
            lines.append(f"    {row(ck)}; {ROW_BYTES} B per alive row + {KEPT_BYTES} B per kept row = {moved / 1e6:.0f} MB -> {moved / (med[ck] * 1e-3) / PEAK:.2f} of 8 TB/s")
            lines.append(f"    {row(ak)}")
            lines.append(f"    {row(bk)}")
            tail = ""
            if frac in BAR_FRACTIONS:
                ok = same and ratio <= 1 + spread
                verdicts.append(ok)
                tail = f"; bar (cull <= the faster of A and B within the spread, outputs identical): {'met' if ok else 'MISSED'}"
            lines.append(f"    cull / min(A, B) = {ratio:.3f}; cull / sorted = {med[ck] / med['sorted']:.3f}{tail}")
        curve = sorted((radii[f][1] / max(alive, 1), med[f"cull_{f:g}"]) for f in FRACTIONS + MORE_FRACTIONS)
        lines.append("  cull alone, kept fraction -> ms: " + ", ".join(f"{f:.3f} -> {t:.4f}" for f, t in curve))
        cross = None
        for (f0, t0), (f1, t1) in zip(curve, curve[1:]):
            if (t0 - med["sorted"]) * (t1 - med["sorted"]) <= 0 and t1 != t0:
                cross = f0 + (med["sorted"] - t0) * (f1 - f0) / (t1 - t0)
        model = (SORTED_BYTES - ROW_BYTES) / KEPT_BYTES
        lines.append(f"  break-even with the sorted export: the byte model says {model:.2f} kept; measured (linear between the fractions above): "
                     + (f"{cross:.2f}" if cross is not None else "none inside (0.01, 1): " + ("cull is faster everywhere" if curve[-1][1] < med["sorted"] else "cull is slower everywhere")))
        del dst_a, dst_b, dst_c
        result.clear()
        ctx.close()
    lines.append(f"the bar at 25 % and 1 % in every state: {'met' if all(verdicts) else 'MISSED'}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
