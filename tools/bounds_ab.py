#!/usr/bin/env python3
"""A/B of the particle bounds (hnb_effect_bounds / hnb_program_bounds of POSITION) against what a user has without them, sides alternating window
by window in ONE process on ONE device (the method of tools/program_export_filtered_ab.py). Firework particles.

    new      the call: one HnbBounds record (program: one per instance and the union)
    export   hnb_effect_export / hnb_program_export of POSITION at stride 12, the export's stream synchronised, then torch.aminmax over the records
             (program: over all instances' records - the union only, which is less than the call gives)
    view     torch directly on the POSITION plane of hnb_effect_device_view / hnb_program_device_view, gathered through the alive list, then
             torch.aminmax (program: instance by instance, then over the instances)

Workloads: one effect of 16,777,216 slots after the burst (all alive), in steady churn (a rate spawner of capacity / mean lifetime per second: the
c2_mixed regime) and late in the die-off of the burst; 512 instances x 4096 slots and 512 x 65,536 (C4) after the burst. The alive counts the
alternatives slice by are taken once on the host, outside the windows (the state does not change while the sides run). Every side's box is compared
with the new call's. The bar, against the alternatives and never against the code under test: new is no slower than the faster of export and view
by more than the same-run spread of the windows (largest max / min - 1 over the sides), in every row. Also reported: the time against the modelled
bytes, capacity x (1 + 4 x 3) per instance less 48 for every quad of four free slots.

    python tools/bounds_ab.py --windows 10 --reps 20 --log profiles/bounds_ab.log
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
MEAN_LIFETIME = 1.0
WORKLOADS = ("1x16777216:burst", "1x16777216:churn", "1x16777216:dieoff", "512x4096:burst", "512x65536:burst")


class Raw:
    """device memory the library owns, as torch sees an array of another library"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


def prepare(n_inst, cap, state):
    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects
    from export_ab import frame_seed
    ctx = bh.Context(0)
    churn = state == "churn"
    asset = effects.firework_trails(cap, bh.SpawnerSettings.rate(float(cap) / MEAN_LIFETIME)) if churn else effects.firework_trails(cap)
    prog = ctx.create_program(bh.lower(asset))
    fxs = [prog.create_effect(slot_base=k * cap) for k in range(n_inst)]
    if churn:
        sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
        for f in range(240):
            ctx.frame_begin(1 / 60, f / 60)
            n = sp.tick(1 / 60, rng)
            for k, fx in enumerate(fxs):
                fx.set_frame(n, frame_seed(f * 7 + k))
            ctx.simulate()
    else:
        frames, dt = (66, 1 / 60) if state == "dieoff" else (6, 1 / 600)
        for f in range(frames):
            ctx.frame_begin(dt, f * dt)
            for k, fx in enumerate(fxs):
                fx.set_frame(cap if f == 0 else 0, frame_seed(f * 7 + k))
            ctx.simulate()
    ctx.synchronize()
    return ctx, prog, fxs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import torch

    import bevy_hanabi_amd as bh
    from export_sorted_ab import windows
    A = bh.Attribute
    fields = [(A.POSITION.id, 0)]
    lines = [f"bounds_ab: POSITION, {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
    verdicts = []
    for w in [x for x in args.workloads.split(",") if x]:
        shape, state = w.split(":")
        n_inst, cap = (int(x) for x in shape.split("x"))
        ctx, prog, fxs = prepare(n_inst, cap, state)
        program = n_inst > 1
        counts = [fx.alive_count() for fx in fxs]
        total, rows = sum(counts), n_inst * cap
        # the modelled bytes: every alive byte, and the plane of every quad that holds an alive slot
        quads_read = 0
        for fx in fxs[: 1 if not program else n_inst]:
            mask = np.zeros((cap + 3) // 4 * 4, bool)
            mask[fx.alive_list()] = True
            quads_read += int(mask.reshape(-1, 4).any(axis=1).sum())
        moved = rows + quads_read * 48
        full = rows * 13
        rec = torch.zeros((n_inst + 2) * 12, dtype=torch.int32, device="cuda")
        dst = torch.zeros((rows, 3), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        result = {}
        target = prog if program else fxs[0]

        def new_side():
            target.bounds(A.POSITION.id, rec.data_ptr(), n_inst + 1)

        def export_side():
            if program:
                prog.export(fields, dst.data_ptr(), 12, rows, cnt.data_ptr())
            else:
                fxs[0].export(fields, dst.data_ptr(), 12, rows, cnt.data_ptr())
            ctx.synchronize()
            result["export"] = torch.aminmax(dst[:total], dim=0)
            torch.cuda.synchronize()

        # the planes and lists where the library keeps them (the list's column and head do not change while the sides run; no ring lists here)
        views = []
        if program:
            pv = prog.device_view()
            pos_off = [a.plane_off for a in pv.attrs[: pv.n_attrs] if a.attr == A.POSITION.id][0]
            slabs = torch.as_tensor(Raw(pv.slabs, (n_inst,), "<i8"), device="cuda").cpu().tolist()
            metas = torch.as_tensor(Raw(pv.meta, (n_inst, 8), "<i4"), device="cuda").cpu().numpy().view(np.uint32)
            for k in range(n_inst):
                assert metas[k, 2] >> 1 == 0
                views.append((torch.as_tensor(Raw(slabs[k] + pos_off, (cap, 3), "<f4"), device="cuda"),
                              torch.as_tensor(Raw(slabs[k] + pv.alive_list_off[int(metas[k, 2]) & 1], (cap,), "<i4"), device="cuda"), counts[k]))
        else:
            v = fxs[0].device_view()
            plane = [a.plane for a in v.attrs[: v.n_attrs] if a.attr == A.POSITION.id][0]
            meta = torch.as_tensor(Raw(v.meta, (8,), "<i4"), device="cuda").cpu().numpy().view(np.uint32)
            assert meta[2] >> 1 == 0 and meta[0] == total
            views.append((torch.as_tensor(Raw(plane, (cap, 3), "<f4"), device="cuda"),
                          torch.as_tensor(Raw(v.alive_list[int(meta[2]) & 1], (cap,), "<i4"), device="cuda"), total))

        def view_side():
            ctx.synchronize()                                            # (the frames are done; torch's stream is not the simulation's)
            los, his = [], []
            for plane_t, list_t, n in views:
                if n:
                    lo, hi = torch.aminmax(plane_t[list_t[:n].long()], dim=0)
                    los.append(lo); his.append(hi)
            result["view"] = (torch.stack(los).amin(dim=0), torch.stack(his).amax(dim=0))
            torch.cuda.synchronize()

        sides = {"new": new_side, "export": export_side, "view": view_side}
        ms = windows(sides, ctx.synchronize, args.windows, args.reps)
        med = {k: statistics.median(x) for k, x in ms.items()}
        spread = max(max(x) / min(x) - 1 for x in ms.values())
        for fn in sides.values():
            fn()
        ctx.synchronize()
        box = rec.cpu().numpy().view(np.uint32).reshape(-1, 12)[n_inst if program else 0]
        lo, hi = box[:3].view(np.float32), box[4:7].view(np.float32)
        same = box[8] == total and box[9] == 0
        for k in ("export", "view"):
            same = same and bool((result[k][0].cpu().numpy() == lo).all()) and bool((result[k][1].cpu().numpy() == hi).all())
        best = min(("export", "view"), key=lambda k: med[k])
        ratio = med["new"] / med[best]
        met = bool(ratio <= 1 + spread and same)
        verdicts.append(met)
        launches = (1 if cap <= 4096 else 2) + (1 if program else 0)
        lines.append(f"workload {n_inst} x {cap}, {state} ({launches} launches): alive {total} of {rows}; box lo {lo.tolist()} hi {hi.tolist()}; every side's box equal to the new call's: {bool(same)}; "
                     f"same-run spread of the windows (largest max / min - 1 over the sides): {spread * 100:.1f} %")
        lines.append(f"    new      {med['new']:.4f} ms (min {min(ms['new']):.4f}, max {max(ms['new']):.4f}); modelled {moved / 1e6:.1f} MB ({full / 1e6:.1f} MB less the quads of free slots) -> "
                     f"{moved / (med['new'] * 1e-3) / 1e12:.2f} TB/s")
        for k in ("export", "view"):
            lines.append(f"    {k:8s} {med[k]:.4f} ms (min {min(ms[k]):.4f}, max {max(ms[k]):.4f}); new / {k} = {med['new'] / med[k]:.3f}")
        lines.append(f"    new / {best} = {ratio:.3f}; bar (no slower than the faster of export and view by more than the spread): {'met' if met else 'MISSED'}")
        del views, dst, rec, result
        ctx.close()
        torch.cuda.empty_cache()
    lines.append(f"the bar of every row: {'met' if all(verdicts) else 'MISSED'}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
