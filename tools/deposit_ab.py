#!/usr/bin/env python3
"""A/B of the deposit (hnb_effect_deposit) against what a user does without it, on one effect of 16,777,216 firework particles - c2's burst after
`--frames` frames of 1/60 s, so that the cloud has spread - the sides alternating window by window in ONE process on ONE device, for a grid of 8^3
cells (the table in LDS: k_deposit_lds) and one of 64^3 (k_deposit_global) around the cloud, with 0 channels and with 1 (VELOCITY.y, frac_bits 16):

    deposit   hnb_effect_deposit into count (and sums)
    binned    (a) hnb_effect_export_binned of {POSITION @0, VELOCITY @12} at stride 32, the count as the differences of cell_start and, with a
              channel, a segmented sum of the records' source in torch (f32: the order is the sort's, but the library gives no bit-exact recipe)
    binonly   the same call into a destination of 0 records: keys, sort and table alone - the export-free floor of (a), counts only
    torch     (b) hnb_effect_export of the same fields, the cell computed in torch binary32, torch.bincount and index_add_

A window is `--reps` calls between two synchronisations, timed on the host. Reported: median / min / max ms per call and, per baseline, the spread
of its own windows (max / min - 1): deposit is said to be faster only where it beats the baseline's median by more than that. Before any time is
taken the deposited grid is checked on the device: count against the differences of cell_start and against bincount, sums against an int64
index_add_ of round-half-even(float64(v) * 2^16). In front of that state the worst case once, deposit alone: frame 0 of the burst, every particle
at one point. Kernel times need a run of their own:
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/deposit_ab.py --only deposit --windows 2 --reps 5`.

    python tools/deposit_ab.py --windows 6 --reps 10 --log profiles/deposit_ab.log
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FRAC = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--grids", default="8,64")
    ap.add_argument("--only", default="", help="comma-separated sides to time (deposit, binned, binonly, torch): a kernel trace wants deposit alone")
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects
    from export_ab import frame_seed
    from export_sorted_ab import windows
    A = bh.Attribute
    cap = args.capacity
    fields = [(A.POSITION.id, 0), (A.VELOCITY.id, 12)]
    lines = [f"deposit_ab: capacity {cap}, {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()

    def frame(f, dt):
        ctx.frame_begin(dt, f * dt)
        fx.set_frame(cap if f == 0 else 0, frame_seed(f))
        ctx.simulate()

    dst = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                             # (the fills run on torch's stream, the calls on the simulation's)
    ok_all = True

    def run_state(name, timed):
        nonlocal ok_all
        alive = fx.alive_count()
        fx.export(fields, dst.data_ptr(), 32, cap, cnt.data_ptr())        # the box of the cloud, from the plain export's records
        ctx.synchronize()
        p = dst[:alive, 0:3].view(torch.float32)
        lo, hi = p.min(dim=0).values.double(), p.max(dim=0).values.double()
        size = torch.clamp(hi - lo, min=1e-3)
        origin = (lo - 0.01 * size).float().cpu().numpy()
        lines.append(f"state {name}: alive {alive} of {cap}; box {[round(float(x), 4) for x in lo.cpu()]} .. {[round(float(x), 4) for x in hi.cpu()]}")
        for g in [int(x) for x in args.grids.split(",")]:
            dims = (g, g, g)
            n_cells = g ** 3
            inv_cell = (torch.tensor(dims, dtype=torch.float64, device="cuda") / (1.02 * size)).float().cpu().numpy()
            o, iv, dm = torch.tensor(origin, device="cuda"), torch.tensor(inv_cell, device="cuda"), torch.tensor(dims, dtype=torch.float32, device="cuda")
            table = torch.zeros(n_cells + 2, dtype=torch.int32, device="cuda")
            count = torch.zeros(n_cells + 1, dtype=torch.int32, device="cuda")
            sums = torch.zeros(n_cells + 1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()

            def cells_of(pos):                                           # the header's formulas in torch binary32, operation by operation
                t = (pos - o) * iv
                inside = ((t >= 0) & (t < dm)).all(dim=1)
                i = torch.where(inside[:, None], t, torch.zeros_like(t)).to(torch.int64)
                return torch.where(inside, (i[:, 2] * g + i[:, 1]) * g + i[:, 0], torch.full_like(i[:, 0], n_cells))

            grid = dict(dims=dims, origin=origin, inv_cell=inv_cell)
            keep = {}

            def binned(k):
                fx.export_binned(fields, dst.data_ptr(), 32, cap, cnt.data_ptr(), cell_start_ptr=table.data_ptr(), **grid)
                ctx.synchronize()                                        # the consumer runs on torch's stream
                keep["count"] = torch.diff(table[: n_cells + 2])
                if k:
                    keep["sum"] = torch.segment_reduce(dst[:alive, 4].view(torch.float32), "sum", lengths=keep["count"].to(torch.int64))
                torch.cuda.synchronize()

            def by_torch(k):
                fx.export(fields, dst.data_ptr(), 32, cap, cnt.data_ptr())
                ctx.synchronize()
                cells = cells_of(dst[:alive, 0:3].view(torch.float32))
                keep["count"] = torch.bincount(cells, minlength=n_cells + 1)
                if k:
                    keep["sum"] = torch.zeros(n_cells + 1, device="cuda").index_add_(0, cells, dst[:alive, 4].view(torch.float32))
                torch.cuda.synchronize()

            for k in (0, 1):
                ch = [(A.VELOCITY.id, 1, FRAC)][:k]
                deposit = lambda: fx.deposit(count_ptr=count.data_ptr(), channels=ch, sums_ptr=sums.data_ptr() if k else None, stats_ptr=stats.data_ptr(), **grid)
                # ---- the result, on the device, before any time is taken
                deposit()
                binned(k)
                ctx.synchronize()
                from_table = keep["count"].clone()
                by_torch(k)
                cells = cells_of(dst[:alive, 0:3].view(torch.float32))
                ok = bool((count == from_table).all()) and bool((count.to(torch.int64) == keep["count"]).all()) and int(stats[0]) == alive and int(stats[1]) == int(count[n_cells])
                if k:
                    q = torch.round(dst[:alive, 4].view(torch.float32).double() * 2.0 ** FRAC).to(torch.int64)
                    ok = ok and bool((sums == torch.zeros(n_cells + 1, dtype=torch.int64, device="cuda").index_add_(0, cells, q)).all()) and int(stats[2]) == 0
                ok_all = ok_all and ok
                occupied = int((count[:n_cells] != 0).sum())
                lines.append(f"  grid {g}^3, {k} channel(s): deposit == differences of cell_start == bincount{' and sums == int64 index_add_' if k else ''}, on the device: {ok}; "
                             f"occupied cells {occupied} of {n_cells}, outside {int(count[n_cells])}, fullest cell {int(count[:n_cells].max())}")
                if not ok:
                    return
                sides = {"deposit": deposit}
                if timed:
                    sides.update({"binned": lambda: binned(k), "torch": lambda: by_torch(k)})
                    if not k:
                        sides["binonly"] = lambda: fx.export_binned(fields, dst.data_ptr(), 32, 0, None, cell_start_ptr=table.data_ptr(), **grid)
                if args.only:
                    sides = {s: fn for s, fn in sides.items() if s in args.only.split(",")}
                ms = windows(sides, ctx.synchronize, args.windows if timed else 2, args.reps)
                med = {s: statistics.median(x) for s, x in ms.items()}
                for s in sides:
                    lines.append(f"    {s:8s} {med[s]:.4f} ms (min {min(ms[s]):.4f}, max {max(ms[s]):.4f})")
                for s in sides:
                    if s != "deposit" and "deposit" in sides:
                        spread = max(ms[s]) / min(ms[s]) - 1
                        faster = med["deposit"] * (1 + spread) < med[s]
                        lines.append(f"    {s} / deposit = {med[s] / med['deposit']:.2f}; spread of {s}'s own windows {spread * 100:.1f} %: "
                                     f"{'deposit is faster beyond it' if faster else 'not claimed'}")

    frame(0, 0.0)                                                        # a tick of no time: spawned and initialised, nothing has moved
    ctx.synchronize()
    run_state("frame 0 (every particle at one point: the worst case, deposit alone)", False)
    for f in range(1, args.frames):
        frame(f, 1 / 60)
    ctx.synchronize()
    run_state(f"burst after {args.frames} frames of 1/60 s", True)
    ctx.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
