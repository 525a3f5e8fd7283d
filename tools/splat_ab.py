#!/usr/bin/env python3
"""A/B of the splat (hnb_effect_splat) against two baselines that are not the code under test, on one effect of 16,777,216 firework particles - c2's
burst after `--frames` frames of 1/60 s, so that the cloud has spread - the sides alternating window by window in ONE process on ONE device, for a grid
of 8^3 cells (the table in LDS: k_splat_lds) and one of 64^3 (k_splat_global) around the cloud, with 0, 1 (VELOCITY.y) and 4 channels (VELOCITY.xyz and
LIFETIME), all at frac_bits 16:

    splat     hnb_effect_splat into count (and sums)
    deposit   hnb_effect_deposit on the same grid and channels: the nearest-cell cost, which the splat's eight adds per contribution multiply
    torch     what a user does without the call: hnb_effect_export of POSITION, VELOCITY and LIFETIME, the cell and the stencil in torch binary32
              operation by operation, torch.bincount for the count and, per corner, one f32 index_add_ of the weighted values

A window is `--reps` calls between two synchronisations, timed on the host. Reported: median / min / max ms per call, the ratio to the nearest deposit
(no threshold) and, for the torch route, the spread of its own windows (max / min - 1): the splat is said to be faster only where it beats the torch
route's median by more than that. Before any time is taken the splatted grid is checked on the device: count against torch.bincount of the restated
cells, sums against an int64 index_add_ of round-half-even(float64(v * W) * 2^16) per corner, the weights restated in binary32. In front of that state
the worst case once, the splat alone on the LDS grid: frame 0 of the burst, every particle at one point (eight hot rows). Kernel times need a run
of their own: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/splat_ab.py --only splat --windows 2 --reps 5`.

    python tools/splat_ab.py --windows 6 --reps 10 --log profiles/splat_ab.log
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
    ap.add_argument("--channels", default="0,1,4")
    ap.add_argument("--only", default="", help="comma-separated sides to time (splat, deposit, torch): a kernel trace wants splat alone")
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects
    from export_ab import frame_seed
    from export_sorted_ab import windows
    A = bh.Attribute
    cap = args.capacity
    fields = [(A.POSITION.id, 0), (A.VELOCITY.id, 12), (A.LIFETIME.id, 24)]
    # (attribute, component, frac_bits) and the source's word in the exported record
    all_channels = [((A.VELOCITY.id, 1, FRAC), 4), ((A.VELOCITY.id, 0, FRAC), 3), ((A.VELOCITY.id, 2, FRAC), 5), ((A.LIFETIME.id, 0, FRAC), 6)]
    lines = [f"splat_ab: capacity {cap}, {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
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

    def run_state(name, timed, grids):
        nonlocal ok_all
        alive = fx.alive_count()
        fx.export(fields, dst.data_ptr(), 32, cap, cnt.data_ptr())        # the box of the cloud, from the plain export's records
        ctx.synchronize()
        p = dst[:alive, 0:3].view(torch.float32)
        lo, hi = p.min(dim=0).values.double(), p.max(dim=0).values.double()
        size = torch.clamp(hi - lo, min=1e-3)
        origin = (lo - 0.01 * size).float().cpu().numpy()
        lines.append(f"state {name}: alive {alive} of {cap}; box {[round(float(x), 4) for x in lo.cpu()]} .. {[round(float(x), 4) for x in hi.cpu()]}")
        for g in grids:
            dims = (g, g, g)
            n_cells = g ** 3
            inv_cell = (torch.tensor(dims, dtype=torch.float64, device="cuda") / (1.02 * size)).float().cpu().numpy()
            o, iv, dm = torch.tensor(origin, device="cuda"), torch.tensor(inv_cell, device="cuda"), torch.tensor(dims, dtype=torch.float32, device="cuda")
            count = torch.zeros(n_cells + 1, dtype=torch.int32, device="cuda")
            near_count = torch.zeros(n_cells + 1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            grid = dict(dims=dims, origin=origin, inv_cell=inv_cell)

            def stencil(pos):
                """the header's formulas in torch binary32, operation by operation -> (cells [n], inside [n], rows [8][m], W [8][m] of the m inside particles)"""
                t = (pos - o) * iv
                inside = ((t >= 0) & (t < dm)).all(dim=1)
                i = torch.where(inside[:, None], t, torch.zeros_like(t)).to(torch.int64)
                cells = torch.where(inside, (i[:, 2] * g + i[:, 1]) * g + i[:, 0], torch.full_like(i[:, 0], n_cells))
                u = t[inside] - 0.5
                fl = torch.floor(u)
                w1 = u - fl
                w0 = 1.0 - w1
                j = fl.to(torch.int64)
                idx = (torch.clamp(j, min=0), torch.clamp(j + 1, max=g - 1))
                w = (w0, w1)
                rows, W = [], []
                for c in range(8):
                    a, b, z = c & 1, (c >> 1) & 1, c >> 2
                    rows.append((idx[z][:, 2] * g + idx[b][:, 1]) * g + idx[a][:, 0])
                    W.append((w[a][:, 0] * w[b][:, 1]) * w[z][:, 2])
                return cells, inside, rows, W

            keep = {}

            def by_torch(k):
                fx.export(fields, dst.data_ptr(), 32, cap, cnt.data_ptr())
                ctx.synchronize()                                        # the consumer runs on torch's stream
                rec = dst[:alive]
                cells, inside, rows, W = stencil(rec[:, 0:3].view(torch.float32))
                keep["count"] = torch.bincount(cells, minlength=n_cells + 1)
                if k:
                    words = [w for _, w in all_channels[:k]]
                    v = rec[:, words].view(torch.float32)
                    out = torch.zeros((n_cells + 1, k), device="cuda")
                    out.index_add_(0, cells[~inside], v[~inside])
                    vin = v[inside]
                    for c in range(8):
                        out.index_add_(0, rows[c], vin * W[c][:, None])
                    keep["sum"] = out
                torch.cuda.synchronize()

            for k in [int(x) for x in args.channels.split(",")]:
                ch = [c for c, _ in all_channels[:k]]
                sums = torch.zeros((n_cells + 1, max(k, 1)), dtype=torch.int64, device="cuda")
                near_sums = torch.zeros((n_cells + 1, max(k, 1)), dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                splat = lambda: fx.splat(count_ptr=count.data_ptr(), channels=ch, sums_ptr=sums.data_ptr() if k else None, stats_ptr=stats.data_ptr(), **grid)
                deposit = lambda: fx.deposit(count_ptr=near_count.data_ptr(), channels=ch, sums_ptr=near_sums.data_ptr() if k else None, stats_ptr=stats.data_ptr(), **grid)
                # ---- the result, on the device, before any time is taken
                deposit()
                splat()
                fx.export(fields, dst.data_ptr(), 32, cap, cnt.data_ptr())
                ctx.synchronize()
                rec = dst[:alive]
                cells, inside, rows, W = stencil(rec[:, 0:3].view(torch.float32))
                ok = bool((count.to(torch.int64) == torch.bincount(cells, minlength=n_cells + 1)).all()) and bool((count == near_count).all())
                ok = ok and int(stats[0]) == alive and int(stats[1]) == int(count[n_cells]) and int(stats[2]) == 0
                differ = 0
                if k:
                    v = rec[:, [w for _, w in all_channels[:k]]].view(torch.float32)
                    want = torch.zeros((n_cells + 1, k), dtype=torch.int64, device="cuda")
                    want.index_add_(0, cells[~inside], torch.round(v[~inside].double() * 2.0 ** FRAC).to(torch.int64))
                    vin = v[inside]
                    for c in range(8):
                        cv = vin * W[c][:, None]                         # one rounded binary32 product
                        want.index_add_(0, rows[c], torch.round(cv.double() * 2.0 ** FRAC).to(torch.int64))
                    ok = ok and bool((sums == want).all())
                    differ = int((sums[:n_cells] != near_sums[:n_cells]).any(dim=1).sum())
                    del want, vin, v
                del cells, inside, rows, W
                ok_all = ok_all and ok
                occupied = int((count[:n_cells] != 0).sum())
                lines.append(f"  grid {g}^3, {k} channel(s): splat == bincount of the restated cells == the deposit's count"
                             f"{' and sums == int64 index_add_ of the restated corner contributions' if k else ''}, on the device: {ok}; occupied cells {occupied} of {n_cells}, "
                             f"outside {int(count[n_cells])}, fullest cell {int(count[:n_cells].max())}, cells whose sums differ from the nearest deposit's {differ}")
                if not ok:
                    return
                sides = {"splat": splat}
                if timed:
                    sides.update({"deposit": deposit, "torch": lambda: by_torch(k)})
                if args.only:
                    sides = {s: fn for s, fn in sides.items() if s in args.only.split(",")}
                ms = windows(sides, ctx.synchronize, args.windows if timed else 2, args.reps)
                med = {s: statistics.median(x) for s, x in ms.items()}
                for s in sides:
                    lines.append(f"    {s:8s} {med[s]:.4f} ms (min {min(ms[s]):.4f}, max {max(ms[s]):.4f})")
                if "splat" in sides and "deposit" in sides:
                    lines.append(f"    splat / deposit = {med['splat'] / med['deposit']:.2f} (reported, no threshold)")
                if "splat" in sides and "torch" in sides:
                    spread = max(ms["torch"]) / min(ms["torch"]) - 1
                    faster = med["splat"] * (1 + spread) < med["torch"]
                    lines.append(f"    torch / splat = {med['torch'] / med['splat']:.2f}; spread of torch's own windows {spread * 100:.1f} %: "
                                 f"{'splat is faster beyond it' if faster else 'not claimed'}")
                keep.clear()
                print("\n".join(lines[-6:]), flush=True)

    frame(0, 0.0)                                                        # a tick of no time: spawned and initialised, nothing has moved
    ctx.synchronize()
    run_state("frame 0 (every particle at one point, eight hot rows: the worst case, splat alone, the LDS grid)", False, [8])
    for f in range(1, args.frames):
        frame(f, 1 / 60)
    ctx.synchronize()
    run_state(f"burst after {args.frames} frames of 1/60 s", True, [int(x) for x in args.grids.split(",")])
    ctx.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
