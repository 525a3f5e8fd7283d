#!/usr/bin/env python3
"""A/B of the sample (hnb_effect_sample) against what a consumer composes without it, on one effect of 16,777,216 firework particles - c2's burst after
`--frames` frames of 1/60 s, so that the cloud has spread - the sides alternating window by window in ONE process on ONE device, for a grid around
the cloud (a box 2 % wider) and three fields: 8^3 x 4, 64^3 x 1 and 64^3 x 4 channels, NEAREST and TRILINEAR, added into VELOCITY (one channel:
VELOCITY.y; four: VELOCITY.xyz and LIFETIME, whose channel of the field is zero):

    sample    hnb_effect_sample
    torch     hnb_effect_export of {POSITION @0, VELOCITY @12, LIFETIME @24} at stride 32, the header's rule restated in torch binary32 on the device
              operation by operation (cell arithmetic, eight indexed gathers, seven blends, scale, add), hnb_effect_import of VELOCITY (and LIFETIME)
              by rows
    nostats   hnb_effect_sample with out_stats NULL: what the per-wave adds onto the three stats words cost
    bounds    hnb_effect_bounds of POSITION: k_bounds_tile reads the alive bytes and POSITION, the planes the sample's walk reads before its gathers

A window is `--reps` calls between two synchronisations, timed on the host. Reported: median / min / max ms per call, the spread of the baseline's own
windows (max / min - 1) - sample is said to be faster only where it beats the baseline's median by more than that - and the plane bytes a call moves
over its time. Before any time is taken both sides run from the same saved planes and the exported records are compared on the device, bit for bit.
At the end the first frame after a sample call is timed against a plain frame. Kernel times need a run of their own:
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sample_ab.py --only sample --windows 2 --reps 5`.

    python tools/sample_ab.py --windows 6 --reps 10 --log profiles/sample_ab.log
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SCALE = 0.01
CASES = ((8, 4), (64, 1), (64, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated sides to time (sample, nostats, torch, bounds): a kernel trace wants sample alone")
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects, runtime
    from export_ab import frame_seed
    from export_sorted_ab import windows
    A = bh.Attribute
    cap = args.capacity
    exported = [(A.POSITION.id, 0), (A.VELOCITY.id, 12), (A.LIFETIME.id, 24)]
    lines = [f"sample_ab: capacity {cap}, {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()

    def frame(f, dt, t):
        ctx.frame_begin(dt, t)
        fx.set_frame(cap if f == 0 else 0, frame_seed(f))
        ctx.simulate()

    dst = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    dst_f = dst.view(torch.float32)
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    box = torch.zeros(16, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                             # (the fills run on torch's stream, the calls on the simulation's)
    for f in range(args.frames):
        frame(f, 0.0 if f == 0 else 1 / 60, f / 60)
    ctx.synchronize()
    alive = fx.alive_count()
    fx.export(exported, dst.data_ptr(), 32, cap, cnt.data_ptr())          # the box of the cloud, from the plain export's records
    ctx.synchronize()
    p = dst_f[:alive, 0:3]
    lo, hi = p.min(dim=0).values.double(), p.max(dim=0).values.double()
    size = torch.clamp(hi - lo, min=1e-3)
    origin = (lo - 0.01 * size).float().cpu().numpy()
    lines.append(f"state: burst after {args.frames} frames of 1/60 s, alive {alive} of {cap}; box {[round(float(x), 4) for x in lo.cpu()]} .. {[round(float(x), 4) for x in hi.cpu()]}")
    saved = {a: fx.read_attr(a) for a in (A.VELOCITY.id, A.LIFETIME.id)}  # both sides start from these planes

    def restore():
        for a, v in saved.items():
            fx.write_attr(a, v)

    ok_all = True
    for g, k in CASES:
        dims, n_cells = (g, g, g), g ** 3
        inv_cell = (torch.tensor(dims, dtype=torch.float64, device="cuda") / (1.02 * size)).float().cpu().numpy()
        o, iv = torch.tensor(origin, device="cuda"), torch.tensor(inv_cell, device="cuda")
        field = torch.randn((n_cells, k), generator=torch.Generator(device="cuda").manual_seed(g * 10 + k), device="cuda") * 30.0
        if k == 4:
            field[:, 3] = 0.0                                            # LIFETIME + 0 * scale: the lifetimes stay what they are
        ch = [(A.VELOCITY.id, 1, runtime.SAMPLE_ADD)] if k == 1 else [(A.VELOCITY.id, c, runtime.SAMPLE_ADD) for c in range(3)] + [(A.LIFETIME.id, 0, runtime.SAMPLE_ADD)]
        imported = [(A.VELOCITY.id, 12)] + ([(A.LIFETIME.id, 24)] if k == 4 else [])
        torch.cuda.synchronize()
        # plane bytes per slot: the alive byte, POSITION read, VELOCITY read and written as whole quads (and LIFETIME)
        plane_bytes = cap * (1 + 12 + 24 + (8 if k == 4 else 0))
        for mode, mode_name in ((runtime.SAMPLE_NEAREST, "nearest"), (runtime.SAMPLE_TRILINEAR, "trilinear")):
            def sample():
                fx.sample(dims, origin, inv_cell, field.data_ptr(), ch, mode, SCALE, stats.data_ptr())

            def sample_no_stats():
                fx.sample(dims, origin, inv_cell, field.data_ptr(), ch, mode, SCALE, None)

            def by_torch():
                fx.export(exported, dst.data_ptr(), 32, cap, cnt.data_ptr())
                ctx.synchronize()                                        # the consumer runs on torch's stream
                pos = dst_f[:alive, 0:3]
                t = (pos - o) * iv
                inside = ((t >= 0) & (t < float(g))).all(dim=1)
                if mode == runtime.SAMPLE_NEAREST:
                    i = torch.where(inside[:, None], t, torch.zeros_like(t)).to(torch.int64)
                    s = field[(i[:, 2] * g + i[:, 1]) * g + i[:, 0]]
                else:
                    u = t - 0.5
                    fl = torch.floor(u)
                    w = u - fl
                    j = torch.where(inside[:, None], fl, torch.zeros_like(fl)).to(torch.int64)
                    l, h = torch.clamp(j, min=0), torch.clamp(j + 1, max=g - 1)
                    F = lambda x, y, z: field[(z * g + y) * g + x]
                    lerp = lambda a, b, wc: a + wc * (b - a)             # (three kernels: every operation is rounded on its own)
                    w0, w1, w2 = w[:, 0:1], w[:, 1:2], w[:, 2:3]
                    a00 = lerp(F(l[:, 0], l[:, 1], l[:, 2]), F(h[:, 0], l[:, 1], l[:, 2]), w0)
                    a10 = lerp(F(l[:, 0], h[:, 1], l[:, 2]), F(h[:, 0], h[:, 1], l[:, 2]), w0)
                    a01 = lerp(F(l[:, 0], l[:, 1], h[:, 2]), F(h[:, 0], l[:, 1], h[:, 2]), w0)
                    a11 = lerp(F(l[:, 0], h[:, 1], h[:, 2]), F(h[:, 0], h[:, 1], h[:, 2]), w0)
                    s = lerp(lerp(a00, a10, w1), lerp(a01, a11, w1), w2)
                r = s * SCALE
                if k == 1:
                    dst_f[:alive, 4] = torch.where(inside, dst_f[:alive, 4] + r[:, 0], dst_f[:alive, 4])
                else:
                    dst_f[:alive, 3:6] = torch.where(inside[:, None], dst_f[:alive, 3:6] + r[:, 0:3], dst_f[:alive, 3:6])
                    dst_f[:alive, 6] = torch.where(inside, dst_f[:alive, 6] + r[:, 3], dst_f[:alive, 6])
                torch.cuda.synchronize()
                fx.import_records(imported, dst.data_ptr(), 32, cap)

            def bounds():
                fx.bounds(A.POSITION.id, box.data_ptr())

            # ---- the result, on the device, before any time is taken: both sides from the saved planes
            restore()
            sample()
            fx.export(exported, dst.data_ptr(), 32, cap, cnt.data_ptr())
            ctx.synchronize()
            got = dst[:alive, 3:7].clone()
            st = stats.cpu().tolist()
            restore()
            by_torch()
            fx.export(exported, dst.data_ptr(), 32, cap, cnt.data_ptr())
            ctx.synchronize()
            ok = bool((got == dst[:alive, 3:7]).all()) and st[0] == alive and st[1] + st[2] == alive
            ok_all = ok_all and ok
            lines.append(f"  field {g}^3 x {k}, {mode_name}: sample == export + torch + import, bit for bit on the device: {ok}; sampled {st[1]}, outside {st[2]}")
            if not ok:
                continue
            restore()
            sides = {"sample": sample, "nostats": sample_no_stats, "torch": by_torch, "bounds": bounds}
            if args.only:
                sides = {s: fn for s, fn in sides.items() if s in args.only.split(",")}
            ms = windows(sides, ctx.synchronize, args.windows, args.reps)
            med = {s: statistics.median(x) for s, x in ms.items()}
            for s in sides:
                lines.append(f"    {s:8s} {med[s]:.4f} ms (min {min(ms[s]):.4f}, max {max(ms[s]):.4f})")
            if "sample" in sides:
                lines.append(f"    sample: {plane_bytes / 1e6:.0f} MB of planes per call = {plane_bytes / med['sample'] / 1e9:.2f} TB/s of plane traffic; field {n_cells * k * 4 / 1024:.0f} KiB")
            if "sample" in sides and "nostats" in sides:
                lines.append(f"    nostats: {plane_bytes / med['nostats'] / 1e9:.2f} TB/s of plane traffic; sample / nostats = {med['sample'] / med['nostats']:.2f} in time")
            if "sample" in sides and "bounds" in sides:
                lines.append(f"    bounds reads {cap * 13 / 1e6:.0f} MB = {cap * 13 / med['bounds'] / 1e9:.2f} TB/s; sample / bounds = {med['sample'] / med['bounds']:.2f} in time")
            if "sample" in sides and "torch" in sides:
                spread = max(ms["torch"]) / min(ms["torch"]) - 1
                faster = med["sample"] * (1 + spread) < med["torch"]
                lines.append(f"    torch / sample = {med['torch'] / med['sample']:.1f}; spread of torch's own windows {spread * 100:.1f} %: {'sample is faster beyond it' if faster else 'not claimed'}")
    # ---- the first frame after a sample call against a plain frame (a tiny dt: the state stays what it is)
    restore()
    g, k = 8, 4
    dims = (g, g, g)
    inv_cell = (torch.tensor(dims, dtype=torch.float64, device="cuda") / (1.02 * size)).float().cpu().numpy()
    field = torch.zeros((g ** 3, 1), device="cuda")
    torch.cuda.synchronize()
    plain, after = [], []
    f = args.frames
    for i in range(2 * max(args.windows, 4) + 2):
        if i % 2:
            fx.sample(dims, origin, inv_cell, field.data_ptr(), [(A.VELOCITY.id, 1, runtime.SAMPLE_ADD)], runtime.SAMPLE_TRILINEAR, SCALE)
        ctx.synchronize()
        t0 = time.perf_counter()
        frame(f, 1e-6, args.frames / 60 + (f - args.frames) * 1e-6)
        ctx.synchronize()
        if i >= 2:                                                       # (the first of each kind warms up)
            (after if i % 2 else plain).append((time.perf_counter() - t0) * 1e3)
        f += 1
    lines.append(f"frame after a sample call {statistics.median(after):.4f} ms (min {min(after):.4f}, max {max(after):.4f}); plain frame {statistics.median(plain):.4f} ms "
                 f"(min {min(plain):.4f}, max {max(plain):.4f})")
    ctx.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
