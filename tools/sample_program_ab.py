#!/usr/bin/env python3
"""A/B of the sample's program form (hnb_program_sample) against the loop it replaces - hnb_effect_sample once per instance, existing code - the sides
alternating window by window in ONE process on ONE device, for three shapes: c4's own (512 instances x 65,536 slots of examples/instancing.rs), many
small instances (4,096 x 1,024) and one large one (1 x 16,777,216), each a burst of the whole capacity after `--frames` frames of 1/60 s; a grid of
8^3 cells around the cloud of instance 0 (a box 2 % wider), every instance reading a field of its own; NEAREST and TRILINEAR; one channel (added
into VELOCITY.y) and four (VELOCITY.xyz and LIFETIME, whose channel of the field is zero); with and without stats:

    loop             hnb_effect_sample per instance, out_stats = the instance's row of a [n, 4] tensor (the descriptions are built once, outside the
                     windows: a window times the library calls and a ctypes call each, not the binding's conveniences)
    loop_nostats     the same with out_stats NULL
    program          hnb_program_sample with out_stats and out_instance_stats
    program_nostats  hnb_program_sample with both NULL

A window is `--reps` calls (of the whole loop, for the loop) between two synchronisations, timed on the host. Reported: median / min / max ms per
call and the spread of the baseline's own windows (max / min - 1): the program form is said to be faster - or, for one instance, not slower - only
beyond that spread. Before any time is taken both sides run from the same saved planes and the records of hnb_program_export (VELOCITY, LIFETIME)
and the stats rows are compared bit for bit. Kernel times need a run of their own:
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sample_program_ab.py --only program,program_nostats --windows 2 --reps 3`.

    python tools/sample_program_ab.py --log profiles/sample_program_ab.log
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
SCALE = 0.01
G = 8
SHAPES = {"c4": (512, 65536), "small": (4096, 1024), "one": (1, 1 << 24)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,small,one")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--reps", type=int, default=0, help="calls per window; 0: 10 for one instance, 3 otherwise")
    ap.add_argument("--only", default="", help="comma-separated sides to time (loop, loop_nostats, program, program_nostats)")
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects, runtime
    from export_ab import frame_seed
    from export_sorted_ab import windows
    A = bh.Attribute
    lib = runtime.load_library()
    lines = [f"sample_program_ab: {args.windows} windows per side, alternating; grid {G}^3, a field per instance; device {torch.cuda.get_device_name(0)}"]
    ok_all = True
    for shape in args.shapes.split(","):
        n, cap = SHAPES[shape]
        reps = args.reps or (10 if n == 1 else 3)
        ctx = bh.Context(0)
        prog = ctx.create_program(bh.lower(effects.instancing(cap) if shape == "c4" else effects.firework_trails(cap)))
        fxs = [prog.create_effect() for _ in range(n)]
        for f in range(args.frames):
            ctx.frame_begin(0.0 if f == 0 else 1 / 60, f / 60)
            for k, fx in enumerate(fxs):
                fx.set_frame(cap if f == 0 else 0, frame_seed(f * 16 + k))
            ctx.simulate()
        ctx.synchronize()
        alive = sum(fx.alive_count() for fx in fxs[:: max(1, n // 8)])
        pos = fxs[0].read_attr(A.POSITION.id).reshape(-1, 3).astype(np.float64)
        lo, hi = pos.min(axis=0), pos.max(axis=0)
        size = np.maximum(hi - lo, 1e-3)
        origin = (lo - 0.01 * size).astype(np.float32)
        inv_cell = (G / (1.02 * size)).astype(np.float32)
        lines.append(f"shape {shape}: {n} instances x {cap} slots, burst after {args.frames} frames of 1/60 s; alive in every 8th-of-the-program instance sampled: {alive}; "
                     f"{reps} calls per window")
        saved = [{a: fx.read_attr(a) for a in (A.VELOCITY.id, A.LIFETIME.id)} for fx in fxs]      # both sides start from these planes

        def restore():
            for fx, s in zip(fxs, saved):
                for a, v in s.items():
                    fx.write_attr(a, v)

        total = n * cap
        rec = torch.zeros((total, 4), dtype=torch.int32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        exported = [(A.VELOCITY.id, 0), (A.LIFETIME.id, 12)]
        for k in (1, 4):
            n_cells = G ** 3
            stride = n_cells * k
            field = torch.randn((n, n_cells, k), generator=torch.Generator(device="cuda").manual_seed(10 * n + k), device="cuda") * 30.0
            if k == 4:
                field[:, :, 3] = 0.0                                     # LIFETIME + 0 * scale: the lifetimes stay what they are
            ch = [(A.VELOCITY.id, 1, runtime.SAMPLE_ADD)] if k == 1 else [(A.VELOCITY.id, c, runtime.SAMPLE_ADD) for c in range(3)] + [(A.LIFETIME.id, 0, runtime.SAMPLE_ADD)]
            rows_loop = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
            rows_prog = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
            totals = torch.zeros(4, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for mode, mode_name in ((runtime.SAMPLE_NEAREST, "nearest"), (runtime.SAMPLE_TRILINEAR, "trilinear")):
                descs = [runtime.sample_desc((G, G, G), origin, inv_cell, field.data_ptr() + 4 * i * stride, ch, mode, SCALE, rows_loop.data_ptr() + 16 * i) for i in range(n)]
                descs_ns = [runtime.sample_desc((G, G, G), origin, inv_cell, field.data_ptr() + 4 * i * stride, ch, mode, SCALE, None) for i in range(n)]
                pd = runtime.program_sample_desc((G, G, G), origin, inv_cell, field.data_ptr(), ch, mode, SCALE, totals.data_ptr(), stride, rows_prog.data_ptr())
                pd_ns = runtime.program_sample_desc((G, G, G), origin, inv_cell, field.data_ptr(), ch, mode, SCALE, None, stride, None)
                handles = [fx._h for fx in fxs]

                def loop(ds=descs):
                    for h, d in zip(handles, ds):
                        if lib.hnb_effect_sample(h, C.byref(d)) != 0:
                            raise RuntimeError(lib.hnb_last_error())

                def program(d=pd):
                    if lib.hnb_program_sample(prog._h, C.byref(d)) != 0:
                        raise RuntimeError(lib.hnb_last_error())

                # ---- the result, on the device, before any time is taken: both sides from the saved planes
                restore()
                loop()
                prog.export(exported, rec.data_ptr(), 16, total, cnt.data_ptr())
                ctx.synchronize()
                got = rec.clone()
                restore()
                program()
                prog.export(exported, rec.data_ptr(), 16, total, cnt.data_ptr())
                ctx.synchronize()
                n_rec = int(cnt.cpu()[0])
                ok = bool((got[:n_rec] == rec[:n_rec]).all()) and bool((rows_loop == rows_prog).all()) and bool((rows_prog.sum(dim=0, dtype=torch.int64).to(torch.int32) == totals).all())
                ok_all = ok_all and ok
                st = totals.cpu().tolist()
                lines.append(f"  {k} channel(s), {mode_name}: program == loop, records and stats rows bit for bit on the device: {ok}; records {n_rec}, visited {st[0]}, sampled {st[1]}, outside {st[2]}")
                if not ok:
                    continue
                restore()
                sides = {"loop": loop, "loop_nostats": lambda: loop(descs_ns), "program": program, "program_nostats": lambda: program(pd_ns)}
                if args.only:
                    sides = {s: fn for s, fn in sides.items() if s in args.only.split(",")}
                ms = windows(sides, ctx.synchronize, args.windows, reps)
                med = {s: statistics.median(x) for s, x in ms.items()}
                for s in sides:
                    lines.append(f"    {s:16s} {med[s]:9.4f} ms (min {min(ms[s]):.4f}, max {max(ms[s]):.4f})")
                for a, b in (("loop", "program"), ("loop_nostats", "program_nostats")):
                    if a in sides and b in sides:
                        spread = max(ms[a]) / min(ms[a]) - 1
                        if med[b] * (1 + spread) < med[a]:
                            verdict = "the program form is faster beyond it"
                        elif med[b] <= med[a] * (1 + spread):
                            verdict = "the program form is not slower beyond it"
                        else:
                            verdict = "THE PROGRAM FORM IS SLOWER BEYOND IT"
                        lines.append(f"    {a} / {b} = {med[a] / med[b]:.2f}; spread of the loop's own windows {spread * 100:.1f} %: {verdict}")
                for a, b in (("program", "program_nostats"), ("loop", "loop_nostats")):
                    if a in sides and b in sides:
                        lines.append(f"    stats cost: {a} - {b} = {med[a] - med[b]:+.4f} ms ({med[a] / med[b]:.2f} x)")
                print("\n".join(lines[-8:]), flush=True)
        del saved, rec, fxs, prog
        ctx.close()
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
