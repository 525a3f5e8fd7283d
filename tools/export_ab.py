#!/usr/bin/env python3
"""A/B of the packed export (hnb_effect_export: k_export_rows) against the stand-in consumer that reads through the device view
(tests/device_view/consumer.hip: k_render_like), on one effect of 16,777,216 firework particles in two states:

    burst   c2: the burst and 5 frames - the list is the identity, every slot alive
    churn   c2_mixed: a rate spawner of capacity / mean lifetime per second, 240 frames at 1/60 s - mixed ages, spawns into recycled slots, a
            permuted list (HNB_LIST_ORDER_SPAWN)

Both gather POSITION, AGE and LIFETIME by list row. The export writes records of 32 bytes {POSITION @0, AGE @12, LIFETIME @16, 12 bytes of zeroed
padding}: list 4 + planes 20 bytes read, 32 written per record = 56; the consumer writes a float4 (position, age / lifetime): 4 + 20 read, 16
written = 40. The two alternate, window by window, in ONE process on ONE device (the pool's box-to-box spread is 3 - 15 %: only same-box pairs
count); a window is `--reps` launches between two hnb_ctx_synchronize, timed on the host (>= 2 ms: the synchronisation's 10 us are < 1 %).
Reported per state and side: median / min / max ms per launch over the windows, bytes per record, and the fraction of 8 TB/s those bytes are.
`--only export|consumer` runs one side alone (`--windows 1 --reps 4`: a counter pass, rocprofv3 --pmc FETCH_SIZE or WRITE_SIZE, no tracing).

    python tools/export_ab.py --windows 10 --reps 20 --log profiles/export_ab.log
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8e12
MEAN_LIFETIME = 1.0


def frame_seed(f):
    import oracle
    return oracle.pcg_hash(0xC0FFEE + f)


def prepare(state, cap):
    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects
    ctx = bh.Context(0)
    if state == "burst":
        asset = effects.firework_trails(cap)
        fx = ctx.create_program(bh.lower(asset)).create_effect()
        for f in range(6):
            ctx.frame_begin(1 / 600, f / 600)
            fx.set_frame(cap if f == 0 else 0, frame_seed(f))
            ctx.simulate()
    else:
        asset = effects.firework_trails(cap, bh.SpawnerSettings.rate(float(cap) / MEAN_LIFETIME))
        fx = ctx.create_program(bh.lower(asset)).create_effect()
        sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
        for f in range(240):
            ctx.frame_begin(1 / 60, f / 60)
            fx.set_frame(sp.tick(1 / 60, rng), frame_seed(f))
            ctx.simulate()
    ctx.synchronize()
    return ctx, fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--states", default="burst,churn")
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="", choices=["", "export", "consumer"])
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import runtime
    A = bh.Attribute
    cons = C.CDLL(os.path.join(ROOT, "tests", "device_view", "libconsumer.so"))
    cons.consumer_render_like.argtypes = [C.POINTER(runtime.DeviceView), C.c_void_p]
    fields = [(A.POSITION.id, 0), (A.AGE.id, 12), (A.LIFETIME.id, 16)]
    lines = [f"export_ab: capacity {args.capacity}, {args.windows} windows x {args.reps} launches per side, alternating; device {torch.cuda.get_device_name(0)}"]
    for state in args.states.split(","):
        ctx, fx = prepare(state, args.capacity)
        alive = fx.alive_count()
        dst = torch.zeros(args.capacity * 8, dtype=torch.int32, device="cuda")        # 32-byte records
        out4 = torch.zeros(args.capacity * 4, dtype=torch.float32, device="cuda")     # the consumer's float4 per row
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        view = fx.device_view()
        stale = view.stale_attr_mask
        sides = {"export": lambda: fx.export(fields, dst.data_ptr(), 32, args.capacity, cnt.data_ptr()),
                 "consumer": lambda: cons.consumer_render_like(C.byref(view), out4.data_ptr())}
        if args.only:
            sides = {args.only: sides[args.only]}
        ms = {k: [] for k in sides}
        for k, fn in sides.items():       # warm-up: module load, TLBs
            fn()
        ctx.synchronize()
        for _ in range(args.windows):
            for k, fn in sides.items():
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                ctx.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / args.reps)
        assert [int(x) for x in cnt.cpu()] == [alive, alive] or args.only == "consumer"
        lines.append(f"state {state}: alive {alive} of {args.capacity}, stale_attr_mask {stale:#x}, update kernel {fx._prog.kernel_info().splitlines()[0]}")
        for k, per in (("export", 56), ("consumer", 40)):
            if k not in ms:
                continue
            med = statistics.median(ms[k])
            lines.append(f"  {k:8s} {med:.4f} ms (min {min(ms[k]):.4f}, max {max(ms[k]):.4f}); {per} B per record = {alive * per / 1e6:.0f} MB -> "
                         f"{alive * per / (med * 1e-3) / 1e12:.2f} TB/s = {alive * per / (med * 1e-3) / PEAK:.2f} of 8 TB/s")
        if len(ms) == 2:
            e, c = statistics.median(ms["export"]), statistics.median(ms["consumer"])
            spread = max(max(v) / min(v) - 1 for v in ms.values())
            lines.append(f"  export / consumer = {e / c:.3f} (same-box spread of the windows: {spread * 100:.1f} %)")
        ctx.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
