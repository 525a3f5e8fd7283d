#!/usr/bin/env python3
"""hnb_effect_neighbours_from between two effects against the parent's closest offer: hnb_effect_neighbours on the source alone with the same three
channels - one sort, one snapshot and one walk over the same candidate density (DESIGN.md "Neighbours across effects / Measured"). Same box, same
state. Three configurations, query and source of the same size: 1,048,576 and 16,777,216 particles each, uniform in one cube over a grid of about 4
sources per cell with radius = the cell edge, and two c2 bursts after 30 frames over a grid of 8 times as many per cell with candidate_limit 4096.
The yardstick is timed in front of and behind the new calls; the LOWER of its two medians is quoted and both series are logged. Expected on top of
the yardstick: one more sort of cell keys and one scattered 12-byte read per query; there is no snapshot of the queries. Per configuration one JSON
line. Wall-clock between two synchronisations over `--reps` calls.

    python tools/neighbours_from_ab.py [--reps 5] [--only uniform_1m|uniform_16m|burst]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bevy_hanabi_amd as bh                      # noqa: E402
from bevy_hanabi_amd import effects, runtime      # noqa: E402

F32 = np.float32


def timed(ctx, fn, reps):
    fn(); fn()
    ctx.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), [round(x, 4) for x in out]


def run(name, cap, frames, uniform, per_cell, limit, reps):
    A = bh.Attribute
    ctx = bh.Context(0)
    fq = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    fs = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    for f in range(frames):
        dt = 1 / 600 if f == 0 else 1 / 60
        ctx.frame_begin(dt, f * dt)
        fq.set_frame(cap if f == 0 else 0, 0x9E3779B9 * (f + 1) & 0xFFFFFFFF)
        fs.set_frame(cap if f == 0 else 0, 0x85EBCA6B * (f + 1) & 0xFFFFFFFF)
        ctx.simulate()
    ctx.synchronize()
    side = max(1, round((cap / per_cell) ** (1 / 3)))
    if uniform:
        fq.write_attr(A.POSITION.id, np.random.default_rng(1).random((cap, 3), dtype=F32))
        fs.write_attr(A.POSITION.id, np.random.default_rng(2).random((cap, 3), dtype=F32))
        dims, origin, inv_cell = (side,) * 3, (0.0,) * 3, (float(side),) * 3
    else:
        p = fs.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fs.alive_list()].astype(np.float64)
        lo, hi = p.min(axis=0), p.max(axis=0)
        dims, origin = (side,) * 3, tuple(lo - 0.01 * (hi - lo))
        inv_cell = tuple(side / (1.02 * (hi - lo)))
    radius = float(F32(0.9999 / max(inv_cell)))
    stats = torch.zeros(8, dtype=torch.int32, device="cuda")
    own = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ch = [(runtime.SPLAT_ATTR_ONE, 0, 0, 0, A.VELOCITY.id, 0, runtime.SAMPLE_SET), (runtime.SPLAT_ATTR_ONE, 0, 0, 30, A.VELOCITY.id, 1, runtime.SAMPLE_SET),
          (A.POSITION.id, 0, runtime.NEIGHBOUR_DIFF, 16, A.VELOCITY.id, 2, runtime.SAMPLE_SET)]
    call = lambda: fq.neighbours_from(fs, dims, origin, inv_cell, radius, ch, runtime.NEIGHBOUR_W_U3, limit, 1.0, stats.data_ptr())
    yard = lambda: fs.neighbours(dims, origin, inv_cell, radius, ch, runtime.NEIGHBOUR_W_U3, limit, 1.0, own.data_ptr())
    t_y1, all_y1 = timed(ctx, yard, reps)
    t_call, all_call = timed(ctx, call, reps)
    t_y2, all_y2 = timed(ctx, yard, reps)
    s, o = stats.cpu().numpy().view(np.uint32), own.cpu().numpy().view(np.uint32)
    t_yard = min(t_y1, t_y2)
    print(json.dumps(dict(config=name, queries=int(s[0]), gathered=int(s[1]), outside=int(s[2]), crowded=int(s[3]), inside_sources=int(s[5]), sources=int(s[6]), dims=dims, radius=radius,
                          candidate_limit=limit,
                          neighbours_from_ms=round(t_call, 4), neighbours_from_ms_all=all_call, neighbours_source_alone_ms=round(t_yard, 4), neighbours_source_alone_ms_before=all_y1,
                          neighbours_source_alone_ms_after=all_y2, source_alone_gathered=int(o[1]), source_alone_crowded=int(o[3]), ratio=round(t_call / t_yard, 3))), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    configs = [("uniform_1m", 1 << 20, 1, True, 4, 4096), ("uniform_16m", 1 << 24, 1, True, 4, 4096), ("burst", 1 << 20, 30, False, 4 * 8, 4096)]
    for name, cap, frames, uniform, per_cell, limit in configs:
        if a.only in (None, name):
            run(name, cap, frames, uniform, per_cell, limit, a.reps)


if __name__ == "__main__":
    main()
