#!/usr/bin/env python3
"""hnb_effect_pairs against the closest thing the library offered before it: hnb_effect_neighbours with one HNB_SPLAT_ATTR_ONE / W_ONE count channel on
the same state - the same sort and one walk, with no list (DESIGN.md "Neighbour pairs / Measured"). The three states of tools/neighbours_ab.py:
1,048,576 and 16,777,216 particles uniform in a cube over a grid of about 4 particles per cell with radius = the cell edge, and the c2 burst state
after 30 frames over a grid of 8 times as many particles per cell with candidate_limit 4096. Per configuration one JSON line: the median of `--reps`
calls, wall-clock between two synchronisations, of the full and the HALF list with and without out_d2 and of a count-only call (pair_capacity 0);
the count call of hnb_effect_neighbours beside them; the ratios; the pairs and the bytes written per pair. The yardstick is timed twice, in
front of and behind the pairs calls; `neighbours_count_ms` is the LOWER of the two medians (the choice that favours the yardstick) and both
series are logged. The split by kernel is read from a profiler's kernel trace of this script (`--only` picks one configuration).

    python tools/pairs_ab.py [--reps 5] [--only uniform_1m|uniform_16m|burst]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bevy_hanabi_amd as bh                      # noqa: E402
from bevy_hanabi_amd import effects, runtime      # noqa: E402
from neighbours_ab import F32, timed              # noqa: E402


def run(name, cap, frames, uniform, per_cell, limit, reps):
    A = bh.Attribute
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    for f in range(frames):
        dt = 1 / 600 if f == 0 else 1 / 60
        ctx.frame_begin(dt, f * dt)
        fx.set_frame(cap if f == 0 else 0, 0x9E3779B9 * (f + 1) & 0xFFFFFFFF)
        ctx.simulate()
    ctx.synchronize()
    side = max(1, round((cap / per_cell) ** (1 / 3)))
    if uniform:
        fx.write_attr(A.POSITION.id, np.random.default_rng(1).random((cap, 3), dtype=F32))
        dims, origin, inv_cell = (side,) * 3, (0.0,) * 3, (float(side),) * 3
    else:
        p = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fx.alive_list()].astype(np.float64)
        lo, hi = p.min(axis=0), p.max(axis=0)
        dims, origin = (side,) * 3, tuple(lo - 0.01 * (hi - lo))
        inv_cell = tuple(side / (1.02 * (hi - lo)))
    radius = float(F32(0.9999 / max(inv_cell)))
    rows = torch.empty(cap, dtype=torch.int32, device="cuda")
    start = torch.empty(cap + 1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(8, dtype=torch.int32, device="cuda")
    nstats = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    grid = (dims, origin, inv_cell, radius)
    totals = {}
    for half in (False, True):                   # count only first: the true totals size the destinations
        fx.pairs(*grid, rows.data_ptr(), start.data_ptr(), stats_ptr=stats.data_ptr(), candidate_limit=limit, half=half)
        ctx.synchronize()
        s = stats.cpu().numpy().view(np.uint32)
        totals[half] = int(s[4]) | int(s[5]) << 32
    assert totals[False] < 1 << 32, totals
    pairs = torch.empty(totals[False], dtype=torch.int32, device="cuda")
    d2 = torch.empty(totals[False], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    count = lambda: fx.neighbours(dims, origin, inv_cell, radius, [(runtime.SPLAT_ATTR_ONE, 0, 0, 0, A.VELOCITY.id, 0, runtime.SAMPLE_SET)], runtime.NEIGHBOUR_W_ONE, limit, 1.0,
                                  nstats.data_ptr())
    call = lambda half, with_d2, pc: lambda: fx.pairs(*grid, rows.data_ptr(), start.data_ptr(), pairs.data_ptr() if pc else None, pc, d2.data_ptr() if with_d2 and pc else None,
                                                      stats.data_ptr(), limit, half)
    t_count, all_count = timed(ctx, count, reps)
    ms = {}
    for key, half, with_d2 in (("full", False, False), ("full_d2", False, True), ("half", True, False), ("half_d2", True, True)):
        ms[key], _ = timed(ctx, call(half, with_d2, totals[half]), reps)
        s = stats.cpu().numpy().view(np.uint32)
        assert (int(s[4]) | int(s[5]) << 32, int(s[6])) == (totals[half], totals[half]), (key, s)
    ms["count_only"], _ = timed(ctx, call(False, False, 0), reps)
    t_count2, all_count2 = timed(ctx, count, reps)   # interleaved: the yardstick again behind the calls
    t_count = min(t_count, t_count2)              # the lower median: the comparison that favours the yardstick
    ns = nstats.cpu().numpy().view(np.uint32)
    assert (int(s[0]), int(s[3])) == (int(ns[0]), int(ns[3])) and int(s[1]) == int(ns[1]) + int(ns[3]), (s, ns)
    table_bytes = 4 * cap + 4 * (cap + 1)
    print(json.dumps(dict(config=name, particles=int(s[0]), inside=int(s[1]), crowded=int(s[3]), dims=dims, radius=radius, candidate_limit=limit, pairs_full=totals[False],
                          pairs_half=totals[True], pairs_per_inside=round(totals[False] / max(1, int(s[1])), 2), neighbours_count_ms=round(t_count, 4),
                          neighbours_count_ms_is="the lower of the medians of the two series below",
                          neighbours_count_ms_before=[round(x, 4) for x in all_count], neighbours_count_ms_after=[round(x, 4) for x in all_count2], pairs_ms={k: round(v, 4) for k, v in ms.items()},
                          ratio_to_neighbours_count={k: round(v / t_count, 3) for k, v in ms.items()},
                          bytes_written_per_pair=dict(full=round(4 + table_bytes / max(1, totals[False]), 3), full_d2=round(8 + table_bytes / max(1, totals[False]), 3),
                                                      half=round(4 + table_bytes / max(1, totals[True]), 3), half_d2=round(8 + table_bytes / max(1, totals[True]), 3)))), flush=True)
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
