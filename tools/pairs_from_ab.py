#!/usr/bin/env python3
"""hnb_effect_pairs_from between two effects against the parent's closest offer: hnb_effect_pairs on the source alone with the same variants - one
sort, one snapshot, two walks over the same candidate density (DESIGN.md "Neighbour pairs across effects / Measured"). Same box, same state. The three
states of tools/neighbours_from_ab.py, query and source of the same size: 1,048,576 and 16,777,216 particles each, uniform in one cube over a grid of
about 4 sources per cell with radius = the cell edge, and two c2 bursts after 30 frames over a grid of 8 times as many per cell with candidate_limit
4096. Variants: count only (pair_capacity 0), full, full + out_d2; destinations sized from a count-only call, so nothing is truncated. The yardstick
is timed in front of and behind the new calls; the LOWER of its two medians is quoted and both series are logged. Expected on top of the yardstick:
one more sort of cell keys and two scattered 12-byte reads per query; there is no snapshot of the queries. Per configuration one JSON line. Wall-clock
between two synchronisations over `--reps` calls.

    python tools/pairs_from_ab.py [--reps 5] [--only uniform_1m|uniform_16m|burst]
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
from bevy_hanabi_amd import effects               # noqa: E402
from neighbours_from_ab import F32, timed         # noqa: E402

VARIANTS = (("count_only", False, False), ("full", True, False), ("full_d2", True, True))


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
    rows = torch.empty(cap, dtype=torch.int32, device="cuda")
    start = torch.empty(cap + 1, dtype=torch.int32, device="cuda")
    stats = torch.zeros(8, dtype=torch.int32, device="cuda")
    own = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    grid = (dims, origin, inv_cell, radius)

    def total_of(buf):
        s = buf.cpu().numpy().view(np.uint32)
        return int(s[4]) | int(s[5]) << 32

    # count only first: the true totals size the destinations, shared by the call and the yardstick
    fq.pairs_from(fs, *grid, rows.data_ptr(), start.data_ptr(), stats_ptr=stats.data_ptr(), candidate_limit=limit)
    fs.pairs(*grid, rows.data_ptr(), start.data_ptr(), stats_ptr=own.data_ptr(), candidate_limit=limit)
    ctx.synchronize()
    total, total_own = total_of(stats), total_of(own)
    assert max(total, total_own) < 1 << 32, (total, total_own)
    pairs = torch.empty(max(total, total_own), dtype=torch.int32, device="cuda")
    d2 = torch.empty(max(total, total_own), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    args = lambda listed, with_d2, pc: (rows.data_ptr(), start.data_ptr(), pairs.data_ptr() if listed else None, pc if listed else 0, d2.data_ptr() if listed and with_d2 else None)
    call = lambda listed, with_d2: lambda: fq.pairs_from(fs, *grid, *args(listed, with_d2, total), stats.data_ptr(), limit)
    yard = lambda listed, with_d2: lambda: fs.pairs(*grid, *args(listed, with_d2, total_own), own.data_ptr(), limit)
    before, ms, after, series = {}, {}, {}, {}
    for key, listed, with_d2 in VARIANTS:
        before[key], series[key + "_before"] = timed(ctx, yard(listed, with_d2), reps)
    for key, listed, with_d2 in VARIANTS:
        ms[key], series[key] = timed(ctx, call(listed, with_d2), reps)
        s = stats.cpu().numpy().view(np.uint32)
        assert (total_of(stats), int(s[6])) == (total, total if listed else 0), (key, s)
    for key, listed, with_d2 in VARIANTS:               # interleaved: the yardstick again behind the calls
        after[key], series[key + "_after"] = timed(ctx, yard(listed, with_d2), reps)
    yard_ms = {k: min(before[k], after[k]) for k in before}      # the lower median: the comparison that favours the yardstick
    o = own.cpu().numpy().view(np.uint32)
    table_bytes = 4 * cap + 4 * (cap + 1)
    print(json.dumps(dict(config=name, queries=int(s[0]), inside=int(s[1]), outside=int(s[2]), crowded=int(s[3]), inside_sources=int(s[7]), dims=dims, radius=radius,
                          candidate_limit=limit, pairs=total, pairs_per_inside=round(total / max(1, int(s[1])), 2), pairs_source_alone=total_own, source_alone_crowded=int(o[3]),
                          pairs_from_ms={k: round(v, 4) for k, v in ms.items()}, pairs_source_alone_ms={k: round(v, 4) for k, v in yard_ms.items()},
                          pairs_source_alone_ms_is="the lower of the medians of the _before and _after series", ratio={k: round(ms[k] / yard_ms[k], 3) for k in ms},
                          difference_ms={k: round(ms[k] - yard_ms[k], 4) for k in ms}, series=series,
                          bytes_written_per_pair=dict(full=round(4 + table_bytes / max(1, total), 3), full_d2=round(8 + table_bytes / max(1, total), 3)))), flush=True)
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
