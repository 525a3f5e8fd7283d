#!/usr/bin/env python3
"""hnb_effect_neighbours against the only thing the library offered for the job before it: hnb_effect_export_binned of POSITION (the caller's own walk
would come on top). Same box, same state, interleaved repetitions (DESIGN.md "Neighbours / Measured"). Three configurations: 1,048,576 and
16,777,216 particles uniform in a cube over a grid of about 4 particles per cell with radius = the cell edge (about 100 candidates per query), and the
c2 burst state after 30 frames over a grid of 8 times as many particles per cell with candidate_limit 4096. Per configuration one JSON line: the call's time, the export's time on
the same state, the pairs tested (from the cells, on the host), pairs per second and the snapshot bytes read per pair tested. Wall-clock between two
synchronisations over `--reps` calls; the split by kernel is read from a profiler's kernel trace of this script (`--only` picks one configuration).

    python tools/neighbours_ab.py [--reps 5] [--only uniform_1m|uniform_16m|burst]
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


def cells_of(pos, dims, origin, inv_cell):
    """the header's cell function in numpy binary32 -> ([n] int64 cells, n_cells for the outside bin)"""
    inside = np.ones(len(pos), bool)
    idx = []
    for c in range(3):
        t = (pos[:, c] - F32(origin[c])) * F32(inv_cell[c])
        ok = (t >= 0) & (t < F32(dims[c]))
        idx.append(np.where(ok, t, 0).astype(np.int64))
        inside &= ok
    cell = (idx[2] * dims[1] + idx[1]) * dims[0] + idx[0]
    return np.where(inside, cell, dims[0] * dims[1] * dims[2])


def pairs_tested(pos, dims, origin, inv_cell, limit):
    """sum over the gathered queries of candidates - 1, and the gathered and crowded counts"""
    n_cells = dims[0] * dims[1] * dims[2]
    cells = cells_of(pos, dims, origin, inv_cell)
    ins = cells[cells != n_cells]
    box = np.zeros((dims[2] + 2, dims[1] + 2, dims[0] + 2), np.int64)
    box[1:-1, 1:-1, 1:-1] = np.bincount(ins, minlength=n_cells).reshape(dims[2], dims[1], dims[0])
    tot = sum(box[z: z + dims[2], y: y + dims[1], x: x + dims[0]] for z in range(3) for y in range(3) for x in range(3)).reshape(-1)
    cand = tot[ins]
    g = cand <= limit
    return int((cand[g] - 1).sum()), int(g.sum()), int((~g).sum())


def timed(ctx, fn, reps):
    fn(); fn()
    ctx.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), out


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
    if uniform:
        rng = np.random.default_rng(1)
        fx.write_attr(A.POSITION.id, rng.random((cap, 3), dtype=F32))
        side = max(1, round((cap / per_cell) ** (1 / 3)))
        dims, origin, inv_cell = (side,) * 3, (0.0,) * 3, (float(side),) * 3
    else:
        p = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fx.alive_list()].astype(np.float64)
        lo, hi = p.min(axis=0), p.max(axis=0)
        side = max(1, round((cap / per_cell) ** (1 / 3)))
        dims, origin = (side,) * 3, tuple(lo - 0.01 * (hi - lo))
        inv_cell = tuple(side / (1.02 * (hi - lo)))
    radius = float(F32(0.9999 / max(inv_cell)))
    pos = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fx.alive_list()]
    pairs, gathered, crowded = pairs_tested(pos, dims, np.asarray(origin, F32), np.asarray(inv_cell, F32), limit)
    n_cells = dims[0] * dims[1] * dims[2]
    dst = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    table = torch.zeros(n_cells + 2, dtype=torch.int32, device="cuda")
    stats = torch.zeros(8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ch = [(runtime.SPLAT_ATTR_ONE, 0, 0, 0, A.VELOCITY.id, 0, runtime.SAMPLE_SET), (runtime.SPLAT_ATTR_ONE, 0, 0, 30, A.VELOCITY.id, 1, runtime.SAMPLE_SET),
          (A.POSITION.id, 0, runtime.NEIGHBOUR_DIFF, 16, A.VELOCITY.id, 2, runtime.SAMPLE_SET)]
    call = lambda: fx.neighbours(dims, origin, inv_cell, radius, ch, runtime.NEIGHBOUR_W_U3, limit, 1.0, stats.data_ptr())
    export = lambda: fx.export_binned([(A.POSITION.id, 0)], dst.data_ptr(), 16, cap, cnt.data_ptr(), dims=dims, origin=origin, inv_cell=inv_cell, cell_start_ptr=table.data_ptr())
    t_call, all_call = timed(ctx, call, reps)
    t_exp, all_exp = timed(ctx, export, reps)
    t_call2, _ = timed(ctx, call, reps)                 # interleaved: the call again behind the export
    s = stats.cpu().numpy().view(np.uint32)
    assert int(s[1]) == gathered and int(s[3]) == crowded, (s, gathered, crowded)
    src_channels = 1                                   # snapshot bytes per candidate record: 16, plus 4 per source plane read for a neighbour
    print(json.dumps(dict(config=name, particles=int(s[0]), dims=dims, radius=radius, candidate_limit=limit, gathered=gathered, crowded=crowded, pairs_tested=pairs,
                          call_ms=round(min(t_call, t_call2), 4), call_ms_all=[round(x, 4) for x in all_call], export_binned_ms=round(t_exp, 4),
                          export_ms_all=[round(x, 4) for x in all_exp], pairs_per_s=round(pairs / (min(t_call, t_call2) * 1e-3), 1),
                          snapshot_bytes_per_pair=16, source_bytes_per_neighbour=4 * src_channels)), flush=True)
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
