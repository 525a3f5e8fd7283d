#!/usr/bin/env python3
"""A/B of the binned export (hnb_effect_export_binned, a 64 x 64 x 64 grid around the cloud) against the sorted export (hnb_effect_export_sorted, key
DEPTH) on one effect of 16,777,216 firework particles in the burst state of tools/export_ab.py (identity list, everything alive), the sides
alternating window by window in ONE process on ONE device:

    sorted    hnb_effect_export_sorted of {POSITION @0, AGE @12, LIFETIME @16} at stride 32, depth along (0.3, -0.5, 0.8): four digit passes
    binned    hnb_effect_export_binned of the same records: the cells of 64^3 = 262,144 cells and the outside key are below 2^19, so the highest
              digit pass leaves at its first scalar load; behind the sort k_export_bin_starts writes the 262,146 words of the table
    sortonly / binonly   the same two calls into a destination of 0 records: every gather workgroup leaves after its scalar loads, so the call is
              the key, sort and (binned) table stages alone

A window is `--reps` calls between two synchronisations, timed on the host. Reported: median / min / max ms per call, the spread of the sorted
side's own windows (max / min - 1: what the same call on the same box varies by), the digit passes the binned call's keys make run, and whether
binned <= sorted * (1 + that spread). The binned side's output is checked on the device first: the records' cells, recomputed in torch binary32,
never decrease, and the table is their searchsorted. The share of k_export_bin_starts needs kernel times: run the tool under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/export_binned_ab.py --only binned --windows 2 --reps 5` in a run of
its own and read the kernel statistics it writes.

    python tools/export_binned_ab.py --windows 10 --reps 20 --log profiles/export_binned_ab.log
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
DIR = (0.3, -0.5, 0.8)
DIMS = (64, 64, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="", help="comma-separated sides to run (sorted, binned, sortonly, binonly)")
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    import bevy_hanabi_amd as bh
    from export_ab import prepare
    from export_sorted_ab import windows
    A = bh.Attribute
    fields = [(A.POSITION.id, 0), (A.AGE.id, 12), (A.LIFETIME.id, 16)]
    cap = args.capacity
    lines = [f"export_binned_ab: capacity {cap}, grid {DIMS[0]} x {DIMS[1]} x {DIMS[2]}, {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
    ctx, fx = prepare("burst", cap)
    alive = fx.alive_count()
    n_cells = DIMS[0] * DIMS[1] * DIMS[2]
    dst = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    dst2 = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    table = torch.zeros(n_cells + 2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                                             # (the fills run on torch's stream, the exports on the simulation's)
    fx.export(fields, dst.data_ptr(), 32, cap, cnt.data_ptr())            # the box of the cloud, from the plain export's records
    ctx.synchronize()
    p = dst[:alive, 0:3].view(torch.float32)
    lo, hi = p.min(dim=0).values.double(), p.max(dim=0).values.double()
    size = torch.clamp(hi - lo, min=1e-3)
    origin = (lo - 0.01 * size).float().cpu().numpy()
    inv_cell = (torch.tensor(DIMS, dtype=torch.float64, device="cuda") / (1.02 * size)).float().cpu().numpy()
    grid = dict(dims=DIMS, origin=origin, inv_cell=inv_cell, cell_start_ptr=table.data_ptr())

    def cells_of(pos):                                                   # the header's formulas in torch binary32, operation by operation
        o, iv = torch.tensor(origin, device="cuda"), torch.tensor(inv_cell, device="cuda")
        t = (pos - o) * iv
        inside = ((t >= 0) & (t < torch.tensor(DIMS, dtype=torch.float32, device="cuda"))).all(dim=1)
        i = torch.where(inside[:, None], t, torch.zeros_like(t)).to(torch.int64)
        return torch.where(inside, (i[:, 2] * DIMS[1] + i[:, 1]) * DIMS[0] + i[:, 0], torch.full_like(i[:, 0], n_cells))

    sides = {"sorted": lambda: fx.export_sorted(fields, dst.data_ptr(), 32, cap, cnt.data_ptr(), key="depth", v=DIR),
             "binned": lambda: fx.export_binned(fields, dst2.data_ptr(), 32, cap, cnt.data_ptr(), **grid),
             "sortonly": lambda: fx.export_sorted(fields, dst.data_ptr(), 32, 0, None, key="depth", v=DIR),
             "binonly": lambda: fx.export_binned(fields, dst2.data_ptr(), 32, 0, None, **grid)}
    if args.only:
        sides = {k: sides[k] for k in args.only.split(",")}
    lines.append(f"state burst: alive {alive} of {cap}; origin {[float(x) for x in origin]}, inv_cell {[float(x) for x in inv_cell]}")
    if "binned" in sides:
        sides["binned"]()
        ctx.synchronize()
        cells = cells_of(dst2[:alive, 0:3].view(torch.float32))
        want = torch.searchsorted(cells, torch.arange(n_cells + 2, device="cuda"), right=False)
        ok = bool((cells[1:] >= cells[:-1]).all()) and bool((table.to(torch.int64) == want).all()) and [int(x) for x in cnt.cpu()] == [alive, alive]
        present = cells.unique()
        varying = int(np.bitwise_or.reduce(present.cpu().numpy().astype(np.uint32))) & int(np.bitwise_or.reduce(~present.cpu().numpy().astype(np.uint32)))
        passes = [b for b in range(4) if (varying >> (8 * b)) & 0xFF]
        lines.append(f"  binned output checked on the device (cells never decrease, table = searchsorted, counts): {ok}")
        lines.append(f"  occupied cells {len(present)} of {n_cells}, outside {int((cells == n_cells).sum())}; digit passes that run: {passes} ({len(passes)} of 4; the sorted side's depth keys run all 4)")
        if not ok:
            print("\n".join(lines), flush=True)
            return 1
    ms = windows(sides, ctx.synchronize, args.windows, args.reps)
    for k in sides:
        lines.append(f"  {k:8s} {statistics.median(ms[k]):.4f} ms (min {min(ms[k]):.4f}, max {max(ms[k]):.4f})")
    med = {k: statistics.median(x) for k, x in ms.items()}
    if "sorted" in med and "binned" in med:
        spread = max(ms["sorted"]) / min(ms["sorted"]) - 1
        verdict = "not slower" if med["binned"] <= med["sorted"] * (1 + spread) else "SLOWER"
        lines.append(f"  binned / sorted = {med['binned'] / med['sorted']:.3f}; spread of the sorted side's own windows {spread * 100:.1f} %: binned is {verdict} beyond it")
    if "sortonly" in med and "binonly" in med:
        lines.append(f"  without the gather: binonly / sortonly = {med['binonly'] / med['sortonly']:.3f}")
    ctx.close()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
