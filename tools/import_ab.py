#!/usr/bin/env python3
"""A/B of the packed input (hnb_effect_import) against what a user could do on the device before it existed: torch indexed assignment into plane
tensors made from hnb_effect_device_view, indexed by the alive list or by the ids. That side resets none of the library's cached proofs, so it is
not even correct; it is the yardstick for the copy alone. 16,777,216 firework particles on one device, {POSITION @0, VELOCITY @16} at stride 32
(the ID, where there is one, in the uncovered dword at byte 12), both sides alternating window by window in ONE process:

    a  rows-burst   HNB_IMPORT_ROWS behind the burst: the list is nearly the identity
    b  rows-churn   HNB_IMPORT_ROWS in the steady spawn / death churn of tools/export_ab.py: a permuted list
    c  ids-sorted   HNB_IMPORT_IDS over the output of a DEPTH-sorted export of the burst: the slots are random

The records are the export of the state with y negated; the import's result is checked on the device first (the planes, gathered through the same
index, are the records' fields, and out_count). The torch side's index is converted to int64 ONCE, outside the timed windows: in its favour. A
window is `--reps` calls between two synchronisations (of the simulation stream and of torch's), timed on the host. Reported per row: median / min /
max ms per call, the spread of the torch side's own windows (max / min - 1), whether import <= torch * (1 + that spread), and the modelled bytes
per record (stride + the list word or the alive byte + 4 bytes per stored component) as achieved payload bandwidth - in rows b and c the 12-byte
stores are scattered and reach the fabric as 32-byte sectors (the write amplification VERDICT.md measured for the churn init), so the figure is no
fraction of peak. Last: what the resets cost the NEXT frame - the first frame behind an import (the chunks' lifetime bounds are rebuilt, the
lists are not skipped) against a frame behind a frame.

Two sides more, for the causes: in row b the import as one call per field (the torch side writes one plane per kernel), in row c the torch side with
a one-byte gather through the same index (the alive test the import makes and the torch side does not).

    python tools/import_ab.py --windows 10 --reps 50 --log profiles/import_ab.log
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
DIR = (0.3, -0.5, 0.8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=1 << 24)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="a,b,c")
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import runtime
    from bounds_ab import Raw
    from export_ab import frame_seed, prepare
    from export_sorted_ab import windows
    A = bh.Attribute
    cap = args.capacity
    rows_fields = [(A.POSITION.id, 0), (A.VELOCITY.id, 16)]
    ids_fields = rows_fields + [(A.ID.id, 12)]
    lines = [f"import_ab: capacity {cap}, {{POSITION, VELOCITY}} at stride 32, {args.windows} windows x {args.reps} calls per side, alternating; device {torch.cuda.get_device_name(0)}"]
    rec = torch.zeros((cap, 8), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    verdicts = []
    for row, name, state, mode in (("a", "rows-burst", "burst", runtime.IMPORT_ROWS), ("b", "rows-churn", "churn", runtime.IMPORT_ROWS), ("c", "ids-sorted", "burst", runtime.IMPORT_IDS)):
        if row not in args.rows.split(","):
            continue
        ctx, fx = prepare(state, cap)

        def sync():
            ctx.synchronize()
            torch.cuda.synchronize()

        alive = fx.alive_count()
        if mode == runtime.IMPORT_IDS:
            fx.export_sorted(ids_fields, rec.data_ptr(), 32, cap, cnt.data_ptr(), key="depth", v=DIR)
        else:
            fx.export(rows_fields, rec.data_ptr(), 32, cap, cnt.data_ptr())
        sync()
        rec[:alive, 1].view(torch.float32).neg_()                          # the consumer's change: y negated
        v = fx.device_view()
        plane = {a.attr: a.plane for a in v.attrs[: v.n_attrs]}
        pos_t = torch.as_tensor(Raw(plane[A.POSITION.id], (cap, 3), "<f4"), device="cuda")
        vel_t = torch.as_tensor(Raw(plane[A.VELOCITY.id], (cap, 3), "<f4"), device="cuda")
        meta = torch.as_tensor(Raw(v.meta, (8,), "<i4"), device="cuda").cpu().numpy().view("uint32")
        assert meta[0] == alive and meta[2] >> 1 == 0                     # (no ring list here: the list starts at row 0 of its column)
        list_t = torch.as_tensor(Raw(v.alive_list[int(meta[2]) & 1], (cap,), "<i4"), device="cuda")
        idx = (rec[:alive, 3] if mode == runtime.IMPORT_IDS else list_t[:alive]).long()      # converted once, outside the windows
        src_pos, src_vel = rec[:alive, 0:3].view(torch.float32), rec[:alive, 4:7].view(torch.float32)
        identity = float((idx == torch.arange(alive, device="cuda")).float().mean())
        sync()

        def do_import():
            fx.import_records(ids_fields if mode == runtime.IMPORT_IDS else rows_fields, rec.data_ptr(), 32, cap, mode, cnt.data_ptr(), out.data_ptr())

        def do_torch():
            pos_t[idx] = src_pos
            vel_t[idx] = src_vel

        do_import()
        sync()
        ok = (bool((pos_t[idx].view(torch.int32) == rec[:alive, 0:3]).all()) and bool((vel_t[idx].view(torch.int32) == rec[:alive, 4:7]).all())
              and [int(x) for x in out.cpu()] == [alive, 0])
        lines.append(f"row {row} {name}: alive {alive} of {cap}, rows whose slot is their row {identity * 100:.1f} %; import checked on the device (planes through the index = the records, out_count): {ok}")
        if not ok:
            print("\n".join(lines), flush=True)
            return 1
        sides = {"import": do_import, "torch": do_torch}
        if mode == runtime.IMPORT_IDS:                                    # what the import does more than the torch side: one alive byte per record, wherever its id points
            byte_t = torch.ones(cap, dtype=torch.uint8, device="cuda")    # (a stand-in of the same size: the views hand out no alive bytes)

            def do_torch_byte():
                do_torch()
                byte_t[idx]

            sides["torch+byte"] = do_torch_byte
        if row == "b":                                                    # the torch side is two kernels, a plane each: the same split of the import, the records read twice

            def do_import_split():
                for field in rows_fields:
                    fx.import_records([field], rec.data_ptr(), 32, cap, mode, cnt.data_ptr(), out.data_ptr())

            sides["import/field"] = do_import_split
        ms = windows(sides, sync, args.windows, args.reps)
        med = {k: statistics.median(x) for k, x in ms.items()}
        per = 32 + (1 if mode == runtime.IMPORT_IDS else 4) + 24
        for k in sides:
            lines.append(f"  {k:12s} {med[k]:.4f} ms (min {min(ms[k]):.4f}, max {max(ms[k]):.4f}); modelled {per} B per record = {alive * per / 1e6:.0f} MB -> {alive * per / (med[k] * 1e-3) / 1e12:.2f} TB/s of payload")
        spread = max(ms["torch"]) / min(ms["torch"]) - 1
        verdict = "not slower" if med["import"] <= med["torch"] * (1 + spread) else "SLOWER"
        verdicts.append(verdict)
        lines.append(f"  import / torch = {med['import'] / med['torch']:.3f}; spread of the torch side's own windows {spread * 100:.1f} %: the import is {verdict} beyond it")
        lines.append(f"  windows, ms: " + "; ".join(k + " " + " ".join(f"{x:.3f}" for x in ms[k]) for k in sides))
        if "import/field" in med:
            lines.append(f"  import/field / torch = {med['import/field'] / med['torch']:.3f} (one call per field, as the torch side writes one plane per kernel)")
        if "torch+byte" in med:
            lines.append(f"  import / torch+byte = {med['import'] / med['torch+byte']:.3f} (the torch side with a one-byte gather through the same index: the alive test's traffic)")
        if row == "a":                                                    # what the resets cost the next frame
            t = {"behind an import": [], "behind a frame": []}
            f = 6

            def frame():
                nonlocal f
                ctx.frame_begin(1 / 600, f / 600)
                fx.set_frame(0, frame_seed(f))
                ctx.simulate()
                f += 1

            for _ in range(3):
                frame()
            sync()
            for _ in range(args.windows):
                for k in t:
                    if k == "behind an import":
                        do_import()
                    else:
                        frame()
                    sync()
                    t0 = time.perf_counter()
                    frame()
                    sync()
                    t[k].append((time.perf_counter() - t0) * 1e3)
            lines.append("  the next frame: " + "; ".join(f"{k} {statistics.median(x):.4f} ms (min {min(x):.4f}, max {max(x):.4f})" for k, x in t.items()))
        ctx.close()
    lines.append("bar (the import no slower than the torch side beyond the torch side's own spread, in every row): " + ("met" if verdicts and all(v == "not slower" for v in verdicts) else "NOT met"))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.log:
        with open(args.log, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
