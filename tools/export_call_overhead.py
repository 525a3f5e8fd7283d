"""Host cost of one packed-export call, per form: hnb_effect_export, hnb_program_export, hnb_effect_export_sorted, hnb_program_export_sorted (both
scopes, and with an HnbExportSortFiltered), hnb_effect_export_filtered, hnb_program_export_filtered, hnb_effect_export_filtered_sorted - and of
hnb_program_bounds, which shares their loader -, each enqueued CALLS times between two synchronisations, WINDOWS times over.

One effect and a program of three instances, 4096 slots each, records of 32 bytes: every form is on its one-launch-per-stage path, where the time of a
call is the library's host path and the launches behind it, not the kernels. The descriptions are built once; the loop calls the C ABI directly.
Two figures per form, in microseconds per call, as median / min / max over the windows: `call`, from synchronisation to synchronisation, and
`enqueue`, until the last call returned.

    python tools/export_call_overhead.py [--label NAME] [--calls 2000] [--windows 10] [--alive 256]

HNB_LIB=<another build's libhanabi_amd.so> measures that build with the same script (runtime.load_library), in a fresh process."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this build", help="what the output calls the build")
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--alive", type=int, default=256, help="particles alive per instance")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch

    import bevy_hanabi_amd as bh
    from bevy_hanabi_amd import effects, runtime

    cap, stride = 4096, 32
    pos, age, life, vel = 2, 4, 5, 3                                    # attribute ids: POSITION, AGE, LIFETIME, VELOCITY
    fields = [(pos, 0), (age, 12), (life, 16), (vel, 20)]
    ctx = bh.Context(0)
    lib = ctx._lib
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    prog = ctx.create_program(bh.lower(effects.firework_trails(cap)))
    fxs = [prog.create_effect() for _ in range(3)]
    ctx.frame_begin(1 / 600, 0.0)
    for k, e in enumerate([fx] + fxs):
        e.set_frame(args.alive, 0x1234 + k)
    ctx.simulate()
    dst = torch.zeros((3 * cap * stride // 4,), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((2,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    d = runtime.export_desc(fields, dst.data_ptr(), stride, 3 * cap, cnt.data_ptr())
    s = runtime.export_sort("depth", (0.3, -0.5, 0.8), 0, False)
    f = runtime.export_filter("planes", [(1.0, 0.0, -0.5, 0.0)], None, 0, 0, 0, False)
    sf, sf_filters = runtime.export_sort_filtered(s, [f])               # the 48-byte form: the same key, the same one filter for every instance
    bounds = torch.zeros((4 * 12,), dtype=torch.int32, device="cuda")   # a record per instance and their union
    b = runtime.bounds_desc(pos, bounds.data_ptr(), 4)
    pd, ps, pf, pb = C.byref(d), C.byref(s), C.byref(f), C.byref(b)
    psf = C.cast(C.byref(sf), C.POINTER(runtime.ExportSort))
    forms = [("effect_export", lambda: lib.hnb_effect_export(fx._h, pd)),
             ("program_export", lambda: lib.hnb_program_export(prog._h, pd, None)),
             ("effect_export_sorted", lambda: lib.hnb_effect_export_sorted(fx._h, pd, ps)),
             ("program_export_sorted/instance", lambda: lib.hnb_program_export_sorted(prog._h, pd, ps, runtime.SORT_SCOPE_INSTANCE, None)),
             ("program_export_sorted/program", lambda: lib.hnb_program_export_sorted(prog._h, pd, ps, runtime.SORT_SCOPE_PROGRAM, None)),
             ("effect_export_filtered", lambda: lib.hnb_effect_export_filtered(fx._h, pd, pf)),
             ("program_export_filtered", lambda: lib.hnb_program_export_filtered(prog._h, pd, pf, 1, None)),
             ("effect_export_filtered_sorted", lambda: lib.hnb_effect_export_filtered_sorted(fx._h, pd, pf, ps)),
             ("program_export_filtered_sorted", lambda: lib.hnb_program_export_sorted(prog._h, pd, psf, runtime.SORT_SCOPE_INSTANCE, None)),
             ("program_bounds", lambda: lib.hnb_program_bounds(prog._h, pb))]
    print(f"{args.label}: {args.calls} calls per window, {args.windows} windows, {args.alive} of {cap} slots alive, us per call")
    for name, call in forms:
        for _ in range(50):                                              # loads the code object, allocates the scratch
            runtime._check(call())
        ctx.synchronize()
        total, enqueue = [], []
        for _ in range(args.windows):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            t1 = time.perf_counter()
            ctx.synchronize()
            t2 = time.perf_counter()
            total.append((t2 - t0) / args.calls * 1e6)
            enqueue.append((t1 - t0) / args.calls * 1e6)
        print(f"{name:32s} call median {statistics.median(total):8.2f} min {min(total):8.2f} max {max(total):8.2f}"
              f"   enqueue median {statistics.median(enqueue):8.2f} min {min(enqueue):8.2f} max {max(enqueue):8.2f}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
