"""hnb_program_export_sorted on the GPU (include/hanabi_amd.h "Packed output", Sorted export, program form). Instance scope: the layout of
hnb_program_export with every instance's segment in the order of its own hnb_effect_export_sorted. Program scope: one order over the particles of
all instances, ties by (instance, list row). Expected records are built on the host as tests/test_gpu_export_sorted.py builds them - read_attr +
alive_list(), the keys restated in numpy binary32, a stable argsort - and everything is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, frame_seed
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, _device_meta, assert_export, expected_records
from test_gpu_export_sorted import DIR, TILE, adversarial_x, key_f32, sort_keys, varying_bytes

pytestmark = pytest.mark.gpu

POS_AGE_ID = [(A.POSITION.id, 0), (A.AGE.id, 12), (A.ID.id, 16)]        # stride 20: segments start at any dword
SCOPES = ("instance", "program")


def make(cap, n_inst, asset=None, slot_bases=None, **options):
    ctx = bh.Context(0)
    for o, v in options.items():
        ctx.set_option(o, v)
    prog = ctx.create_program(bh.lower(asset if asset is not None else effects.firework_trails(cap)))
    fxs = [prog.create_effect(slot_base=slot_bases[k] if slot_bases else 0) for k in range(n_inst)]
    return ctx, prog, fxs


def step(ctx, fxs, f, spawns, dt=1 / 600):
    ctx.frame_begin(dt, f * dt)
    for k, fx in enumerate(fxs):
        fx.set_frame(int(spawns[k]), frame_seed(f * 16 + k))
    ctx.simulate()


def run_sorted(ex, prog, scope, **sort):
    kw = {"offsets_ptr": ex.offsets.data_ptr()} if ex.offsets is not None else {}
    prog.export_sorted(ex.fields, ex.dst.data_ptr(), ex.stride, ex.capacity, ex.cnt.data_ptr(), scope=scope, **kw, **sort)
    return ex


def expected_program(fxs, fields, stride, scope, slot_bases=None, **sort):
    """-> (records [total, stride / 4] in the order the call must write them, alive counts, keys of the concatenated lists) (synchronises)"""
    recs, keys = [], []
    for k, fx in enumerate(fxs):
        alive = fx.alive_list()
        rec = expected_records(fx, fields, stride, slot_base=slot_bases[k] if slot_bases else 0)
        key = sort_keys(fx, alive, **sort)
        if scope == "instance":
            rec = rec[np.argsort(key, kind="stable")]
        recs.append(rec); keys.append(key)
    rec, key = np.concatenate(recs), np.concatenate(keys)
    if scope == "program":
        rec = rec[np.argsort(key, kind="stable")]                        # stable over the concatenation: ties by (instance, list row)
    return rec, [len(r) for r in recs], key


def check(ctx, prog, fxs, what, scope, fields=POS_AGE_LIFE_VEL, stride=32, slot_bases=None, capacity=None, **sort):
    n = len(fxs)
    total_cap = sum(fx.capacity for fx in fxs)
    ex = Export(fields, stride, total_cap if capacity is None else capacity, n_offsets=n + 1 if scope == "instance" else 0)
    run_sorted(ex, prog, scope, **sort)
    ctx.synchronize()
    rec, counts, key = expected_program(fxs, fields, stride, scope, slot_bases, **sort)
    assert_export(ex, rec, f"{what}, scope {scope}, {sort}", alive_rows=len(rec))
    if scope == "instance":
        np.testing.assert_array_equal(ex.offsets.cpu().numpy().view(np.uint32), np.concatenate([[0], np.cumsum(counts)]), err_msg=what)
    return ex, rec, counts, key


@pytest.mark.parametrize("cap,spawns", [(300, [7, 0, 60, 31, 75]), (4096, [37, 0, 700, 301, 1024])])
def test_small_instances_one_workgroup_each(cap, spawns):
    """Five instances in different states - one empty, one frozen in mid-run, one full - at capacities of the one-launch path."""
    n_inst = 5
    bases = [1000 * k for k in range(n_inst)]
    ctx, prog, fxs = make(cap, n_inst, effects.instancing(cap, rate=cap / 0.25), slot_bases=bases)
    for f in range(6):
        if f == 3:
            fxs[2].set_simulated(False)                                  # frozen from here on: its state of frame 2 is what is exported
        step(ctx, fxs, f, spawns if f < 4 else [0] * n_inst, dt=1 / 60)
    for desc in (False, True):
        sort = dict(key="depth", v=DIR, descending=desc)
        ex, rec, counts, key = check(ctx, prog, fxs, f"capacity {cap}", "instance", POS_AGE_ID, 20, bases, **sort)
        assert counts[1] == 0 and counts[2] == 3 * spawns[2] and counts[4] == cap and len(set(counts)) == n_inst
        singles = [Export(POS_AGE_ID, 20, cap) for _ in fxs]
        for fx, single in zip(fxs, singles):
            fx.export_sorted(single.fields, single.dst.data_ptr(), 20, cap, single.cnt.data_ptr(), **sort)
        ctx.synchronize()
        offs = np.concatenate([[0], np.cumsum(counts)])
        for k, single in enumerate(singles):                             # ... and every segment is that instance's own hnb_effect_export_sorted
            np.testing.assert_array_equal(ex.words()[offs[k] * 5: offs[k + 1] * 5], single.words()[: counts[k] * 5], err_msg=f"instance {k}")
        check(ctx, prog, fxs, f"capacity {cap}", "program", POS_AGE_ID, 20, bases, **sort)
    ctx.close()


@pytest.mark.parametrize("cap", [4097, 10_000])
def test_multi_tile_instances(cap):
    """Three instances past one tile: alive counts 0, 1, 4096, then 4097, everything, 4097; both directions."""
    ctx, prog, fxs = make(cap, 3)
    for f, spawns in enumerate(([0, 1, TILE], [TILE + 1, cap - 1, 1])):
        step(ctx, fxs, f, spawns)
        for desc in (False, True):
            ex, rec, counts, key = check(ctx, prog, fxs, f"capacity {cap}, frame {f}", "instance", key="depth", v=DIR, descending=desc)
            assert counts == ([0, 1, TILE] if f == 0 else [TILE + 1, cap, TILE + 1])
        check(ctx, prog, fxs, f"capacity {cap}, frame {f}", "program", key="distance", v=(1, 2, 3))
    ctx.close()


def test_program_scope_past_a_group_of_tiles():
    """3 x 50,000 rows, all alive: 37 tiles of the concatenated space, past a group of 32, the instances' boundaries inside tiles. Then a
    partial state after a die-off: permuted lists."""
    cap = 50_000
    ctx, prog, fxs = make(cap, 3)
    step(ctx, fxs, 0, [cap] * 3)
    ex, rec, counts, key = check(ctx, prog, fxs, "all alive", "program", key="depth", v=DIR)
    assert counts == [cap] * 3 and (3 * cap + TILE - 1) // TILE == 37 and varying_bytes(key) == [0, 1, 2, 3]
    for f in range(1, 5):                                               # lifetimes are 0.8 .. 1.2 s: a second later part of the burst is gone
        step(ctx, fxs, f, [0] * 3, dt=0.25)
    ex, rec, counts, key = check(ctx, prog, fxs, "after the die-off", "program", key="depth", v=DIR, descending=True)
    assert all(0 < c < cap for c in counts) and not np.array_equal(fxs[1].alive_list(), np.arange(counts[1]))
    check(ctx, prog, fxs, "after the die-off", "instance", key="depth", v=DIR)
    ctx.close()


def test_adversarial_keys_and_stability_across_instances():
    """Planes written through write_attr: the depth key along (1, 0, 0) with y = z = -0 is x itself. The key patterns run over the concatenation of
    the three lists, so every value occurs in different instances: ties must come out by (instance, list row), ascending and descending."""
    cap, n_inst = 5000, 3
    ctx, prog, fxs = make(cap, n_inst)
    step(ctx, fxs, 0, [cap] * n_inst)
    ctx.synchronize()
    lists = [fx.alive_list() for fx in fxs]
    assert all(len(a) == cap for a in lists)
    cases = adversarial_x(cap * n_inst)
    i = np.arange(cap * n_inst, dtype=np.uint64)
    cases["two values"] = np.asarray([1.0, -2.0], np.float32).view(np.uint32)[(i * np.uint64(7919) % np.uint64(2)).astype(np.int64)]
    passes = {}
    for name in ("one value", "two values", "four values", "lowest byte", "highest byte", "specials"):
        xbits = cases[name]
        for k, fx in enumerate(fxs):
            pos = np.full((cap, 3), np.float32(-0.0).view(np.uint32), np.uint32)
            pos[lists[k], 0] = xbits[k * cap: (k + 1) * cap]
            fx.write_attr(A.POSITION.id, pos)
        for desc in (False, True):
            ex, rec, counts, key = check(ctx, prog, fxs, name, "program", key="depth", v=(1, 0, 0), descending=desc)
            np.testing.assert_array_equal(key, ~key_f32(xbits) if desc else key_f32(xbits), err_msg=name)       # the key is x itself
            if name == "one value":                                      # nothing to order by: instance after instance, each in list order
                np.testing.assert_array_equal(rec, np.concatenate([expected_records(fx, POS_AGE_LIFE_VEL, 32) for fx in fxs]))
            if not desc:
                passes[name] = varying_bytes(key)
        check(ctx, prog, fxs, name, "instance", key="depth", v=(1, 0, 0), descending=True)
    assert passes["one value"] == [] and passes["lowest byte"] == [0] and passes["highest byte"] == [3] and passes["specials"] == [0, 1, 2, 3]
    assert len(passes["two values"]) >= 1
    ctx.close()


def test_clamp_is_global_in_both_scopes():
    cap, n_inst = 4097, 3
    ctx, prog, fxs = make(cap, n_inst)
    step(ctx, fxs, 0, [cap, 3000, cap])
    sort = dict(key="distance", v=(1, 2, 3))
    rec_i, counts, _ = expected_program(fxs, POS_AGE_LIFE_VEL, 32, "instance", **sort)
    rec_p, _, _ = expected_program(fxs, POS_AGE_LIFE_VEL, 32, "program", **sort)
    total = sum(counts)
    assert counts == [cap, 3000, cap]
    room = counts[0] + counts[1] + counts[2] // 2                        # two and a half instances: the cut one keeps the FIRST records of its order
    ex = run_sorted(Export(POS_AGE_LIFE_VEL, 32, room, slack=total), prog, "instance", **sort)
    ctx.synchronize()
    assert ex.counts() == [room, total]
    assert_export(ex, rec_i, "instance scope, two and a half instances", alive_rows=total)
    for K in (1, 255, 4097, total - 1):
        ex = run_sorted(Export(POS_AGE_LIFE_VEL, 32, K, slack=64), prog, "program", **sort)
        ctx.synchronize()
        assert ex.counts() == [K, total]
        assert_export(ex, rec_p, f"nearest {K} of the program", alive_rows=total)
    for scope in SCOPES:
        ex0 = run_sorted(Export(POS_AGE_LIFE_VEL, 32, 0, slack=16), prog, scope, **sort)
        ctx.synchronize()
        assert ex0.counts() == [0, total] and (ex0.words() == SENTINEL).all()
    ctx.close()


def test_ring_lists_are_read_through_their_heads_and_left_alone():
    cap = 10_000
    fields = [(A.AGE.id, 0), (A.POSITION.id, 4), (A.RIBBON_ID.id, 16), (A.SIZE.id, 20)]
    asset = effects.ribbon(cap)
    ctx, prog, fxs = make(cap, 2, asset, ring_lists=1)
    sps, rng = [bh.EffectSpawner(asset.spawner) for _ in fxs], bh.Pcg32()
    for f in range(90):
        dt = 1 / 60
        ctx.frame_begin(dt, f * dt)
        for k, fx in enumerate(fxs):
            n = sps[k].tick(dt, rng)
            fx.set_frame(n if (k == 0 or f >= 20) else 0, frame_seed(f * 2 + k))     # the second ribbon starts later: another head, another count
        ctx.simulate()
    ctx.synchronize()
    metas = [_device_meta(fx) for fx in fxs]
    assert all((m.list_column >> 1) != 0 and m.alive_count > 64 for m in metas)
    assert (metas[0].list_column, metas[0].alive_count) != (metas[1].list_column, metas[1].alive_count)
    before = [fx.alive_list().copy() for fx in fxs]
    for scope in SCOPES:
        for desc in (False, True):
            check(ctx, prog, fxs, "ring", scope, fields, 24, key="attr", attr=A.AGE.id, descending=desc)
    for fx, b, m in zip(fxs, before, metas):
        np.testing.assert_array_equal(fx.alive_list(), b)
        m2 = _device_meta(fx)
        assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


@pytest.mark.parametrize("cohort", [1, 3], ids=["lean", "auto"])
def test_stale_age_is_current_as_field_and_as_key(cohort):
    cap = 65_536
    fields = [(A.AGE.id, 0), (A.LIFETIME.id, 4), (A.POSITION.id, 8)]
    ctx, prog, fxs = make(cap, 2, age_cohort=cohort)
    for f in range(5):
        step(ctx, fxs, f, [40_000, 9000] if f == 0 else [3000, 5000], dt=1 / 60)
    keep = [run_sorted(Export(fields, 20, 2 * cap, n_offsets=3 if scope == "instance" else 0), prog, scope, key="attr", attr=A.AGE.id, descending=True)
            for scope in SCOPES]                                         # no materialise call in front of them
    ctx.synchronize()
    for scope, ex in zip(SCOPES, keep):
        rec, counts, key = expected_program(fxs, fields, 20, scope, key="attr", attr=A.AGE.id, descending=True)       # (the read-back materialises for itself)
        assert counts == [52_000, 29_000] and len(np.unique(rec[:, 0])) == 5
        assert_export(ex, rec, f"stale AGE, cohort mode {cohort}, scope {scope}")
    ages = keep[1].words()[: 81_000 * 5].reshape(-1, 5)[:, 0].view(np.float32)
    assert (ages[1:] <= ages[:-1]).all() and ages[0] > ages[-1]           # oldest first over the whole program
    ctx.close()


def test_disturbs_nothing():
    cap, n_inst = 10_000, 3
    pairs = [make(cap, n_inst) for _ in range(2)]
    for f in range(5):
        for ctx, prog, fxs in pairs:
            step(ctx, fxs, f, [cap, cap // 2, 17] if f == 0 else [0] * n_inst, dt=0.25 if f else 1 / 600)
    (ctx, prog, fxs), (tctx, tprog, twins) = pairs
    ctx.synchronize()
    lists = [(fx.alive_list().copy(), fx.dead_list().copy()) for fx in fxs]
    for scope in SCOPES:
        check(ctx, prog, fxs, "between frames", scope, key="depth", v=DIR, descending=True)
    plain = Export(POS_AGE_LIFE_VEL, 32, n_inst * cap, n_offsets=n_inst + 1).run(prog)
    ctx.synchronize()
    assert_export(plain, np.concatenate([expected_records(fx, POS_AGE_LIFE_VEL, 32) for fx in fxs]), "hnb_program_export behind: list order")
    for fx, (alive, dead) in zip(fxs, lists):
        np.testing.assert_array_equal(fx.alive_list(), alive)
        np.testing.assert_array_equal(fx.dead_list(), dead)
    keep = []
    for f in range(5, 20):
        for c, p, e in pairs:
            step(c, e, f, [300, 0, 50] if f % 4 == 0 else [0] * n_inst, dt=1 / 20)
        if f % 5 == 0:                                                   # exports between the frames, nothing waits
            for scope in SCOPES:
                keep.append(run_sorted(Export(POS_AGE_LIFE_VEL, 32, n_inst * cap), prog, scope, key="distance", v=(1, 2, 3)))
    ctx.synchronize(); tctx.synchronize()
    for fx, twin in zip(fxs, twins):
        d = fx.compare(twin)
        assert d["equal"] == 1, d
        assert fx.check()["ok"] == 1
    ctx.close(); tctx.close()


@pytest.mark.parametrize("cap", [1000, 6000])
def test_a_program_that_gains_an_instance(cap):
    ctx, prog, fxs = make(cap, 2)
    step(ctx, fxs, 0, [cap, cap // 3])
    for scope in SCOPES:
        check(ctx, prog, fxs, "two instances", scope, key="depth", v=DIR)
    fxs.append(prog.create_effect())
    step(ctx, fxs, 1, [0, 100, cap - 7])
    for scope in SCOPES:
        ex, rec, counts, key = check(ctx, prog, fxs, "three instances", scope, key="depth", v=DIR)
        assert counts == [cap, cap // 3 + 100, cap - 7]
    ctx.close()


def test_argument_errors_enqueue_nothing():
    cap = 1000
    ctx, prog, fxs = make(cap, 2)
    empty = ctx.create_program(bh.lower(effects.firework_trails(cap)))    # a program without instances
    step(ctx, fxs, 0, [cap, 10])
    ex = Export(POS_AGE_LIFE_VEL, 32, 2 * cap, n_offsets=3)
    dst, cnt, offs = ex.dst.data_ptr(), ex.cnt.data_ptr(), ex.offsets.data_ptr()
    ok = dict(key="depth", v=DIR)
    bad = {
        "scope 2": dict(scope=2),
        "out_offsets with the program scope": dict(scope="program", offsets_ptr=offs),
        "misaligned out_offsets": dict(offsets_ptr=offs + 2),
        "no instances": dict(prog=empty),
        "PARTICLE_COUNTER": dict(fields=[(A.PARTICLE_COUNTER.id, 0)]),
        "an attribute the layout lacks": dict(fields=[(A.POSITION.id, 0), (A.SIZE.id, 12)]),
        "overlapping fields": dict(fields=[(A.POSITION.id, 0), (A.AGE.id, 8)]),
        "a misaligned dst": dict(dst=dst + 4),
        "a stride above 256": dict(fields=[(A.AGE.id, 0)], stride=260),
        "an unknown key": dict(sort=dict(key=3)),
        "descending above 1": dict(sort=dict(key="depth", v=DIR, descending=2)),
        "ATTR with a vector attribute": dict(sort=dict(key="attr", attr=A.VELOCITY.id)),
        "ATTR with ID": dict(sort=dict(key="attr", attr=A.ID.id)),
        "DEPTH with a NaN direction": dict(sort=dict(key="depth", v=(float("nan"), 0, 1))),
    }
    for what, kw in bad.items():
        for scope in ([kw["scope"]] if "scope" in kw else SCOPES):
            with pytest.raises(bh.HanabiError) as ei:
                kw.get("prog", prog).export_sorted(kw.get("fields", POS_AGE_LIFE_VEL), kw.get("dst", dst), kw.get("stride", 32), 2 * cap, cnt,
                                                   kw.get("offsets_ptr"), scope=scope, **kw.get("sort", ok))
            assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    lib = runtime.load_library()
    d = runtime.export_desc(POS_AGE_LIFE_VEL, dst, 32, 2 * cap, cnt)
    s = runtime.export_sort("depth", v=DIR)
    assert lib.hnb_program_export_sorted(prog._h, C.byref(d), None, 0, None) == -1 and lib.hnb_program_export_sorted(prog._h, None, C.byref(s), 1, None) == -1
    for obj, field, value in ((s, "struct_size", 28), (s, "reserved", 1), (d, "struct_size", 64), (d, "flags", 1)):
        keep = getattr(obj, field)
        setattr(obj, field, value)
        for scope in (0, 1):
            assert lib.hnb_program_export_sorted(prog._h, C.byref(d), C.byref(s), scope, None) == -1 and len(lib.hnb_last_error()) > 8, field
        setattr(obj, field, keep)
    ctx.synchronize()
    assert ex.untouched() and (ex.offsets.cpu().numpy().view(np.uint32) == SENTINEL).all()
    for scope in SCOPES:                                                 # ... and a valid call behind the refusals gives the right result
        check(ctx, prog, fxs, "after the refusals", scope, key="depth", v=DIR)
    ctx.close()
