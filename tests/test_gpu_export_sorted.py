"""hnb_effect_export_sorted on the GPU (include/hanabi_amd.h "Packed output", Sorted export): record r of the caller's buffer = the particle with the
r-th smallest key, ties in list order. Expected records are built on the host as tests/test_gpu_export.py builds them (read_attr + alive_list()),
the keys restated in numpy binary32 / uint32 from the header's formulas, the order from a stable argsort. Everything is compared bit for bit:
every result is uniquely determined, there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, frame_seed
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, _device_meta, assert_export, expected_records, step

pytestmark = pytest.mark.gpu

TILE = 4096                                     # rows per workgroup of the sort; capacities up to it take the one-launch path
CAPS = (300, 4096, 4097, 10_000, 135_245)       # partial tile | exactly one tile | first multi-tile, last tile of one row | three ragged tiles | 33 tiles + 77: past a group of 32
DIR = (0.3, -0.5, 0.8)


def key_f32(bits):
    b = np.asarray(bits, np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def sort_keys(fx, alive, key, v=(0, 0, 0), attr=0, descending=False):
    """The header's key of every alive row, in list order: binary32 operations one by one, in the order the header writes them."""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        if key == "attr":
            bits = fx.read_attr(attr).view(np.uint32).reshape(-1)[alive]
            k = key_f32(bits) if runtime.ATTR_IS_FLOAT[int(attr)] else bits.copy()
        else:
            p = fx.read_attr(A.POSITION.id).view(np.float32).reshape(-1, 3)[alive]
            if key == "depth":
                d = (p[:, 0] * v[0] + p[:, 1] * v[1]) + p[:, 2] * v[2]
            else:
                e = p - v
                d = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            assert d.dtype == np.float32
            k = key_f32(d.view(np.uint32))
    return ~k if descending else k


def expected_sorted(fx, fields, stride, **sort):
    alive = fx.alive_list()
    k = sort_keys(fx, alive, **sort)
    order = np.argsort(k, kind="stable")
    return expected_records(fx, fields, stride)[order], k, order


def run_sorted(ex, fx, **sort):
    fx.export_sorted(ex.fields, ex.dst.data_ptr(), ex.stride, ex.capacity, ex.cnt.data_ptr(), **sort)
    return ex


def check_sorted(ctx, fx, what, fields=POS_AGE_LIFE_VEL, stride=32, capacity=None, **sort):
    """export, synchronise, compare; -> (keys in list order, the stable order)"""
    ex = run_sorted(Export(fields, stride, fx.capacity if capacity is None else capacity), fx, **sort)
    ctx.synchronize()
    rec, k, order = expected_sorted(fx, fields, stride, **sort)
    assert_export(ex, rec, f"{what} {sort}", alive_rows=len(rec))
    return k, order


def make(cap, asset=None, **options):
    ctx = bh.Context(0)
    for o, v in options.items():
        ctx.set_option(o, v)
    fx = ctx.create_program(bh.lower(asset if asset is not None else effects.firework_trails(cap))).create_effect()
    return ctx, fx


@pytest.mark.parametrize("cap", CAPS)
def test_tile_and_group_edges(cap):
    """Alive counts 0, 1, 255..257, 4095..4097 and everything, reached by spawning; depth along a slanted direction, both directions."""
    ctx, fx = make(cap)
    f, have = 0, 0
    for want in [c for c in (0, 1, 255, 256, 257, 4095, 4096, 4097) if c <= cap] + [cap]:
        if want > have:
            step(ctx, fx, f, want - have)
            f += 1
            have = want
        for desc in (False, True):
            k, order = check_sorted(ctx, fx, f"capacity {cap}, {want} alive", key="depth", v=DIR, descending=desc)
            assert len(k) == want
        if want > 64:
            assert not np.array_equal(order, np.arange(want))           # the keys do reorder the list
    ctx.close()


def burst_then_die_off(cap):
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    for f in range(1, 5):                                               # lifetimes are 0.8 .. 1.2 s: a second later part of the burst is gone
        step(ctx, fx, f, 0, dt=0.25)
    return ctx, fx


@pytest.mark.parametrize("cap", [10_000, 135_245])
def test_permuted_partial_list_after_a_die_off(cap):
    ctx, fx = burst_then_die_off(cap)
    alive = fx.alive_list()
    assert 0 < len(alive) < cap and not np.array_equal(alive, np.arange(len(alive)))
    for sort in (dict(key="depth", v=DIR), dict(key="distance", v=(1, 2, 3)), dict(key="distance", v=(1, 2, 3), descending=True)):
        check_sorted(ctx, fx, f"die-off at {cap}", **sort)
    ctx.close()


def test_permuted_list_of_a_rate_spawner_churn():
    cap = 135_245
    ctx, fx = make(cap, effects.firework_trails(cap, spawner=bh.SpawnerSettings.rate(3000.0)))
    rng = np.random.default_rng(5)
    for f in range(60):
        step(ctx, fx, f, int(rng.integers(1000, 6000)), dt=1 / 20)
    alive = fx.alive_list()
    assert 4 * TILE < len(alive) < cap and not np.array_equal(alive, np.sort(alive))
    for sort in (dict(key="depth", v=DIR, descending=True), dict(key="distance", v=(1, 2, 3))):
        check_sorted(ctx, fx, "churn", **sort)
    ctx.close()


def test_ring_list_is_read_through_its_head_and_left_alone():
    cap = 10_000
    fields = [(A.AGE.id, 0), (A.POSITION.id, 4), (A.RIBBON_ID.id, 16), (A.SIZE.id, 20)]
    asset = effects.ribbon(cap)
    ctx, fx = make(cap, asset, ring_lists=1)
    sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
    for f in range(90):
        dt = 1 / 60
        ctx.frame_begin(dt, f * dt)
        fx.set_frame(sp.tick(dt, rng), frame_seed(f))
        ctx.simulate()
    ctx.synchronize()
    m = _device_meta(fx)
    assert (m.list_column >> 1) != 0 and m.alive_count > 256            # kept as a ring, the head somewhere inside the column
    before = fx.alive_list().copy()
    check_sorted(ctx, fx, "ring", fields=fields, stride=24, key="attr", attr=A.AGE.id)
    k, order = check_sorted(ctx, fx, "ring", fields=fields, stride=24, key="attr", attr=A.AGE.id, descending=True)
    assert not np.array_equal(order, np.arange(len(order)))             # (the ribbon's own order is youngest first: oldest first moves every row)
    np.testing.assert_array_equal(fx.alive_list(), before)              # the list, and with it the ribbon's own sort order, is what it was
    m2 = _device_meta(fx)
    assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


def _perm256(i, mul=167, add=13):
    return ((i.astype(np.uint64) * mul + add) % 256).astype(np.uint32)


def adversarial_x(n):
    """name -> x bits in list order; the depth key along (1, 0, 0) with y = z = -0 is x itself: (x * 1 + -0 * 0) + -0 * 0 = x for every x, -0 included."""
    i = np.arange(n, dtype=np.uint64)
    f32 = lambda a: np.asarray(a, np.float32).view(np.uint32)
    specials = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC01234, 0xFFFFFFFF,
                         0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)
    rng = np.random.default_rng(n)
    mixed = rng.uniform(-4.0, 4.0, n).astype(np.float32).view(np.uint32)
    mixed[np.arange(n) % 3 == 1] = specials[(np.arange(n)[np.arange(n) % 3 == 1] // 3 * 5) % len(specials)]
    return {
        "one value": np.full(n, f32(0.75), np.uint32),                                                      # no pass runs: list order, both directions
        "four values": f32(np.array([1.0, -2.0, 0.5, 3e10], np.float32))[(i * np.uint64(7919) % np.uint64(4)).astype(np.int64)],   # thousands of ties each
        "lowest byte": np.uint32(0x3F000000) | _perm256(i),                                                 # one pass (odd: the result is in the other buffer)
        "highest byte": ((_perm256(i) & np.uint32(0x7F)) << np.uint32(24)) | np.uint32(0x00123456),         # one pass, the last; denormals where the byte is 0
        "bytes 0 and 3": ((_perm256(i // np.uint64(3), 201, 128) & np.uint32(0x7F)) << np.uint32(24)) | np.uint32(0x00123400) | _perm256(i),          # two passes
        "bytes 0, 1 and 3": ((_perm256(i // np.uint64(5), 91, 7) & np.uint32(0x7F)) << np.uint32(24)) | np.uint32(0x00120000) | (_perm256(i // np.uint64(2), 77, 255) << np.uint32(8)) | _perm256(i),   # three
        "specials": mixed,                                                                                  # +-0, +-inf, NaNs of both signs, denormals among normals
        "sorted": f32(np.arange(n, dtype=np.float32)),
        "reversed": f32(np.arange(n, 0, -1, dtype=np.float32)),
    }


def varying_bytes(k):
    v = int(np.bitwise_or.reduce(k) & np.bitwise_or.reduce(~k))
    return [b for b in range(4) if (v >> (8 * b)) & 0xFF]


@pytest.mark.parametrize("cap", [10_000, 135_245])
def test_adversarial_keys_and_stability(cap):
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    alive = fx.alive_list()
    assert len(alive) == cap
    passes = {}
    for name, xbits in adversarial_x(cap).items():
        pos = np.full((cap, 3), np.float32(-0.0).view(np.uint32), np.uint32)
        pos[alive, 0] = xbits
        fx.write_attr(A.POSITION.id, pos)
        for desc in (False, True):
            k, order = check_sorted(ctx, fx, f"{name} at {cap}", key="depth", v=(1, 0, 0), descending=desc)
            np.testing.assert_array_equal(k, ~key_f32(xbits) if desc else key_f32(xbits), err_msg=name)     # the key is x itself
            if not desc:
                passes[name] = varying_bytes(k)
        if name == "one value":
            assert np.array_equal(order, np.arange(cap))                # list order, ascending and descending (check_sorted compared both with it)
        if name == "four values":
            assert len(np.unique(k)) == 4 and np.bincount(np.unique(k, return_inverse=True)[1]).min() > 2000
    assert passes["one value"] == [] and passes["lowest byte"] == [0] and passes["highest byte"] == [3]
    assert passes["bytes 0 and 3"] == [0, 3] and passes["bytes 0, 1 and 3"] == [0, 1, 3] and passes["specials"] == [0, 1, 2, 3]
    ctx.close()


@pytest.mark.parametrize("cap", [3000, 10_000])
def test_u32_attribute_sorts_unsigned(cap):
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    assert not runtime.ATTR_IS_FLOAT[A.COLOR.id]
    rng = np.random.default_rng(cap)
    color = (0x7FFFFFFF + rng.integers(-300, 300, cap).astype(np.int64)).astype(np.uint32)
    color[::7] = 0x80000000
    color[3::7] = 0x7FFFFFFF
    color[5::11] = 0xFFFFFFFF
    color[6::13] = 0
    fx.write_attr(A.COLOR.id, color.reshape(cap, 1))
    fields = [(A.COLOR.id, 0), (A.POSITION.id, 4)]
    for desc in (False, True):
        k, order = check_sorted(ctx, fx, "COLOR", fields=fields, stride=16, key="attr", attr=A.COLOR.id, descending=desc)
    got = color[fx.alive_list()][order]                                 # (descending, from the last round)
    assert (got[1:].astype(np.int64) <= got[:-1].astype(np.int64)).all() and got[0] == 0xFFFFFFFF and got[-1] == 0       # unsigned: 0x80000000 above 0x7FFFFFFF
    ctx.close()


def test_top_k_clamp():
    cap = 10_000
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0)
    for K in (1, 255, 4096, cap - 1):
        ex = run_sorted(Export(POS_AGE_LIFE_VEL, 32, K, slack=64), fx, key="distance", v=(1, 2, 3))
        ctx.synchronize()
        rec, k, order = expected_sorted(fx, POS_AGE_LIFE_VEL, 32, key="distance", v=(1, 2, 3))
        assert len(rec) == cap and ex.counts() == [K, cap]
        assert_export(ex, rec, f"nearest {K}", alive_rows=cap)           # the first K of the sorted order, sentinels behind record K
    ex0 = run_sorted(Export(POS_AGE_LIFE_VEL, 32, 0, slack=16), fx, key="distance", v=(1, 2, 3))
    ctx.synchronize()
    assert ex0.counts() == [0, cap] and (ex0.words() == SENTINEL).all()
    ctx.close()


def test_stale_age_is_current_as_field_and_as_key_and_nothing_later_changes():
    """LEAN cohorts: the AGE plane is stale until something materialises it. The sorted export does, for the field and for the key; a twin context
    that never exports ends the run in the same state."""
    cap = 100_000
    fields = [(A.AGE.id, 0), (A.LIFETIME.id, 4), (A.POSITION.id, 8)]
    pairs = [make(cap, age_cohort=1) for _ in range(2)]
    (ctx, fx), (tctx, twin) = pairs
    assert fx.device_view().stale_attr_mask == 1 << A.AGE.id
    keep = []
    for f in range(5):
        for c, e in pairs:
            step(c, e, f, 70_000 if f == 0 else 3000, dt=1 / 60)
        if f >= 3:
            for desc in (False, True):                                   # no materialise call in front of it
                keep.append((f, desc, run_sorted(Export(fields, 20, cap), fx, key="attr", attr=A.AGE.id, descending=desc)))
    for f, desc, ex in keep[-2:]:                                        # the last frame's two, against the read-back (which materialises for itself)
        ctx.synchronize()
        rec, k, order = expected_sorted(fx, fields, 20, key="attr", attr=A.AGE.id, descending=desc)
        assert len(rec) == 70_000 + 4 * 3000 and len(np.unique(rec[:, 0])) == 5
        assert_export(ex, rec, f"stale AGE, descending={desc}")
        ages = rec[:, 0].view(np.float32)
        assert (ages[1:] <= ages[:-1]).all() if desc else (ages[1:] >= ages[:-1]).all()
    assert keep[0][2].counts() == [70_000 + 3 * 3000] * 2
    for f in range(5, 12):
        for c, e in pairs:
            step(c, e, f, 0, dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    d = fx.compare(twin)
    assert d["equal"] == 1, d
    assert fx.check()["ok"] == 1
    ctx.close(); tctx.close()


def test_sorted_export_disturbs_nothing():
    cap = 10_000
    (ctx, fx), (tctx, twin) = burst_then_die_off(cap), burst_then_die_off(cap)
    ctx.synchronize()
    alive, dead = fx.alive_list().copy(), fx.dead_list().copy()
    first = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    mid = run_sorted(Export(POS_AGE_LIFE_VEL, 32, cap), fx, key="depth", v=DIR, descending=True)
    second = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    ctx.synchronize()
    rec = expected_records(fx, POS_AGE_LIFE_VEL, 32)
    assert_export(first, rec, "plain export in front")
    assert_export(second, rec, "plain export behind: list order again")
    assert_export(mid, expected_sorted(fx, POS_AGE_LIFE_VEL, 32, key="depth", v=DIR, descending=True)[0], "between them")
    np.testing.assert_array_equal(fx.alive_list(), alive)
    np.testing.assert_array_equal(fx.dead_list(), dead)
    for f in range(5, 25):
        for c, e in ((ctx, fx), (tctx, twin)):
            step(c, e, f, 300 if f % 4 == 0 else 0, dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    d = fx.compare(twin)
    assert d["equal"] == 1, d
    ctx.close(); tctx.close()


def test_back_to_back_exports_share_the_scratch_in_stream_order():
    """Different keys into different destinations with no synchronisation between the calls; and effects on both paths in one context. (The capacity
    belongs to the program, so the one-launch and the multi-tile path are two programs here, two effects of each.)"""
    ctx = bh.Context(0)
    fxs = []
    for cap in (TILE, 10_000):
        prog = ctx.create_program(bh.lower(effects.firework_trails(cap)))
        fxs += [prog.create_effect(), prog.create_effect()]
    ctx.frame_begin(1 / 60, 0.0)
    for i, fx in enumerate(fxs):
        fx.set_frame(fx.capacity - 100 * i, frame_seed(i))
    ctx.simulate()
    step_sorts = [dict(key="depth", v=DIR), dict(key="distance", v=(1, 2, 3), descending=True), dict(key="attr", attr=A.LIFETIME.id), dict(key="depth", v=(0, 1, 0))]
    runs = []
    for fx in fxs:                                                      # four exports per effect, sixteen in all, nothing waits in between
        for sort in step_sorts:
            runs.append((fx, sort, run_sorted(Export(POS_AGE_LIFE_VEL, 32, fx.capacity), fx, **sort)))
    ctx.synchronize()
    for fx, sort, ex in runs:
        assert_export(ex, expected_sorted(fx, POS_AGE_LIFE_VEL, 32, **sort)[0], f"capacity {fx.capacity}, effect {fx.index()}, {sort}")
    ctx.close()


def test_argument_errors_enqueue_nothing():
    """Every refusal of the contract but one: DEPTH / DISTANCE on a layout without POSITION cannot be reached from here, because the lowering
    refuses an asset whose layout lacks POSITION ("missing the 'POSITION' attribute") - no program of that kind can be created to export from."""
    cap = 1000
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    step(ctx, fx, 0, cap)
    ex = Export(POS_AGE_LIFE_VEL, 32, cap)
    ok = dict(key="depth", v=DIR)
    bad_desc = {       # every case hnb_effect_export rejects
        "PARTICLE_COUNTER": dict(fields=[(A.PARTICLE_COUNTER.id, 0)]),
        "an attribute the layout lacks": dict(fields=[(A.POSITION.id, 0), (A.SIZE.id, 12)]),
        "overlapping fields": dict(fields=[(A.POSITION.id, 0), (A.AGE.id, 8)]),
        "a field past the stride": dict(fields=[(A.POSITION.id, 0), (A.VELOCITY.id, 24)]),
        "a field at an odd byte": dict(fields=[(A.AGE.id, 2)]),
        "a misaligned dst": dict(dst=ex.dst.data_ptr() + 4),
        "no field": dict(fields=[]),
        "too many fields": dict(fields=[(A.AGE.id, 0)] * 17, stride=128),
        "a stride that is no multiple of 4": dict(stride=34),
        "a stride above 256": dict(fields=[(A.AGE.id, 0)], stride=260),
        "an unknown attribute id": dict(fields=[(39, 0)]),
    }
    for what, kw in bad_desc.items():
        with pytest.raises(bh.HanabiError) as ei:
            fx.export_sorted(kw.get("fields", POS_AGE_LIFE_VEL), kw.get("dst", ex.dst.data_ptr()), kw.get("stride", 32), cap, ex.cnt.data_ptr(), **ok)
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    bad_sort = {
        "an unknown key": dict(key=3),
        "descending above 1": dict(key="depth", v=DIR, descending=2),
        "ATTR with an attribute the layout lacks": dict(key="attr", attr=A.SIZE.id),
        "ATTR with a vector attribute": dict(key="attr", attr=A.VELOCITY.id),
        "ATTR with ID": dict(key="attr", attr=A.ID.id),
        "ATTR with PARTICLE_COUNTER": dict(key="attr", attr=A.PARTICLE_COUNTER.id),
        "ATTR with an unknown attribute": dict(key="attr", attr=39),
        "DEPTH with an infinite direction": dict(key="depth", v=(0, float("inf"), 1)),
        "DEPTH with a NaN direction": dict(key="depth", v=(float("nan"), 0, 1)),
        "DISTANCE from a non-finite point": dict(key="distance", v=(0, 0, float("-inf"))),
    }
    for what, sort in bad_sort.items():
        with pytest.raises(bh.HanabiError) as ei:
            fx.export_sorted(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, cap, ex.cnt.data_ptr(), **sort)
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    lib = runtime.load_library()
    d = runtime.export_desc(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, cap, ex.cnt.data_ptr())
    s = runtime.export_sort("depth", v=DIR)
    assert lib.hnb_effect_export_sorted(fx._h, C.byref(d), None) == -1 and lib.hnb_effect_export_sorted(fx._h, None, C.byref(s)) == -1
    for field, value in (("struct_size", 28), ("reserved", 1)):
        keep = getattr(s, field)
        setattr(s, field, value)
        assert lib.hnb_effect_export_sorted(fx._h, C.byref(d), C.byref(s)) == -1 and len(lib.hnb_last_error()) > 8, field
        setattr(s, field, keep)
    for field, value in (("struct_size", 64), ("flags", 1)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert lib.hnb_effect_export_sorted(fx._h, C.byref(d), C.byref(s)) == -1, field
        setattr(d, field, keep)
    ctx.synchronize()
    assert ex.untouched()
    assert lib.hnb_effect_export_sorted(fx._h, C.byref(d), C.byref(s)) == 0       # ... and the same arguments, unbroken, are accepted
    ctx.synchronize()
    assert ex.counts() == [cap, cap]
    assert_export(ex, expected_sorted(fx, POS_AGE_LIFE_VEL, 32, key="depth", v=DIR)[0], "after the refusals")
    ctx.close()
