"""hnb_program_export_sorted with an HnbExportSortFiltered on the GPU (include/hanabi_amd.h "Packed output", Filtered, then sorted export, program
form): the layout of hnb_program_export_filtered, instance k's segment byte for byte what hnb_effect_export_filtered_sorted(effect k, the filter of
k, sort) writes. The expected buffer of every case IS that: the per-effect calls' records, read back and concatenated. Independently of the
library, the kept sets and the orders are held against the numpy binary32 restatements of the header's predicates and keys that the sibling tests
share (filter_mask, sort_keys, a stable argsort). Everything is compared bit for bit: there is no tolerance anywhere."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, frame_seed
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, _device_meta, assert_export, expected_records
from test_gpu_export_filtered import ALL, HALF, NONE, cloud_sphere, filter_mask
from test_gpu_export_filtered_sorted import Frozen, run_fs
from test_gpu_export_sorted import DIR, sort_keys
import test_gpu_program_export_filtered as pef
import test_gpu_program_export_sorted as pes
from test_gpu_program_export_filtered import BASES, filters_of, fx_slot_base, make_based
from test_gpu_program_export_sorted import POS_AGE_ID, make, step

pytestmark = pytest.mark.gpu

F32 = np.float32
DEPTH, DEPTH_DESC = dict(key="depth", v=DIR), dict(key="depth", v=DIR, descending=True)
NEAR, FAR = dict(key="distance", v=(1, 2, 3)), dict(key="distance", v=(1, 2, 3), descending=True)
TIES = dict(key="depth", v=(0, 0, 0))                                    # every key is that of +0 or of a NaN: list order decides
SMALL_CAPS = (1, 63, 64, 65, 4095, 4096)                                 # one workgroup per instance
LARGE_CAPS = (4097, 8193, 300_007)                                       # tiles: two, the second of one row | three, the last of one row | 74, past two groups of 32


def run_prog(ex, prog, flt, sort):
    prog.export_filtered_sorted(ex.fields, ex.dst.data_ptr(), ex.stride, ex.capacity, ex.cnt.data_ptr(), ex.offsets.data_ptr() if ex.offsets is not None else None,
                                filter=flt, sort=sort)
    return ex


def expected_prog(ctx, fxs, fields, stride, flt, sort, verify=None):
    """-> (records, kept counts, alive counts): the concatenation of hnb_effect_export_filtered_sorted per instance, read back (synchronises).
    For every instance in `verify` (default: all) the records are held against the restatement: the predicate's mask over the list, the keys of
    the kept rows, a stable argsort."""
    sdw = stride // 4
    flts = filters_of(flt, len(fxs))
    singles = [run_fs(Export(fields, stride, fx.capacity), fx, f, sort) for fx, f in zip(fxs, flts)]
    ctx.synchronize()
    recs, kept, alive = [], [], []
    for k, (fx, f, single) in enumerate(zip(fxs, flts, singles)):
        written, found = single.counts()
        assert written == found <= fx.capacity
        rec = single.words()[: found * sdw].reshape(found, sdw)
        if verify is None or k in verify:
            host = Frozen(fx)
            mask = filter_mask(host, host.alive_list(), **f)
            order = np.argsort(sort_keys(host, host.alive_list(), **sort)[mask], kind="stable")
            assert int(mask.sum()) == found, (k, f, int(mask.sum()), found)
            np.testing.assert_array_equal(rec, expected_records(host, fields, stride, slot_base=fx_slot_base(fx))[mask][order], err_msg=f"instance {k}")
            alive.append(len(host.alive_list()))
        else:
            alive.append(fx.alive_count())
        recs.append(rec); kept.append(found)
    return np.concatenate(recs), kept, alive


def check(ctx, prog, fxs, what, flt, sort, fields=POS_AGE_ID, stride=20, capacity=None, offsets=True, partial=True, verify=None):
    """the program call in FRONT of the per-effect ones (nothing before it has materialised or computed anything for it), then compare"""
    n = len(fxs)
    ex = run_prog(Export(fields, stride, sum(fx.capacity for fx in fxs) if capacity is None else capacity, n_offsets=n + 1 if offsets else 0), prog, flt, sort)
    rec, kept, alive = expected_prog(ctx, fxs, fields, stride, flt, sort, verify)
    assert_export(ex, rec, f"{what}: {flt} {sort}", alive_rows=sum(kept))
    if offsets:
        np.testing.assert_array_equal(ex.offsets.cpu().numpy().view(np.uint32), np.concatenate([[0], np.cumsum(kept)]), err_msg=what)
    if partial:
        assert any(0 < k < a for k, a in zip(kept, alive)), (what, flt, kept, alive)
    return ex, kept, alive


def burst_freeze_die_off(cap, n=3):
    """-> a program of n instances after a burst: [full, empty, cap - 1 ...]"""
    ctx, prog, fxs = make_based(cap, n)
    step(ctx, fxs, 0, [cap, 0, max(cap - 1, 1)][:n])
    return ctx, prog, fxs


# ---- capacity and tile edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", SMALL_CAPS + LARGE_CAPS)
def test_capacity_and_tile_edges_all_alive_and_after_a_die_off(cap):
    """Three instances: one full, one EMPTY, one that is FROZEN before the others lose particles. All alive, then after a die-off: a plane through
    the cloud and its inverse, by depth in both directions and by distance; with filters that keep everything the call is the 32-byte form's, with
    a key equal for every row it is hnb_program_export_filtered's - dst, offsets and counts."""
    n = 3
    ctx, prog, fxs = burst_freeze_die_off(cap, n)
    partial = cap >= 63                                                  # (a plane cannot keep part of one particle)
    check(ctx, prog, fxs, f"burst at {cap}", HALF, DEPTH, partial=partial)
    check(ctx, prog, fxs, f"burst at {cap}", dict(HALF, invert=True), NEAR, POS_AGE_LIFE_VEL, 32, offsets=False, partial=partial)
    fxs[2].set_simulated(False)
    for f in (1, 2, 3):
        step(ctx, fxs, f, [0] * n, dt=0.3)
    ctx.synchronize()
    counts = [fx.alive_count() for fx in fxs]
    assert counts[1] == 0 and counts[2] == max(cap - 1, 1) and counts[0] <= cap and (cap < 63 or 0 < counts[0] < cap)
    for flt, sort in ((HALF, DEPTH_DESC), (dict(HALF, invert=True), DEPTH), ([HALF, ALL, dict(HALF, invert=True)], FAR)):
        check(ctx, prog, fxs, f"die-off at {cap}", flt, sort, partial=partial)
    # the two identities
    total = n * cap
    everything = run_prog(Export(POS_AGE_ID, 20, total, n_offsets=n + 1), prog, ALL, DEPTH)
    plain = pes.run_sorted(Export(POS_AGE_ID, 20, total, n_offsets=n + 1), prog, "instance", **DEPTH)
    for fx in fxs:
        fx.write_attr(A.COLOR.id, np.full((cap, 1), 0x80000007, np.uint32))
    const = run_prog(Export(POS_AGE_ID, 20, total, n_offsets=n + 1), prog, HALF, dict(key="attr", attr=A.COLOR.id, descending=True))
    filtered = pef.run_prog(Export(POS_AGE_ID, 20, total, n_offsets=n + 1), prog, HALF)
    ctx.synchronize()
    for got, want in ((everything, plain), (const, filtered)):
        np.testing.assert_array_equal(got.words(), want.words())
        np.testing.assert_array_equal(got.offsets.cpu().numpy(), want.offsets.cpu().numpy())
        assert got.counts() == want.counts()
    assert everything.counts() == [sum(counts)] * 2
    ctx.close()


# ---- instance counts --------------------------------------------------------------------------------------------------------------------------------
def test_three_hundred_instances_take_a_second_round_of_the_offsets_scan():
    cap, n = 64, 300
    ctx, prog, fxs = make(cap, n)
    step(ctx, fxs, 0, [(k * 7) % (cap + 1) for k in range(n)])
    ex, kept, alive = check(ctx, prog, fxs, "300 x 64", HALF, DEPTH, POS_AGE_LIFE_VEL, 32, verify=range(0, n, 37))
    assert sum(kept) > 2000
    flts = [dict(kind="planes", planes=[(1.0, 0.0, -0.5, 0.0)] * (1 + k % 6), invert=bool(k % 5 == 0)) for k in range(n)]
    check(ctx, prog, fxs, "300 x 64, a filter each", flts, NEAR, POS_AGE_ID, 20, verify=range(3, n, 41))
    ctx.close()


def test_five_instances_of_ten_thousand():
    cap, n = 10_000, 5
    ctx, prog, fxs = make_based(cap, n)
    step(ctx, fxs, 0, [cap, cap // 2, cap, cap - 1, 4097])
    for f in (1, 2):
        step(ctx, fxs, f, [0] * n, dt=0.3)
    ctx.synchronize()
    check(ctx, prog, fxs, "5 x 10,000", HALF, DEPTH_DESC)
    ex, kept, alive = check(ctx, prog, fxs, "5 x 10,000", [ALL, NONE, HALF, dict(HALF, invert=True), HALF], NEAR, POS_AGE_LIFE_VEL, 32)
    assert kept[0] == alive[0] > 0 and kept[1] == 0 < alive[1]          # one instance keeps everything and one nothing in the same call
    ctx.close()


# ---- every filter kind, every key -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [4096, 8193])
def test_every_filter_kind_with_every_key(cap):
    """PLANES with one and with six planes, SPHERE, ATTR_RANGE on an f32 and on a u32 attribute, each with invert, shared and per instance
    (differing in n_planes, P and invert); DEPTH, DISTANCE, ATTR on f32 and on u32, ascending and descending; ties by DEPTH with v = 0 and by an
    attribute of four distinct values. One instance keeps everything and one nothing."""
    n = 5
    ctx, prog, fxs = make_based(cap, n, age_cohort=0)
    step(ctx, fxs, 0, [cap, cap // 2, cap, cap - 1, max(cap // 3, 64)])
    for f in (1, 2):
        step(ctx, fxs, f, [0] * n, dt=0.3)
    ctx.synchronize()
    rng = np.random.default_rng(cap)
    for fx in fxs:                                                       # a u32 attribute of four distinct values, one of them above 2^31
        fx.write_attr(A.COLOR.id, np.array([3, 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32)[rng.integers(0, 4, cap)].reshape(cap, 1))
    assert not runtime.ATTR_IS_FLOAT[A.COLOR.id] and runtime.ATTR_IS_FLOAT[A.LIFETIME.id]
    p = fxs[2].read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fxs[2].alive_list()]
    q = lambda c, f: float(np.quantile(p[:, c], f))
    box = [(1, 0, 0, -q(0, 0.15)), (-1, 0, 0, q(0, 0.85)), (0, 1, 0, -q(1, 0.1)), (0, -1, 0, q(1, 0.9)), (0, 0, 1, -q(2, 0.1)), (0, 0, -1, q(2, 0.9))]
    L, COL = A.LIFETIME.id, A.COLOR.id
    planes = [ALL, NONE, dict(kind="planes", planes=box), dict(kind="planes", planes=box[:2], invert=True), HALF]
    spheres = [dict(kind="sphere", sphere=(0, 0, 0, 3e38)), dict(kind="sphere", sphere=(1e6, 0, 0, 0.0)), dict(kind="sphere", sphere=cloud_sphere(fxs[2])),
               dict(kind="sphere", sphere=cloud_sphere(fxs[3], 0.5), invert=True), dict(kind="sphere", sphere=cloud_sphere(fxs[4], -0.3))]
    ranges = [dict(kind="attr_range", attr=L, lo=0.0, hi=10.0), dict(kind="attr_range", attr=L, lo=5.0, hi=10.0), dict(kind="attr_range", attr=L, lo=0.9, hi=1.1),
              dict(kind="attr_range", attr=L, lo=1.0, hi=1.05, invert=True), dict(kind="attr_range", attr=L, lo=0.0, hi=1.0)]
    colors = [dict(kind="attr_range", attr=COL, lo=0, hi=0xFFFFFFFF), dict(kind="attr_range", attr=COL, lo=4, hi=0x7FFFFFFE), dict(kind="attr_range", attr=COL, lo=0x7FFFFFFF, hi=0x80000000),
              dict(kind="attr_range", attr=COL, lo=0x80000000, hi=0xFFFFFFFF, invert=True), dict(kind="attr_range", attr=COL, lo=0, hi=3)]
    keys = [DEPTH, DEPTH_DESC, NEAR, FAR, dict(key="attr", attr=L), dict(key="attr", attr=L, descending=True), dict(key="attr", attr=COL), dict(key="attr", attr=COL, descending=True), TIES]
    shared = [dict(kind="planes", planes=box), dict(kind="planes", planes=box[:1], invert=True), spheres[2], dict(spheres[2], invert=True), ranges[2], dict(ranges[2], invert=True),
              colors[2], dict(colors[2], invert=True)]
    cases = [(flts, keys[i % len(keys)]) for i, flts in enumerate((planes, spheres, ranges, colors))] + [(flt, keys[(i + 4) % len(keys)]) for i, flt in enumerate(shared)]
    cases += [(planes, keys[6]), (spheres, keys[7]), (ranges, TIES), (colors, keys[5]), (HALF, keys[3])]
    used = {tuple(sorted(s.items())) for _, s in cases}
    assert len(used) == len(keys)                                        # every key ran
    runs = [(flt, sort, run_prog(Export(POS_AGE_LIFE_VEL, 32, n * cap, n_offsets=n + 1), prog, flt, sort)) for flt, sort in cases]
    for flt, sort, ex in runs:
        rec, kept, alive = expected_prog(ctx, fxs, POS_AGE_LIFE_VEL, 32, flt, sort)
        assert_export(ex, rec, f"{flt} {sort}", alive_rows=sum(kept))
        np.testing.assert_array_equal(ex.offsets.cpu().numpy().view(np.uint32), np.concatenate([[0], np.cumsum(kept)]))
        assert any(0 < k < a for k, a in zip(kept, alive)), (flt, kept, alive)
        if isinstance(flt, list):
            assert kept[0] == alive[0] > 0 and kept[1] == 0 < alive[1], (flt, kept, alive)
    # the ties are ties: a key of four values over thousands of rows, and the keys of +0 and -0 for DEPTH along the zero vector
    host = Frozen(fxs[0])
    assert len(np.unique(sort_keys(host, host.alive_list(), key="attr", attr=COL))) == 4 and len(np.unique(sort_keys(host, host.alive_list(), **TIES))) <= 2
    ctx.close()


# ---- clamp ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,stride", [(1000, 20), (4097, 32)])
def test_global_clamp_counts_sentinels_and_padding(cap, stride):
    n = 3
    ctx, prog, fxs = make_based(cap, n)
    step(ctx, fxs, 0, [cap, cap // 4, cap])
    ctx.synchronize()
    fields = POS_AGE_ID if stride == 20 else [(A.POSITION.id, 4), (A.AGE.id, 24)]      # stride 32: dwords 0, 4, 5 and 7 are padding
    rec, kept, alive = expected_prog(ctx, fxs, fields, stride, HALF, NEAR)
    total = sum(kept)
    assert all(0 < k < a for k, a in zip(kept, alive))
    if stride == 32:
        assert (rec[:, [0, 4, 5, 7]] == 0).all()
    for K in (0, 1, kept[0] + kept[1] // 2, kept[0] + kept[1], total - 1, total, total + 1):   # nothing | one | inside instance 1 | on a boundary | all but one | exactly | room to spare
        ex = run_prog(Export(fields, stride, K, slack=64, n_offsets=n + 1), prog, HALF, NEAR)
        ctx.synchronize()
        assert ex.counts() == [min(K, total), total], (K, ex.counts())
        assert_export(ex, rec, f"the first {K} records", alive_rows=total)      # ... the first ones of every order; sentinels behind them
        np.testing.assert_array_equal(ex.offsets.cpu().numpy().view(np.uint32), np.concatenate([[0], np.cumsum(kept)]))      # the offsets are those of the kept rows, cut or not
    ex = Export(fields, stride, n * cap)                                 # out_count NULL, out_offsets NULL
    prog.export_filtered_sorted(ex.fields, ex.dst.data_ptr(), stride, n * cap, None, None, filter=HALF, sort=NEAR)
    ctx.synchronize()
    assert ex.counts() == [SENTINEL, SENTINEL]
    np.testing.assert_array_equal(ex.words()[: total * stride // 4].reshape(total, -1), rec)
    assert (ex.words()[total * stride // 4:] == SENTINEL).all()
    ctx.close()


# ---- ring lists -------------------------------------------------------------------------------------------------------------------------------------
def test_ribbon_program_with_ring_lists():
    cap, n = 10_000, 3
    fields = [(A.AGE.id, 0), (A.POSITION.id, 4), (A.RIBBON_ID.id, 16), (A.SIZE.id, 20)]
    asset = effects.ribbon(cap)
    ctx, prog, fxs = make(cap, n, asset, ring_lists=1)
    sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
    for f in range(90):
        dt = 1 / 60
        ctx.frame_begin(dt, f * dt)
        count = sp.tick(dt, rng)
        for k, fx in enumerate(fxs):
            fx.set_frame(count if f % (k + 1) == 0 else 0, frame_seed(f * 16 + k))
        ctx.simulate()
    ctx.synchronize()
    metas = [_device_meta(fx) for fx in fxs]
    assert any((m.list_column >> 1) != 0 and m.alive_count > 256 for m in metas)        # kept as rings, a head somewhere inside the column
    before = [fx.alive_list().copy() for fx in fxs]
    mids = [float(np.median(fx.read_attr(A.AGE.id).reshape(-1)[b])) for fx, b in zip(fxs, before)]
    check(ctx, prog, fxs, "ring, shared", dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=mids[0]), DEPTH, fields, 24)
    check(ctx, prog, fxs, "ring, a range each", [dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=m, invert=bool(k & 1)) for k, m in enumerate(mids)],
          dict(key="attr", attr=A.AGE.id, descending=True), fields, 24)
    for fx, b, m in zip(fxs, before, metas):                             # the lists are what they were
        np.testing.assert_array_equal(fx.alive_list(), b)
        m2 = _device_meta(fx)
        assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


# ---- stale AGE; nothing later changes -----------------------------------------------------------------------------------------------------------------
def test_stale_age_as_field_key_and_source_and_a_twin_that_never_exports():
    """LEAN cohorts: the AGE plane is stale until something materialises it. The program call does, for all instances - when AGE is a record
    field, when it is only the key and when it is only the range's source - and runs here in front of anything else that would. A twin context
    that never exports ends the run bit-identical in lists and planes."""
    cap, n = 10_000, 3
    with_age = [(A.AGE.id, 0), (A.LIFETIME.id, 4), (A.POSITION.id, 8)]
    without_age = [(A.LIFETIME.id, 0), (A.POSITION.id, 4)]
    (ctx, prog, fxs), (tctx, tprog, twins) = [make(cap, n, age_cohort=1) for _ in range(2)]
    assert fxs[0].device_view().stale_attr_mask == 1 << A.AGE.id
    dt = F32(1 / 60)
    young = dict(kind="attr_range", attr=A.AGE.id, lo=float(dt), hi=float(dt + dt + dt))
    for f in range(7):
        for c, e in ((ctx, fxs), (tctx, twins)):
            step(c, e, f, [6000, 3000, 0] if f == 0 else [300, 0, 200], dt=1 / 60)
        if f == 4:
            ex, kept, alive = check(ctx, prog, fxs, "stale AGE as a field", HALF, DEPTH, with_age, 20)
            assert len(np.unique(ex.words()[: kept[0] * 5].reshape(-1, 5)[:, 0])) == 5       # five cohorts of ages, all current
        if f == 5:
            check(ctx, prog, fxs, "stale AGE as the key", HALF, dict(key="attr", attr=A.AGE.id, descending=True), without_age, 16)
        if f == 6:
            ex, kept, alive = check(ctx, prog, fxs, "stale AGE as the source", young, DEPTH_DESC, without_age, 16)
            assert kept == [3 * 300, 0, 3 * 200]                         # the bursts of the last three frames are one, two and three ticks old
    for f in range(7, 15):
        for c, e in ((ctx, fxs), (tctx, twins)):
            step(c, e, f, [0, 100, 0], dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    for fx, twin in zip(fxs, twins):
        d = fx.compare(twin)
        assert d["equal"] == 1, d
        assert fx.check()["ok"] == 1
    ctx.close(); tctx.close()


# ---- interleaving and regrow ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [300, 4097])
def test_twenty_calls_interleaved_with_frames_and_the_sibling_exports_then_a_regrow(cap):
    """Twenty calls with other planes each, frames and the three sibling exports between them, nothing synchronises; the staging buffer of the
    per-instance filters is shared with hnb_program_export_filtered, which runs in between with filters of its own. Every destination is checked
    at the end against the state it was enqueued behind: the frames in between spawn nothing and kill nothing (dt = 0), so that state is one."""
    n = 3
    ctx, prog, fxs = make_based(cap, n)
    step(ctx, fxs, 0, [cap, cap - 1, cap // 2])
    step(ctx, fxs, 1, [0] * n, dt=0.3)
    ctx.synchronize()
    state = [(fx.alive_list().copy(), fx.read_attr(A.POSITION.id).view(np.uint32).copy(), fx.read_attr(A.AGE.id).view(np.uint32).copy()) for fx in fxs]
    p = state[0][1].view(F32).reshape(-1, 3)[state[0][0]].astype(np.float64)
    s = p[:, 0] - 0.5 * p[:, 2]                                         # HALF's plane moved through the cloud: between its 20 % and 80 % quantiles, so it always cuts
    cut = lambda i, k: dict(kind="planes", planes=[(1.0, 0.0, -0.5, -float(np.quantile(s, 0.2 + 0.1 * ((3 * i + 2 * k) % 7))))], invert=bool((i + k) % 3 == 0))
    new = lambda: Export(POS_AGE_ID, 20, n * cap, n_offsets=n + 1)
    calls, filtered, sorted_, single = [], [], [], []
    for i in range(20):
        flts = [cut(i, k) for k in range(n)] if i % 4 else cut(i, 0)
        sort = (DEPTH, NEAR, FAR)[i % 3]
        calls.append((flts, sort, run_prog(new(), prog, flts, sort)))
        if i % 2 == 0:
            step(ctx, fxs, 2 + i, [0] * n, dt=0.0)
        other = [cut(i + 1, 2 - k) for k in range(n)]
        filtered.append((other, pef.run_prog(new(), prog, other)))
        if i % 5 == 0:
            sorted_.append((sort, pes.run_sorted(new(), prog, "instance", **sort)))
            single.append((i % n, flts if i % 4 == 0 else flts[i % n], sort, run_fs(Export(POS_AGE_ID, 20, cap), fxs[i % n], flts if i % 4 == 0 else flts[i % n], sort)))
    ctx.synchronize()
    for fx, (alive, pos, age) in zip(fxs, state):                        # (what this test rests on: the frames in between changed nothing that is exported)
        assert np.array_equal(fx.alive_list(), alive) and np.array_equal(fx.read_attr(A.POSITION.id).view(np.uint32), pos) and np.array_equal(fx.read_attr(A.AGE.id).view(np.uint32), age)
    bases = [fx_slot_base(fx) for fx in fxs]
    seen = set()
    for i, (flts, sort, ex) in enumerate(calls):
        rec, kept, alive = expected_prog(ctx, fxs, POS_AGE_ID, 20, flts, sort)
        assert_export(ex, rec, f"call {i}", alive_rows=sum(kept))
        np.testing.assert_array_equal(ex.offsets.cpu().numpy().view(np.uint32), np.concatenate([[0], np.cumsum(kept)]))
        assert any(0 < k < a for k, a in zip(kept, alive))
        seen.add(tuple(kept))
    assert len(seen) >= 10                                             # the calls did differ
    for other, ex in filtered:
        rec, kept, _ = pef.expected_prog(ctx, fxs, POS_AGE_ID, 20, other)
        assert_export(ex, rec, "hnb_program_export_filtered in between", alive_rows=sum(kept))
    for sort, ex in sorted_:
        assert_export(ex, pes.expected_program(fxs, POS_AGE_ID, 20, "instance", bases, **sort)[0], "hnb_program_export_sorted in between")
    for k, flt, sort, ex in single:
        host = Frozen(fxs[k])
        mask = filter_mask(host, host.alive_list(), **flt)
        order = np.argsort(sort_keys(host, host.alive_list(), **sort)[mask], kind="stable")
        assert_export(ex, expected_records(host, POS_AGE_ID, 20, slot_base=bases[k])[mask][order], "hnb_effect_export_filtered_sorted in between", alive_rows=int(mask.sum()))
    # an instance more: the scratch is regrown
    fx3 = prog.create_effect(slot_base=BASES[3])
    fx3.slot_base_given = BASES[3]
    fxs = fxs + [fx3]
    step(ctx, fxs, 40, [0, 0, 0, cap - 1])
    check(ctx, prog, fxs, "a fourth instance", [cut(1, 0), cut(2, 1), cut(3, 2), HALF], DEPTH)
    check(ctx, prog, fxs, "a fourth instance", HALF, FAR)
    ctx.close()


# ---- the effect form --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [300, 10_000])
def test_the_48_byte_descriptor_through_hnb_effect_export_sorted(cap):
    ctx, prog, fxs = make_based(cap, 2)
    step(ctx, fxs, 0, [cap, cap // 2])
    lib = runtime.load_library()
    for fx, flt, sort in ((fxs[0], HALF, DEPTH), (fxs[1], dict(HALF, invert=True), FAR)):
        want = run_fs(Export(POS_AGE_ID, 20, cap), fx, flt, sort)
        got = Export(POS_AGE_ID, 20, cap)
        d = runtime.export_desc(got.fields, got.dst.data_ptr(), 20, cap, got.cnt.data_ptr())
        sf, keep = runtime.export_sort_filtered(sort, [flt])
        assert lib.hnb_effect_export_sorted(fx._h, C.byref(d), C.cast(C.byref(sf), C.POINTER(runtime.ExportSort))) == 0, lib.hnb_last_error()
        ctx.synchronize()
        np.testing.assert_array_equal(got.words(), want.words())
        assert got.counts() == want.counts() and 0 < got.counts()[1] < fx.alive_count()
        sf2, keep2 = runtime.export_sort_filtered(sort, [flt, flt])      # an effect takes one filter
        bad = Export(POS_AGE_ID, 20, cap)
        d = runtime.export_desc(bad.fields, bad.dst.data_ptr(), 20, cap, bad.cnt.data_ptr())
        for broken in (sf2, _with(sf, reserved2=1), _with(sf, filters=None)):
            assert lib.hnb_effect_export_sorted(fx._h, C.byref(d), C.cast(C.byref(broken), C.POINTER(runtime.ExportSort))) == -1 and len(lib.hnb_last_error()) > 8
        ctx.synchronize()
        assert bad.untouched()
    ctx.close()


def _with(sf, **fields):
    """a copy of an ExportSortFiltered with some members set (the filter array stays the original's)"""
    out = runtime.ExportSortFiltered()
    C.memmove(C.byref(out), C.byref(sf), C.sizeof(sf))
    for name, value in fields.items():
        if name in ("filters", "n_filters", "reserved2"):
            setattr(out, name, value)
        else:
            setattr(out.sort, name, value)
    return out


# ---- argument errors --------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    cap, n = 1000, 3
    ctx, prog, fxs = make_based(cap, n)
    step(ctx, fxs, 0, [cap, 10, cap // 2])
    ex = Export(POS_AGE_LIFE_VEL, 32, n * cap, n_offsets=n + 1)
    call = lambda flt, sort=DEPTH, fields=POS_AGE_LIFE_VEL, dst=None, stride=32, offsets=None: prog.export_filtered_sorted(
        fields, ex.dst.data_ptr() if dst is None else dst, stride, n * cap, ex.cnt.data_ptr(), ex.offsets.data_ptr() if offsets is None else offsets, filter=flt, sort=sort)
    inf = float("inf")
    L = A.LIFETIME.id
    bad_filters = {     # what hnb_program_export_filtered rejects
        "no filter": [],
        "two filters for three instances": [HALF, HALF],
        "four filters for three instances": [HALF] * 4,
        "mixed kinds": [HALF, dict(kind="sphere", sphere=(0, 0, 0, 1)), HALF],
        "mixed attributes": [dict(kind="attr_range", attr=L, lo=0.0, hi=1.0), dict(kind="attr_range", attr=L, lo=0.0, hi=1.0), dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=1.0)],
        "an unknown kind": dict(kind=3),
        "PLANES without a plane": dict(kind="planes", planes=[]),
        "seven planes": dict(kind="planes", planes=[(1, 0, 0, 0)] * 7),
        "SPHERE with n_planes": dict(kind="sphere", planes=[(1, 0, 0, 0)], sphere=(0, 0, 0, 1)),
        "a non-finite squared radius": dict(kind="sphere", sphere=(0, 0, 0, inf)),
        "ATTR_RANGE with a vector attribute": dict(kind="attr_range", attr=A.VELOCITY.id, lo=0.0, hi=1.0),
        "ATTR_RANGE with ID": dict(kind="attr_range", attr=A.ID.id, lo=0, hi=10),
        "lo above hi": dict(kind="attr_range", attr=A.AGE.id, lo=1.0, hi=0.5),
    }
    for what, flt in bad_filters.items():
        with pytest.raises(bh.HanabiError) as ei:
            call(flt)
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    for i, broken in itertools.product(range(n), (dict(kind="planes", planes=[(1, 0, 0, inf)]), dict(kind="planes", planes=[(1, 0, 0, 0)], invert=2))):
        flts = [HALF] * n
        flts[i] = broken
        with pytest.raises(bh.HanabiError) as ei:
            call(flts)
        assert ei.value.code == -1 and f"filters[{i}]" in str(ei.value), (i, str(ei.value))      # the text names the filter
    bad_sorts = {       # what hnb_program_export_sorted rejects
        "an unknown key": dict(key=3),
        "descending above 1": dict(key="depth", v=DIR, descending=2),
        "a direction that is not finite": dict(key="depth", v=(0, inf, 0)),
        "ATTR with a vector attribute": dict(key="attr", attr=A.VELOCITY.id),
        "ATTR with ID": dict(key="attr", attr=A.ID.id),
    }
    for what, sort in bad_sorts.items():
        with pytest.raises(bh.HanabiError) as ei:
            call(HALF, sort)
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    bad_desc = {        # what hnb_program_export rejects
        "PARTICLE_COUNTER": dict(fields=[(A.PARTICLE_COUNTER.id, 0)]),
        "overlapping fields": dict(fields=[(A.POSITION.id, 0), (A.AGE.id, 8)]),
        "a misaligned dst": dict(dst=ex.dst.data_ptr() + 4),
        "a stride above 256": dict(fields=[(A.AGE.id, 0)], stride=260),
        "misaligned out_offsets": dict(offsets=ex.offsets.data_ptr() + 2),
    }
    for what, kw in bad_desc.items():
        with pytest.raises(bh.HanabiError) as ei:
            call(HALF, **kw)
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    # the descriptor itself, through the C call
    lib = runtime.load_library()
    d = runtime.export_desc(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, n * cap, ex.cnt.data_ptr())
    sf, keep = runtime.export_sort_filtered(DEPTH, [HALF])
    as_sort = lambda s: C.cast(C.byref(s), C.POINTER(runtime.ExportSort))
    INSTANCE, PROGRAM = runtime.SORT_SCOPES["instance"], runtime.SORT_SCOPES["program"]
    for what, broken, scope, text in (("filters NULL", _with(sf, filters=None), INSTANCE, b"filters"), ("reserved2", _with(sf, reserved2=1), INSTANCE, b"reserved2"),
                                      ("n_filters 0", _with(sf, n_filters=0), INSTANCE, b"n_filters"), ("n_filters 2", _with(sf, n_filters=2), INSTANCE, b"n_filters"),
                                      ("reserved", _with(sf, reserved=1), INSTANCE, b"reserved"), ("struct_size 28", _with(sf, struct_size=28), INSTANCE, b"struct_size"),
                                      ("struct_size 40", _with(sf, struct_size=40), INSTANCE, b"struct_size"), ("struct_size 52", _with(sf, struct_size=52), INSTANCE, b"struct_size"),
                                      ("the program scope", sf, PROGRAM, b"HNB_SORT_SCOPE_PROGRAM"), ("scope 2", sf, 2, b"scope")):
        assert lib.hnb_program_export_sorted(prog._h, C.byref(d), as_sort(broken), scope, None) == -1 and text in lib.hnb_last_error(), (what, lib.hnb_last_error())
    flt = runtime.export_filter(**HALF)
    for field, value in (("struct_size", 124), ("reserved", 1)):
        setattr(flt, field, value)
        sfb, keepb = runtime.export_sort_filtered(DEPTH, [flt])
        assert lib.hnb_program_export_sorted(prog._h, C.byref(d), as_sort(sfb), INSTANCE, None) == -1 and b"filters[0]" in lib.hnb_last_error(), field
        flt = runtime.export_filter(**HALF)
    d64 = runtime.export_desc(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, n * cap, ex.cnt.data_ptr())
    d64.struct_size = 64
    dflag = runtime.export_desc(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, n * cap, ex.cnt.data_ptr())
    dflag.flags = 1
    for broken in (d64, dflag):
        assert lib.hnb_program_export_sorted(prog._h, C.byref(broken), as_sort(sf), INSTANCE, None) == -1
    assert lib.hnb_program_export_sorted(prog._h, C.byref(d), None, INSTANCE, None) == -1 and b"NULL" in lib.hnb_last_error()
    ctx.synchronize()
    assert ex.untouched() and (ex.offsets.cpu().numpy().view(np.uint32) == SENTINEL).all()
    call(HALF)                                                           # ... and the same arguments, unbroken, are accepted
    rec, kept, _ = expected_prog(ctx, fxs, POS_AGE_LIFE_VEL, 32, HALF, DEPTH)
    assert_export(ex, rec, "after the refusals", alive_rows=sum(kept))
    ctx.close()
