"""hnb_effect_export_filtered_sorted on the GPU (include/hanabi_amd.h "Packed output", Filtered, then sorted export): record r of the caller's buffer =
the kept particle with the r-th smallest key, ties in list order. Expected records are built on the host as the tests of the two parent calls build
them: expected_records(...)[mask] (the mask restated in numpy binary32 from the header's predicates), stably sorted by the numpy keys of the kept
rows. Everything is compared bit for bit: every result is uniquely determined, there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, GpuRunner, assert_same_state, frame_seed
from test_export_filtered_abi import FMA_P, FMA_PLANE, FMA_SPHERE, FMA_SPHERE_P
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, _device_meta, assert_export, expected_records, step
from test_gpu_export_filtered import ALL, BOUNDARY_X, HALF, NONE, cloud_sphere, filter_mask, rows_as_x, run_filtered
from test_gpu_export_sorted import DIR, adversarial_x, burst_then_die_off, key_f32, make, run_sorted, sort_keys, varying_bytes

pytestmark = pytest.mark.gpu

TILE = 4096                                     # rows per workgroup of the filter and of the sort; capacities up to it take the one-workgroup kernel
CAPS = (300, 4096, 4097, 10_000, 135_245)       # partial tile | exactly one tile | first multi-tile, last tile of one row | three ragged tiles | 33 tiles + 77: past a group of 32
F32 = np.float32
DEPTH, DEPTH_DESC = dict(key="depth", v=DIR), dict(key="depth", v=DIR, descending=True)
NEAR = dict(key="distance", v=(1, 2, 3))


class Frozen:
    """The host's read-back of an effect, read once: what filter_mask, sort_keys and expected_records ask of an effect, for many (filter, sort)
    pairs on one state. (Synchronises when it reads; make a new one after a frame or a write_attr.)"""

    def __init__(self, fx):
        self._fx, self._alive, self._planes, self.capacity = fx, fx.alive_list().copy(), {}, fx.capacity

    def alive_list(self):
        return self._alive

    def read_attr(self, attr):
        if int(attr) not in self._planes:
            self._planes[int(attr)] = self._fx.read_attr(attr)
        return self._planes[int(attr)]


def run_fs(ex, fx, flt, sort):
    fx.export_filtered_sorted(ex.fields, ex.dst.data_ptr(), ex.stride, ex.capacity, ex.cnt.data_ptr(), filter=flt, sort=sort)
    return ex


def expected_fs(host, fields, stride, flt, sort):
    """-> (records, mask over the list, keys of the kept rows in list order, their stable order)"""
    alive = host.alive_list()
    mask = filter_mask(host, alive, **flt)
    k = sort_keys(host, alive, **sort)[mask]
    order = np.argsort(k, kind="stable")
    return expected_records(host, fields, stride)[mask][order], mask, k, order


def check_fs(ctx, fx, what, flt, sort, fields=POS_AGE_LIFE_VEL, stride=32, capacity=None, host=None):
    """export, synchronise, compare; -> (mask, kept keys, order)"""
    ex = run_fs(Export(fields, stride, fx.capacity if capacity is None else capacity), fx, flt, sort)
    ctx.synchronize()
    rec, mask, k, order = expected_fs(host or Frozen(fx), fields, stride, flt, sort)
    assert_export(ex, rec, f"{what} {flt} {sort}", alive_rows=int(mask.sum()))
    return mask, k, order


def check_many(ctx, fx, what, pairs, fields=POS_AGE_LIFE_VEL, stride=32):
    """Every (filter, sort) of `pairs` enqueued back to back, one synchronisation, one read-back; -> [(mask, kept keys, order)]"""
    runs = [run_fs(Export(fields, stride, fx.capacity), fx, flt, sort) for flt, sort in pairs]
    ctx.synchronize()
    host, out = Frozen(fx), []
    for (flt, sort), ex in zip(pairs, runs):
        rec, mask, k, order = expected_fs(host, fields, stride, flt, sort)
        assert_export(ex, rec, f"{what} {flt} {sort}", alive_rows=int(mask.sum()))
        out.append((mask, k, order))
    return out


# ---- 1. edges of both tilings -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_edges_of_both_tilings_and_the_two_identities(cap):
    """Alive counts 0, 1, 255..257, 4095..4097 and everything, reached by spawning: a plane through the cloud, the same inverted, keep-none and
    keep-all, by depth in both directions. Keep-all is hnb_effect_export_sorted's buffer word for word; a key that is constant over the kept rows
    (a constant u32 plane) gives hnb_effect_export_filtered's."""
    ctx, fx = make(cap)
    f, have = 0, 0
    filters = (HALF, dict(HALF, invert=True), NONE, ALL)
    const_key = dict(key="attr", attr=A.COLOR.id)
    for want in [c for c in (0, 1, 255, 256, 257, 4095, 4096, 4097) if c <= cap] + [cap]:
        if want > have:
            step(ctx, fx, f, want - have)
            f += 1
            have = want
        fx.write_attr(A.COLOR.id, np.full((cap, 1), 0x80000007, np.uint32))             # (spawns initialise COLOR: written again behind every one of them)
        runs = {(i, desc): run_fs(Export(POS_AGE_LIFE_VEL, 32, cap), fx, flt, dict(DEPTH, descending=desc)) for i, flt in enumerate(filters) for desc in (False, True)}
        sorted_runs = [run_sorted(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **dict(DEPTH, descending=desc)) for desc in (False, True)]
        const_runs = [run_fs(Export(POS_AGE_LIFE_VEL, 32, cap), fx, HALF, dict(const_key, descending=desc)) for desc in (False, True)]
        filtered = run_filtered(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **HALF)
        ctx.synchronize()
        host = Frozen(fx)
        what = f"capacity {cap}, {want} alive"
        assert len(host.alive_list()) == want
        for (i, desc), ex in runs.items():
            rec, mask, k, order = expected_fs(host, POS_AGE_LIFE_VEL, 32, filters[i], dict(DEPTH, descending=desc))
            assert_export(ex, rec, f"{what}, filter {i}, descending={desc}", alive_rows=int(mask.sum()))
            assert (i != 2 or not mask.any()) and (i != 3 or mask.all())
        for desc in (False, True):                                                       # keep-all: the sorted export's buffer, sentinels and counts included
            np.testing.assert_array_equal(runs[(3, desc)].words(), sorted_runs[desc].words(), err_msg=what)
            assert runs[(3, desc)].counts() == sorted_runs[desc].counts() == [want, want]
            np.testing.assert_array_equal(const_runs[desc].words(), filtered.words(), err_msg=what)      # a constant key: the filtered export's
            assert const_runs[desc].counts() == filtered.counts()
        half = filter_mask(host, host.alive_list(), **HALF)
        assert filtered.counts() == [int(half.sum())] * 2
        if want > 64:
            assert 0.2 < half.mean() < 0.8, half.mean()                                  # the plane does cut the cloud
            assert not np.array_equal(expected_fs(host, POS_AGE_LIFE_VEL, 32, HALF, DEPTH)[3], np.arange(int(half.sum())))       # and the keys do reorder what is kept
    ctx.close()


# ---- 2. kept counts chosen exactly ------------------------------------------------------------------------------------------------------------------
def _x_at_least(t):
    return dict(kind="planes", planes=[(1, 0, 0, -float(t))])           # x - t >= 0


# keys that scramble rows whose x is the row index, of which the last `kept` are kept: the distance from a point inside the kept range folds the rows
# round it; LIFETIME is random with ties
def _scramblers(cap, kept):
    return (dict(key="distance", v=(cap - kept * 0.39, 0, 0)), dict(key="attr", attr=A.LIFETIME.id, descending=True))


@pytest.mark.parametrize("cap", [4096, 10_000])
def test_kept_counts_at_the_edges_of_a_gather_tile_and_of_a_sort_tile(cap):
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    rows_as_x(fx, cap, np.arange(cap, dtype=F32))
    host = Frozen(fx)
    for kept in [K for K in (0, 1, 255, 256, 257, 4095, 4096, 4097) if K <= cap]:
        for sort in _scramblers(cap, kept):
            mask, k, order = check_fs(ctx, fx, f"{kept} kept of {cap}", _x_at_least(cap - kept), sort, host=host)
            assert int(mask.sum()) == kept and mask[cap - kept:].all()
            if kept > 64:
                assert not np.array_equal(order, np.arange(kept))
    ctx.close()


def test_kept_counts_round_a_group_of_sort_tiles_and_kept_rows_spread_over_the_input_tiles():
    """135 245 slots: 131 071..131 073 kept rows (32 sort tiles, one row less and one more); every third row; only the last row of every input tile."""
    cap = 135_245
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    rows_as_x(fx, cap, np.arange(cap, dtype=F32))
    host = Frozen(fx)
    by_life = _scramblers(cap, cap)[1]
    for kept, which in ((131_071, 0), (131_072, 1), (131_073, 0)):
        mask, k, order = check_fs(ctx, fx, f"{kept} kept", _x_at_least(cap - kept), _scramblers(cap, kept)[which], host=host)
        assert int(mask.sum()) == kept and not np.array_equal(order, np.arange(kept))
    r = np.arange(cap)
    rows_as_x(fx, cap, (r % 3 == 0).astype(F32))
    (mask, k, order), _ = check_many(ctx, fx, "every third row", [(_x_at_least(1), by_life), (_x_at_least(1), dict(key="attr", attr=A.LIFETIME.id))])
    np.testing.assert_array_equal(np.flatnonzero(mask), np.arange(0, cap, 3))
    rows_as_x(fx, cap, (r % TILE == TILE - 1).astype(F32))
    (mask, k, order), (inv_mask, _, _) = check_many(ctx, fx, "last rows", [(_x_at_least(1), by_life), (dict(_x_at_least(1), invert=True), by_life)])
    np.testing.assert_array_equal(np.flatnonzero(mask), np.arange(TILE - 1, cap, TILE))
    assert int(mask.sum()) == 33 and int(inv_mask.sum()) == cap - 33 and not np.array_equal(order, np.arange(33))
    ctx.close()


# ---- 3. stability and adversarial keys on the kept subset --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [4096, 10_000, 135_245])
def test_adversarial_keys_and_stability_on_the_kept_subset(cap):
    """The key is x itself (depth along (1, 0, 0), y = z = -0); the filter is a range of LIFETIME, which is random and independent of x: about half of
    every pattern is kept. Ties stay in list order in both directions (the expectation is a stable argsort of the kept keys)."""
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    alive = fx.alive_list()
    assert len(alive) == cap
    flt = dict(kind="attr_range", attr=A.LIFETIME.id, lo=0.9, hi=1.1)
    passes = {}
    for name, xbits in adversarial_x(cap).items():
        pos = np.full((cap, 3), F32(-0.0).view(np.uint32), np.uint32)
        pos[alive, 0] = xbits
        fx.write_attr(A.POSITION.id, pos)
        asc, desc = check_many(ctx, fx, f"{name} at {cap}", [(flt, dict(key="depth", v=(1, 0, 0))), (flt, dict(key="depth", v=(1, 0, 0), descending=True))])
        mask, k, order = asc
        assert 0.3 < mask.mean() < 0.7
        np.testing.assert_array_equal(k, key_f32(xbits[mask]), err_msg=name)            # the key is x itself
        np.testing.assert_array_equal(desc[1], ~key_f32(xbits[mask]), err_msg=name)
        passes[name] = varying_bytes(k)
        if name == "one value":
            assert np.array_equal(order, np.arange(len(k))) and np.array_equal(desc[2], np.arange(len(k)))      # list order, ascending and descending
        if name == "four values":
            ties = np.bincount(np.unique(k, return_inverse=True)[1])
            assert len(ties) == 4 and ties.min() > cap // 16
            for o in (order, desc[2]):                                                   # inside a run of equal keys the list rows ascend, in both directions
                kk = (k if o is order else desc[1])[o]
                assert (np.diff(o)[kk[1:] == kk[:-1]] > 0).all()
    assert passes["one value"] == [] and passes["lowest byte"] == [0] and passes["highest byte"] == [3]
    assert passes["bytes 0 and 3"] == [0, 3] and passes["bytes 0, 1 and 3"] == [0, 1, 3] and passes["specials"] == [0, 1, 2, 3]
    ctx.close()


# ---- 4. every predicate kind x every key kind ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [3000, 135_245])
def test_every_predicate_kind_with_every_key_kind(cap):
    ctx, fx = make(cap, age_cohort=0)
    step(ctx, fx, 0, cap)
    for f in range(1, 4):
        step(ctx, fx, f, 0, dt=0.3)                                     # the burst has spread, some are gone: a partial, permuted list; positions and keys are finite
    ctx.synchronize()
    rng = np.random.default_rng(cap)
    color = (0x7FFFFFFF + rng.integers(-300, 300, cap).astype(np.int64)).astype(np.uint32)
    color[::7] = 0x80000000
    color[5::11] = 0xFFFFFFFF
    color[6::13] = 0
    fx.write_attr(A.COLOR.id, color.reshape(cap, 1))
    n = fx.alive_count()
    assert 0 < n < cap
    p = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fx.alive_list()]
    assert np.isfinite(p).all()
    q = lambda c, f: float(np.quantile(p[:, c], f))
    skew = float(np.quantile(p.astype(np.float64) @ np.array([0.1, 0.2, 1.0]), 0.1))
    box = [(1, 0, 0, -q(0, 0.15)), (-1, 0, 0, q(0, 0.85)), (0, 1, 0, -q(1, 0.1)), (0, -1, 0, q(1, 0.9)), (0.1, 0.2, 1, -skew), (0, 0, -1, q(2, 0.9))]
    filters = [HALF, dict(kind="planes", planes=box), dict(kind="planes", planes=box, invert=True), dict(kind="sphere", sphere=cloud_sphere(fx)),
               dict(kind="sphere", sphere=cloud_sphere(fx, 0.5), invert=True), dict(kind="attr_range", attr=A.LIFETIME.id, lo=0.9, hi=1.1),
               dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=10.0, invert=True), dict(kind="attr_range", attr=A.COLOR.id, lo=0x80000000, hi=0xFFFFFFFF)]
    sorts = [DEPTH, DEPTH_DESC, NEAR, dict(NEAR, descending=True), dict(key="attr", attr=A.LIFETIME.id), dict(key="attr", attr=A.AGE.id, descending=True),
             dict(key="attr", attr=A.COLOR.id), dict(key="attr", attr=A.COLOR.id, descending=True)]
    fields = [(A.COLOR.id, 0), (A.POSITION.id, 4), (A.AGE.id, 16), (A.LIFETIME.id, 20)]
    out = check_many(ctx, fx, f"capacity {cap}", [(flt, sort) for flt in filters for sort in sorts], fields=fields, stride=24)
    for (flt, sort), (mask, k, order) in zip([(flt, sort) for flt in filters for sort in sorts], out):
        if flt["kind"] == "attr_range" and flt["attr"] == A.AGE.id:
            assert not mask.any()                                        # every age is inside [0, 10]: inverted, nothing is kept
        else:
            assert 0.02 < mask.mean() < 0.98, (flt, mask.mean())
            if sort.get("attr") != A.AGE.id:                             # (one burst: every age is the same, the AGE key leaves the list order)
                assert not np.array_equal(order, np.arange(len(order))), (flt, sort)
    # +-0, +-inf, NaNs of both signs and denormals, where the bits are the stored ones: AGE as the ATTR key and as the ATTR_RANGE source
    alive = fx.alive_list()
    age = np.zeros(cap, np.uint32)
    age[alive] = BOUNDARY_X[(np.arange(n) * 7) % len(BOUNDARY_X)]
    fx.write_attr(A.AGE.id, age.view(F32).reshape(cap, 1))
    by_age, by_age_desc = dict(key="attr", attr=A.AGE.id), dict(key="attr", attr=A.AGE.id, descending=True)
    ranges = [dict(kind="attr_range", attr=A.AGE.id, lo=0xFF800000, hi=0x7F800000), dict(kind="attr_range", attr=A.AGE.id, lo=0xFF800000, hi=0x7F800000, invert=True),     # the numbers | the NaNs
              dict(kind="attr_range", attr=A.AGE.id, lo=0x80000000, hi=0x00000001), dict(kind="attr_range", attr=A.AGE.id, lo=0xFFFFFFFF, hi=0x7FFFFFFF)]               # -0, +0, a denormal | everything
    out = check_many(ctx, fx, "edge values", [(flt, sort) for flt in ranges for sort in (by_age, by_age_desc, DEPTH)] + [(HALF, by_age), (HALF, by_age_desc)], fields=fields, stride=24)
    assert out[9][0].all() and 0 < out[3][0].sum() < n and 0 < out[6][0].sum() < n
    ctx.close()


# ---- 5. products that a fused multiply-add would round differently --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [300, 10_000])
def test_predicate_and_key_are_rounded_operation_by_operation(cap):
    """The triples of tests/test_export_filtered_abi.py, in the predicate and in the key at once. Depth along (a, b, 1) of FMA_P is 0 operation by
    operation and 2^-24 fused; the rows between them hold (0, 0, 2^-25), whose depth is 2^-25: FMA_P's rows come first, fused they would come last.
    The squared distance of FMA_SPHERE_P from the origin is 1 + 2^-11 exactly, the value of (1, 2^-6, 2^-6): all ties, list order; fused it would
    be an ulp more and its rows would follow the others. The filters are the same planes and sphere: fused, they would keep other rows."""
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    alive = fx.alive_list()
    even = np.arange(cap) % 2 == 0
    plane = dict(kind="planes", planes=[tuple(float(c) for c in FMA_PLANE)])
    depth = dict(key="depth", v=(float(FMA_PLANE[0]), float(FMA_PLANE[1]), 1.0))
    pos = np.zeros((cap, 3), F32)
    pos[alive[0::2]] = FMA_P
    pos[alive[1::2]] = (0.0, 0.0, 2.0 ** -25)
    fx.write_attr(A.POSITION.id, pos)
    kept_none, kept_all = check_many(ctx, fx, "the plane", [(plane, depth), (dict(plane, invert=True), depth)])
    assert not kept_none[0].any() and kept_all[0].all()                  # every row is 2^-25 behind the plane operation by operation; fused, FMA_P's would be in front
    mask, k, order = kept_all
    np.testing.assert_array_equal(order, np.concatenate([np.flatnonzero(even), np.flatnonzero(~even)]))     # depth 0 (FMA_P, in list order), then depth 2^-25
    assert set(k[even]) == {int(key_f32(F32(0).view(np.uint32)))} and set(k[~even]) == {int(key_f32(F32(2.0 ** -25).view(np.uint32)))}
    sphere = dict(kind="sphere", sphere=tuple(float(c) for c in FMA_SPHERE))
    pos[alive[0::2]] = FMA_SPHERE_P
    pos[alive[1::2]] = (1.0, 2.0 ** -6, 2.0 ** -6)
    fx.write_attr(A.POSITION.id, pos)
    for desc in (False, True):
        mask, k, order = check_fs(ctx, fx, "the sphere", sphere, dict(key="distance", v=(0, 0, 0), descending=desc))
        assert mask.all() and len(set(k)) == 1                           # every row exactly at the radius, every key equal
        np.testing.assert_array_equal(order, np.arange(cap))
    ctx.close()


# ---- 6. list shapes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [10_000, 135_245])
def test_permuted_partial_list_after_a_die_off(cap):
    ctx, fx = burst_then_die_off(cap)
    alive = fx.alive_list()
    assert 0 < len(alive) < cap and not np.array_equal(alive, np.arange(len(alive)))
    fields = [(A.ID.id, 0), (A.POSITION.id, 4), (A.AGE.id, 16)]
    pairs = [(HALF, DEPTH), (dict(HALF, invert=True), dict(NEAR, descending=True)), (dict(kind="sphere", sphere=cloud_sphere(fx, 0.3)), NEAR),
             (dict(kind="attr_range", attr=A.LIFETIME.id, lo=1.0, hi=1.15), dict(key="attr", attr=A.AGE.id))]
    for mask, k, order in check_many(ctx, fx, f"die-off at {cap}", pairs, fields=fields, stride=20):
        assert 0 < mask.sum() < len(alive)
    ex = run_fs(Export(fields, 20, cap), fx, HALF, DEPTH)
    ctx.synchronize()
    ids = ex.words()[: ex.counts()[0] * 5].reshape(-1, 5)[:, 0]
    rec, mask, k, order = expected_fs(Frozen(fx), fields, 20, HALF, DEPTH)
    np.testing.assert_array_equal(ids, alive[mask][order])              # the kept slots, in key order
    ctx.close()


def test_permuted_list_of_a_rate_spawner_churn():
    cap = 135_245
    ctx, fx = make(cap, effects.firework_trails(cap, spawner=bh.SpawnerSettings.rate(3000.0)))
    rng = np.random.default_rng(5)
    for f in range(60):
        step(ctx, fx, f, int(rng.integers(1000, 6000)), dt=1 / 20)
    alive = fx.alive_list()
    assert 4 * TILE < len(alive) < cap and not np.array_equal(alive, np.sort(alive))
    pairs = [(HALF, DEPTH_DESC), (dict(kind="sphere", sphere=cloud_sphere(fx), invert=True), NEAR), (dict(kind="attr_range", attr=A.AGE.id, lo=0.1, hi=0.5), dict(key="attr", attr=A.LIFETIME.id))]
    for mask, k, order in check_many(ctx, fx, "churn", pairs, fields=[(A.ID.id, 0), (A.POSITION.id, 4)], stride=16):
        assert 0 < mask.sum() < len(alive)
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
    mid = float(np.median(fx.read_attr(A.AGE.id).reshape(-1)[before]))
    young = dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=mid)
    oldest_first = dict(key="attr", attr=A.AGE.id, descending=True)
    out = check_many(ctx, fx, "ring", [(young, oldest_first), (dict(young, invert=True), oldest_first), (ALL, oldest_first), (young, DEPTH)], fields=fields, stride=24)
    assert 0.2 < out[0][0].mean() < 0.8 and not np.array_equal(out[0][2], np.arange(len(out[0][2])))       # (the ribbon's own order is youngest first)
    np.testing.assert_array_equal(fx.alive_list(), before)              # the list is what it was
    m2 = _device_meta(fx)
    assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


# ---- 7. top-K ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [3000, 10_000])
def test_top_k_counts_and_sentinels(cap):
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0)
    ctx.synchronize()
    host = Frozen(fx)
    rec, mask, k, order = expected_fs(host, POS_AGE_LIFE_VEL, 32, HALF, NEAR)
    kept = len(rec)
    assert 256 < kept < cap - 256
    runs = [(K, run_fs(Export(POS_AGE_LIFE_VEL, 32, K, slack=64), fx, HALF, NEAR)) for K in (0, 1, 255, kept - 1, kept, kept + 1, cap)]
    ctx.synchronize()
    for K, ex in runs:
        assert ex.counts() == [min(K, kept), kept], (K, ex.counts())
        assert_export(ex, rec, f"the nearest {K} kept rows", alive_rows=kept)          # the first K of the order, sentinels behind them
    assert (runs[0][1].words() == SENTINEL).all()
    ex = Export(POS_AGE_LIFE_VEL, 32, cap)                                              # out_count NULL: accepted, the records are the same
    fx.export_filtered_sorted(ex.fields, ex.dst.data_ptr(), 32, cap, None, filter=HALF, sort=NEAR)
    ctx.synchronize()
    assert ex.counts() == [SENTINEL, SENTINEL]
    np.testing.assert_array_equal(ex.words()[: kept * 8].reshape(kept, 8), rec)
    assert (ex.words()[kept * 8:] == SENTINEL).all()
    ctx.close()


# ---- 8. stale AGE ---------------------------------------------------------------------------------------------------------------------------------------
def test_stale_age_is_current_as_field_key_and_range_source_and_nothing_later_changes():
    """LEAN cohorts: the AGE plane is stale until something materialises it. The call does - when AGE is only a record field, only the key, only the
    source of the range; a twin that never exports ends the run in the same state."""
    cap = 100_000
    with_age = [(A.AGE.id, 0), (A.LIFETIME.id, 4), (A.POSITION.id, 8)]
    without_age = [(A.LIFETIME.id, 0), (A.POSITION.id, 4)]
    pairs = [make(cap, age_cohort=1) for _ in range(2)]
    (ctx, fx), (tctx, twin) = pairs
    assert fx.device_view().stale_attr_mask == 1 << A.AGE.id
    dt = F32(1 / 60)
    recent = dict(kind="attr_range", attr=A.AGE.id, lo=float(dt), hi=float(dt + dt + dt))
    youngest_first = dict(key="attr", attr=A.AGE.id)                     # (the list is oldest first: this key moves every row)
    cases = [("a field", with_age, 20, HALF, DEPTH), ("the key", without_age, 16, HALF, youngest_first), ("the range source", without_age, 16, recent, DEPTH)]
    keep = []
    for f in range(5):
        for c, e in pairs:
            step(c, e, f, 70_000 if f == 0 else 3000, dt=1 / 60)
        if f >= 3:                                                       # no materialise call in front of them
            keep.append([run_fs(Export(fields, stride, cap), fx, flt, sort) for what, fields, stride, flt, sort in cases])
    ctx.synchronize()
    host = Frozen(fx)
    for (what, fields, stride, flt, sort), ex in zip(cases, keep[-1]):   # the last frame's three, against the read-back (which materialises for itself)
        rec, mask, k, order = expected_fs(host, fields, stride, flt, sort)
        assert_export(ex, rec, f"stale AGE as {what}", alive_rows=int(mask.sum()))
        if what == "a field":
            assert len(np.unique(rec[:, 0])) == 5                        # five cohorts of ages, all current
        if what == "the key":
            assert len(np.unique(k)) == 5 and not np.array_equal(order, np.arange(len(order)))
        if what == "the range source":
            assert int(mask.sum()) == 3 * 3000                           # the bursts of frames 4, 3 and 2 are one, two and three ticks old
    assert keep[0][2].counts() == [3 * 3000] * 2                         # a frame earlier: the bursts of frames 1, 2 and 3
    for f in range(5, 12):
        for c, e in pairs:
            step(c, e, f, 0, dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    d = fx.compare(twin)
    assert d["equal"] == 1, d
    assert fx.check()["ok"] == 1
    ctx.close(); tctx.close()


# ---- 9. the call disturbs nothing ---------------------------------------------------------------------------------------------------------------------
def test_the_call_disturbs_nothing():
    """A twin context that never exports is bit-identical after further frames; a plain export behind the call is in list order."""
    cap = 10_000
    asset = effects.firework_trails(cap)
    a, b = GpuRunner(asset), GpuRunner(asset)
    for r in (a, b):
        step(r.ctx, r.fx, 0, cap)
        for f in range(1, 5):
            step(r.ctx, r.fx, f, 0, dt=0.25)
    ctx, fx = a.ctx, a.fx
    ctx.synchronize()
    alive, dead = fx.alive_list().copy(), fx.dead_list().copy()
    assert 0 < len(alive) < cap
    first = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    c1 = run_fs(Export(POS_AGE_LIFE_VEL, 32, cap), fx, HALF, DEPTH_DESC)
    second = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    c2 = run_fs(Export(POS_AGE_LIFE_VEL, 32, cap), fx, dict(HALF, invert=True), NEAR)
    third = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    ctx.synchronize()
    host = Frozen(fx)
    rec = expected_records(host, POS_AGE_LIFE_VEL, 32)
    for ex in (first, second, third):
        assert_export(ex, rec, "plain export round the calls: list order")
    for ex, flt, sort in ((c1, HALF, DEPTH_DESC), (c2, dict(HALF, invert=True), NEAR)):
        want, mask, k, order = expected_fs(host, POS_AGE_LIFE_VEL, 32, flt, sort)
        assert_export(ex, want, "between them", alive_rows=int(mask.sum()))
    np.testing.assert_array_equal(fx.alive_list(), alive)
    np.testing.assert_array_equal(fx.dead_list(), dead)
    for f in range(5, 25):
        for r in (a, b):
            step(r.ctx, r.fx, f, 300 if f % 4 == 0 else 0, dt=1 / 20)
    a.ctx.synchronize(); b.ctx.synchronize()
    assert_same_state(b.state(), a.state(), "the twin that never exported")
    assert fx.compare(b.fx)["equal"] == 1
    a.ctx.close(); b.ctx.close()


# ---- 10. scratch in stream order ------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_share_the_scratch_in_stream_order():
    """Different filters and sorts into different destinations with no synchronisation between the calls, on effects of both launch paths in one
    context."""
    ctx = bh.Context(0)
    fxs = []
    for cap in (TILE, 10_000):
        prog = ctx.create_program(bh.lower(effects.firework_trails(cap)))
        fxs += [prog.create_effect(), prog.create_effect()]
    ctx.frame_begin(1 / 60, 0.0)
    for i, fx in enumerate(fxs):
        fx.set_frame(fx.capacity - 100 * i, frame_seed(i))
    ctx.simulate()
    pairs = [(HALF, DEPTH), (dict(kind="sphere", sphere=(0, 0, 0, 1e-4), invert=True), dict(NEAR, descending=True)), (dict(kind="attr_range", attr=A.LIFETIME.id, lo=0.8, hi=1.0), dict(key="attr", attr=A.LIFETIME.id)),
             (NONE, DEPTH), (dict(HALF, invert=True), dict(key="depth", v=(0, 1, 0))), (ALL, NEAR)]
    runs = [(fx, flt, sort, run_fs(Export(POS_AGE_LIFE_VEL, 32, fx.capacity), fx, flt, sort)) for fx in fxs for flt, sort in pairs]      # twenty-four, nothing waits in between
    ctx.synchronize()
    hosts = {id(fx): Frozen(fx) for fx in fxs}
    for fx, flt, sort, ex in runs:
        rec, mask, k, order = expected_fs(hosts[id(fx)], POS_AGE_LIFE_VEL, 32, flt, sort)
        assert_export(ex, rec, f"capacity {fx.capacity}, effect {fx.index()}, {flt} {sort}", alive_rows=int(mask.sum()))
    ctx.close()


@pytest.mark.parametrize("cap", [4097, 300], ids=["two_tiles", "one_workgroup"])
def test_interleaved_with_the_sorted_and_the_filtered_export_on_one_effect(cap):
    """The three calls own three scratch allocations: enqueued alternately on one effect with no synchronisation, each is right."""
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0)
    other = dict(HALF, invert=True)
    calls = [("cull", run_fs(Export(POS_AGE_LIFE_VEL, 32, cap), fx, HALF, DEPTH), HALF, DEPTH),
             ("sorted", run_sorted(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **NEAR), None, NEAR),
             ("filtered", run_filtered(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **other), other, None),
             ("cull", run_fs(Export(POS_AGE_LIFE_VEL, 48, cap), fx, other, NEAR), other, NEAR),
             ("filtered", run_filtered(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **HALF), HALF, None),
             ("sorted", run_sorted(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **DEPTH_DESC), None, DEPTH_DESC),
             ("cull", run_fs(Export(POS_AGE_LIFE_VEL, 32, cap), fx, HALF, DEPTH_DESC), HALF, DEPTH_DESC)]
    ctx.synchronize()
    host = Frozen(fx)
    for what, ex, flt, sort in calls:
        if sort is None:                                                 # the filtered export: the kept rows in list order
            mask = filter_mask(host, host.alive_list(), **flt)
            rec = expected_records(host, POS_AGE_LIFE_VEL, ex.stride)[mask]
        else:                                                            # (ALL keeps every finite position: the sorted export is the call with it)
            rec, mask, k, order = expected_fs(host, POS_AGE_LIFE_VEL, ex.stride, flt or ALL, sort)
        assert_export(ex, rec, f"{what} at {cap}", alive_rows=int(mask.sum()))
        assert 0 < mask.sum() <= cap
    ctx.close()


# ---- 11. argument errors ----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    """Every argument error of either parent call and each NULL argument: -1 with text, nothing enqueued - the sentinel buffer is unchanged after a
    synchronise. (PLANES / SPHERE / DEPTH / DISTANCE on a layout without POSITION cannot be reached: the lowering refuses such an asset.)"""
    cap = 1000
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    step(ctx, fx, 0, cap)
    ex = Export(POS_AGE_LIFE_VEL, 32, cap)
    call = lambda fields=POS_AGE_LIFE_VEL, dst=None, stride=32, flt=HALF, sort=DEPTH: fx.export_filtered_sorted(fields, ex.dst.data_ptr() if dst is None else dst, stride, cap, ex.cnt.data_ptr(), filter=flt, sort=sort)
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
    inf, nan = float("inf"), float("nan")
    bad_filter = {     # every case hnb_effect_export_filtered adds
        "an unknown kind": dict(kind=3),
        "invert above 1": dict(kind="planes", planes=[(1, 0, 0, 0)], invert=2),
        "PLANES without a plane": dict(kind="planes", planes=[]),
        "PLANES with seven planes": dict(kind="planes", planes=[(1, 0, 0, 0)] * 7),
        "SPHERE with n_planes": dict(kind="sphere", planes=[(1, 0, 0, 0)], sphere=(0, 0, 0, 1)),
        "ATTR_RANGE with n_planes": dict(kind="attr_range", planes=[(1, 0, 0, 0)], attr=A.AGE.id, lo=0.0, hi=1.0),
        "an infinite plane coefficient": dict(kind="planes", planes=[(1, 0, 0, 0), (0, inf, 0, 1)]),
        "a NaN plane offset": dict(kind="planes", planes=[(1, 0, 0, nan)]),
        "a non-finite centre": dict(kind="sphere", sphere=(0, -inf, 0, 1)),
        "a non-finite squared radius": dict(kind="sphere", sphere=(0, 0, 0, inf)),
        "ATTR_RANGE with an attribute the layout lacks": dict(kind="attr_range", attr=A.SIZE.id, lo=0.0, hi=1.0),
        "ATTR_RANGE with a vector attribute": dict(kind="attr_range", attr=A.VELOCITY.id, lo=0.0, hi=1.0),
        "ATTR_RANGE with ID": dict(kind="attr_range", attr=A.ID.id, lo=0, hi=10),
        "ATTR_RANGE with PARTICLE_COUNTER": dict(kind="attr_range", attr=A.PARTICLE_COUNTER.id, lo=0, hi=10),
        "ATTR_RANGE with an unknown attribute": dict(kind="attr_range", attr=39, lo=0, hi=10),
        "lo above hi, f32": dict(kind="attr_range", attr=A.AGE.id, lo=1.0, hi=0.5),
        "lo above hi in the key order: +0 above -0": dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=-0.0),
        "lo above hi, u32 unsigned": dict(kind="attr_range", attr=A.COLOR.id, lo=0x80000000, hi=0x7FFFFFFF),
    }
    bad_sort = {       # every case hnb_effect_export_sorted adds
        "an unknown key": dict(key=3),
        "descending above 1": dict(key="depth", v=DIR, descending=2),
        "ATTR with an attribute the layout lacks": dict(key="attr", attr=A.SIZE.id),
        "ATTR with a vector attribute": dict(key="attr", attr=A.VELOCITY.id),
        "ATTR with ID": dict(key="attr", attr=A.ID.id),
        "ATTR with PARTICLE_COUNTER": dict(key="attr", attr=A.PARTICLE_COUNTER.id),
        "ATTR with an unknown attribute": dict(key="attr", attr=39),
        "DEPTH with an infinite direction": dict(key="depth", v=(0, inf, 1)),
        "DEPTH with a NaN direction": dict(key="depth", v=(nan, 0, 1)),
        "DISTANCE from a non-finite point": dict(key="distance", v=(0, 0, -inf)),
    }
    for what, kw in list(bad_desc.items()) + [(w, dict(flt=f)) for w, f in bad_filter.items()] + [(w, dict(sort=s)) for w, s in bad_sort.items()]:
        with pytest.raises(bh.HanabiError) as ei:
            call(**kw)
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    lib = runtime.load_library()
    d = runtime.export_desc(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, cap, ex.cnt.data_ptr())
    flt, srt = runtime.export_filter(**HALF), runtime.export_sort(**DEPTH)
    good = [fx._h, C.byref(d), C.byref(flt), C.byref(srt)]
    for i in range(4):
        args = list(good)
        args[i] = None
        assert lib.hnb_effect_export_filtered_sorted(*args) == -1 and b"NULL" in lib.hnb_last_error(), i
    for struct, broken in ((flt, (("struct_size", 124), ("reserved", 1))), (srt, (("struct_size", 28), ("reserved", 1))), (d, (("struct_size", 64), ("flags", 1)))):
        for field, value in broken:
            keep = getattr(struct, field)
            setattr(struct, field, value)
            assert lib.hnb_effect_export_filtered_sorted(*good) == -1 and len(lib.hnb_last_error()) > 8, (type(struct).__name__, field)
            setattr(struct, field, keep)
    ctx.synchronize()
    assert ex.untouched()
    assert lib.hnb_effect_export_filtered_sorted(*good) == 0             # ... and the same arguments, unbroken, are accepted
    ctx.synchronize()
    rec, mask, k, order = expected_fs(Frozen(fx), POS_AGE_LIFE_VEL, 32, HALF, DEPTH)
    assert_export(ex, rec, "after the refusals", alive_rows=int(mask.sum()))
    ctx.close()
