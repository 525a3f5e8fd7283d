"""hnb_effect_export_filtered on the GPU (include/hanabi_amd.h "Packed output", Filtered export): record r of the caller's buffer = the r-th row of the
alive list that the filter keeps. Expected records are built on the host as tests/test_gpu_export.py builds them (read_attr + alive_list()), the
mask restated in numpy binary32 / uint32 from the header's formulas (tests/test_export_filtered_abi.py, where the same restatement is held against
the C++ the kernels call). Everything is compared bit for bit: every result is uniquely determined, there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, GpuRunner, assert_same_state, frame_seed
from test_export_filtered_abi import FMA_P, FMA_PLANE, FMA_SPHERE, FMA_SPHERE_P, pass_planes, pass_range, pass_sphere
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, _device_meta, assert_export, expected_records, step
import test_gpu_program_export_sorted as pes
from test_gpu_export_sorted import DIR, burst_then_die_off, expected_sorted, make, run_sorted

pytestmark = pytest.mark.gpu

TILE = 4096                                     # rows per workgroup of mark / compact; capacities up to it take the one-launch path
CAPS = (300, 4096, 4097, 10_000, 135_245)       # partial tile | exactly one tile | first multi-tile, last tile of one row | three ragged tiles | 33 tiles + 77
F32 = np.float32
HALF = dict(kind="planes", planes=[(1.0, 0.0, -0.5, 0.0)])           # a plane through the y axis: the firework bursts at the origin and falls along y, x and z stay symmetric
ALL = dict(kind="planes", planes=[(0, 0, 0, 1)])                     # s = 1 for every finite position
NONE = dict(kind="planes", planes=[(0, 0, 0, -1)])
ONE, INF, NAN = 0x3F800000, 0x7F800000, 0x7FC00000


def filter_mask(fx, alive, kind, planes=(), sphere=None, attr=0, lo=0, hi=0, invert=False):
    """Which rows of the list the header's predicate keeps: binary32 operations one by one, in the order the header writes them."""
    if kind == "attr_range":
        bits = fx.read_attr(attr).view(np.uint32).reshape(-1)[alive]
        m = pass_range(bits, runtime.ATTR_IS_FLOAT[int(attr)], runtime._scalar_bits(lo), runtime._scalar_bits(hi))
    else:
        p = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[alive]
        m = pass_planes(p, planes) if kind == "planes" else pass_sphere(p, sphere)
    return ~m if invert else m


def cloud_sphere(fx, shift=0.0):
    """(cx, cy, cz, r^2) of a sphere that keeps about half of what is alive: round the cloud's median point, moved along x by `shift` times the
    cloud's size, with the median squared distance from that centre. (The fraction is only ever asserted loosely; the mask is the restatement's.)"""
    p = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fx.alive_list()].astype(np.float64)
    c = np.median(p, axis=0)
    c[0] += shift * np.sqrt(np.median(((p - c) ** 2).sum(1)))
    c = c.astype(F32).astype(np.float64)
    return (float(c[0]), float(c[1]), float(c[2]), float(F32(np.median(((p - c) ** 2).sum(1)))))


def run_filtered(ex, fx, **flt):
    fx.export_filtered(ex.fields, ex.dst.data_ptr(), ex.stride, ex.capacity, ex.cnt.data_ptr(), **flt)
    return ex


def expected_filtered(fx, fields, stride, slot_base=0, **flt):
    alive = fx.alive_list()
    mask = filter_mask(fx, alive, **flt)
    return expected_records(fx, fields, stride, slot_base)[mask], mask


def check_filtered(ctx, fx, what, fields=POS_AGE_LIFE_VEL, stride=32, capacity=None, **flt):
    """export, synchronise, compare; -> the mask over the list"""
    ex = run_filtered(Export(fields, stride, fx.capacity if capacity is None else capacity), fx, **flt)
    ctx.synchronize()
    rec, mask = expected_filtered(fx, fields, stride, **flt)
    assert_export(ex, rec, f"{what} {flt}", alive_rows=int(mask.sum()))
    return mask


# ---- tile and scan edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_tile_and_scan_edges(cap):
    """Alive counts 0, 1, 255..257, 4095..4097 and everything, reached by spawning: a plane through the cloud with both values of invert, a filter
    that keeps nothing, and one that keeps everything - whose buffer is hnb_effect_export's byte for byte."""
    ctx, fx = make(cap)
    f, have = 0, 0
    for want in [c for c in (0, 1, 255, 256, 257, 4095, 4096, 4097) if c <= cap] + [cap]:
        if want > have:
            step(ctx, fx, f, want - have)
            f += 1
            have = want
        runs = [run_filtered(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **flt) for flt in (HALF, dict(HALF, invert=True), NONE, ALL)]
        plain = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
        ctx.synchronize()
        alive = fx.alive_list()
        rec = expected_records(fx, POS_AGE_LIFE_VEL, 32)
        assert len(rec) == want
        half = filter_mask(fx, alive, **HALF)
        what = f"capacity {cap}, {want} alive"
        assert_export(runs[0], rec[half], what + ", half", alive_rows=int(half.sum()))
        assert_export(runs[1], rec[~half], what + ", the other half", alive_rows=int((~half).sum()))
        assert_export(runs[2], rec[:0], what + ", none", alive_rows=0)
        assert_export(runs[3], rec, what + ", all")
        assert_export(plain, rec, what + ", plain")
        np.testing.assert_array_equal(runs[3].words(), plain.words())                 # the whole buffers, sentinels included
        assert runs[3].counts() == plain.counts() == [want, want]
        if want > 64:
            assert 0.2 < half.mean() < 0.8, half.mean()                              # the plane does cut the cloud
    ctx.close()


def rows_as_x(fx, cap, x_of_row):
    """POSITION = (x_of_row[r], 0, 0) for the particle in list row r (everything is alive); -> the x written, in list order"""
    alive = fx.alive_list()
    assert len(alive) == cap
    pos = np.zeros((cap, 3), F32)
    pos[alive, 0] = x_of_row
    fx.write_attr(A.POSITION.id, pos)
    return alive


def test_output_tile_edges():
    """Kept counts of exactly 255, 256 and 257 (an output tile of the gather holds 256 records), and 4095..4097 (what one input tile can keep): x = the
    row index, the plane x <= c."""
    cap = 10_000
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    rows_as_x(fx, cap, np.arange(cap, dtype=F32))
    for kept in (255, 256, 257, 4095, 4096, 4097):
        mask = check_filtered(ctx, fx, f"{kept} kept", kind="planes", planes=[(-1, 0, 0, kept - 1)])      # -x + (kept - 1) >= 0
        assert int(mask.sum()) == kept and mask[:kept].all()
        mask = check_filtered(ctx, fx, f"all but {kept} kept", kind="planes", planes=[(-1, 0, 0, kept - 1)], invert=True)
        assert int(mask.sum()) == cap - kept and mask[kept:].all()
    ctx.close()


def test_only_the_last_row_of_every_input_tile_is_kept():
    cap = 135_245
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    r = np.arange(cap)
    rows_as_x(fx, cap, (r % TILE == TILE - 1).astype(F32))
    mask = check_filtered(ctx, fx, "last rows", kind="planes", planes=[(1, 0, 0, -1)])
    np.testing.assert_array_equal(np.flatnonzero(mask), np.arange(TILE - 1, cap, TILE))
    assert int(mask.sum()) == cap // TILE == 33
    mask = check_filtered(ctx, fx, "first rows", kind="sphere", sphere=(1, 0, 0, 0), invert=True)        # everything but them: d = (x - 1)^2 <= 0 only at x == 1
    assert int(mask.sum()) == cap - 33
    ctx.close()


# ---- every predicate kind -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [3000, 135_245])
def test_every_predicate_kind(cap):
    ctx, fx = make(cap, age_cohort=0)
    step(ctx, fx, 0, cap)
    for f in range(1, 4):
        step(ctx, fx, f, 0, dt=0.3)                                     # the burst has spread; lifetimes are 0.8 .. 1.2 s, some are gone: a partial, permuted list
    ctx.synchronize()
    n = fx.alive_count()
    p = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fx.alive_list()]
    ages = fx.read_attr(A.AGE.id).reshape(-1)[fx.alive_list()]
    q = lambda c, f: float(np.quantile(p[:, c], f))
    skew = float(np.quantile(p.astype(np.float64) @ np.array([0.1, 0.2, 1.0]), 0.1))
    box = [(1, 0, 0, -q(0, 0.15)), (-1, 0, 0, q(0, 0.85)), (0, 1, 0, -q(1, 0.1)), (0, -1, 0, q(1, 0.9)), (0.1, 0.2, 1, -skew), (0, 0, -1, q(2, 0.9))]      # a skewed box inside the cloud
    for flt in (HALF, dict(kind="planes", planes=box[:2]), dict(kind="planes", planes=box), dict(kind="planes", planes=box, invert=True),
                dict(kind="sphere", sphere=cloud_sphere(fx)), dict(kind="sphere", sphere=cloud_sphere(fx, 0.5), invert=True),
                dict(kind="attr_range", attr=A.LIFETIME.id, lo=0.9, hi=1.1), dict(kind="attr_range", attr=A.LIFETIME.id, lo=0.9, hi=1.1, invert=True),
                dict(kind="attr_range", attr=A.AGE.id, lo=float(ages.min()), hi=float(ages.max())), dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=float(np.nextafter(ages.min(), F32(0))))):
        mask = check_filtered(ctx, fx, f"capacity {cap}", **flt)
        if flt["kind"] != "attr_range" or flt["attr"] != A.AGE.id:
            assert 0.02 < mask.mean() < 0.98, (flt, mask.mean())       # every one of these filters does filter
    assert 0 < n < cap
    ctx.close()


@pytest.mark.parametrize("cap", [3000, 10_000])
def test_u32_attribute_range_is_unsigned(cap):
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
    got = color[fx.alive_list()]
    for lo, hi in ((0x80000000, 0xFFFFFFFF), (0x80000000, 0xFFFFFFFE), (0, 0x7FFFFFFF), (0x7FFFFFFF, 0x80000000), (0x80000000, 0x80000000), (0, 0xFFFFFFFF), (1, 0x7FFFFFFE)):
        for inv in (False, True):
            mask = check_filtered(ctx, fx, "COLOR", fields=fields, stride=16, kind="attr_range", attr=A.COLOR.id, lo=lo, hi=hi, invert=inv)
            np.testing.assert_array_equal(mask, ((got.astype(np.int64) >= lo) & (got.astype(np.int64) <= hi)) != inv)      # unsigned: 0x80000000 is above 0x7FFFFFFF
    ctx.close()


# ---- exact boundaries -------------------------------------------------------------------------------------------------------------------------------
BOUNDARY_X = np.array([ONE - 1, ONE, ONE + 1, 0xBF800000 - 1, 0xBF800000, 0xBF800000 + 1,         # one ulp either side of 1 and of -1
                       0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000,   # +-0, denormals, FLT_MIN
                       INF, 0xFF800000, NAN, 0xFFC00000, 0x7F800001, 0x7F7FFFFF, 0xFF7FFFFF,     # +-inf, NaNs of both signs, +-FLT_MAX
                       0x3F000000 - 1, 0x3F000000, 0x3F000000 + 1, 0x40000000 - 1, 0x40000000, 0x40000000 + 1], np.uint32)      # round 0.5 and 2


@pytest.mark.parametrize("cap", [300, 10_000])
def test_exact_boundaries_in_position(cap):
    """x cycles through the edge values (in one wave, in every tile); y = z = 0, so the plane (1, 0, 0, -1) sees s = x - 1 and the unit sphere
    d = x * x. Then the same values in y behind a ZERO coefficient: 0 * inf and 0 * NaN are NaN, the row does not pass."""
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    xbits = BOUNDARY_X[np.arange(cap) % len(BOUNDARY_X)]
    alive = rows_as_x(fx, cap, xbits.view(F32))
    x = xbits.view(F32)
    with np.errstate(all="ignore"):
        on_or_inside = x >= F32(1)
    for inv in (False, True):
        mask = check_filtered(ctx, fx, "x >= 1", kind="planes", planes=[(1, 0, 0, -1)], invert=inv)
        np.testing.assert_array_equal(mask, on_or_inside != inv)                       # s == 0 passes, one ulp below does not, +inf does, NaN does not
        mask = check_filtered(ctx, fx, "x >= 0", kind="planes", planes=[(1, 0, 0, 0)], invert=inv)
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(mask, (x >= F32(0)) != inv)                  # -0 and +0 alike
        mask = check_filtered(ctx, fx, "unit sphere", kind="sphere", sphere=(0, 0, 0, 1), invert=inv)
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(mask, (x * x <= F32(1)) != inv)              # exactly at the radius passes; inf and NaN do not
        check_filtered(ctx, fx, "sphere of radius 0 round -0", kind="sphere", sphere=(-0.0, 0, 0, 0), invert=inv)
    kept = check_filtered(ctx, fx, "x >= 1", kind="planes", planes=[(1, 0, 0, -1)])
    nan_rows = np.isnan(x)
    assert nan_rows.any() and not kept[nan_rows].any()
    assert check_filtered(ctx, fx, "x >= 1, inverted", kind="planes", planes=[(1, 0, 0, -1)], invert=True)[nan_rows].all()       # with invert a NaN is kept
    pos = np.zeros((cap, 3), F32)
    pos[alive, 0] = 2.0
    pos[alive, 1] = x
    fx.write_attr(A.POSITION.id, pos)
    mask = check_filtered(ctx, fx, "y behind a zero coefficient", kind="planes", planes=[(1, 0, 0, -1)])
    np.testing.assert_array_equal(mask, np.isfinite(x))
    ctx.close()


@pytest.mark.parametrize("cap", [300, 10_000])
def test_products_that_a_fused_multiply_add_would_round_differently(cap):
    """The operands of tests/test_export_filtered_abi.py whose fused evaluation gives the other answer, on the device: the plane's row fails and the
    sphere's row sits exactly at the radius, as operation-by-operation rounding says - the kernels contract nothing."""
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    alive = fx.alive_list()
    pos = np.zeros((cap, 3), F32)
    pos[alive[0::2]] = FMA_P
    pos[alive[1::2]] = FMA_SPHERE_P
    fx.write_attr(A.POSITION.id, pos)
    even = np.arange(cap) % 2 == 0
    planes = [tuple(float(c) for c in FMA_PLANE)]
    mask = check_filtered(ctx, fx, "the plane", kind="planes", planes=planes)
    assert not mask[even].any()                                          # (x*a + y*b) + d = 0 - 2^-25 < 0; fused it would be 2^-24 - 2^-25 > 0
    assert check_filtered(ctx, fx, "the plane, inverted", kind="planes", planes=planes, invert=True)[even].all()
    mask = check_filtered(ctx, fx, "the sphere", kind="sphere", sphere=tuple(float(c) for c in FMA_SPHERE))
    assert mask[~even].all()                                             # ex*ex + ey*ey == r^2 exactly; fused it would be one ulp outside
    ctx.close()


@pytest.mark.parametrize("cap", [300, 10_000])
def test_exact_boundaries_in_the_attribute(cap):
    """AGE written with the edge values: the bounds themselves are kept, one ulp outside is not; -0 is below +0; the infinities bound every number
    and no NaN; the NaNs of both signs are the ends of the whole order."""
    ctx, fx = make(cap, age_cohort=0)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    alive = fx.alive_list()
    bits = BOUNDARY_X[np.arange(cap) % len(BOUNDARY_X)]
    age = np.zeros(cap, np.uint32)
    age[alive] = bits
    fx.write_attr(A.AGE.id, age.view(F32).reshape(cap, 1))
    fields = [(A.AGE.id, 0), (A.POSITION.id, 4)]
    v = bits.view(F32)
    number = ~np.isnan(v)
    cases = {
        (0x3F000000, 0x40000000): number & (v >= F32(0.5)) & (v <= F32(2)),
        (0x80000000, 0x00000000): (bits == 0) | (bits == 0x80000000),                                 # [-0, +0]: both zeros, nothing else
        (0x00000000, 0x00000000): bits == 0,                                                          # [+0, +0]: -0 is outside
        (0xFF800000, INF): number,                                                                    # [-inf, +inf]
        (0xFFFFFFFF, 0x7FFFFFFF): np.ones(cap, bool),                                                 # the whole order
        (INF, 0x7FFFFFFF): (bits & 0x7FFFFFFF >= INF) & (bits >> 31 == 0),                            # +inf and the positive NaNs
        (0x80000001, 0x00000001): (bits == 0) | (bits == 0x80000000) | (bits == 1) | (bits == 0x80000001),      # denormals are numbers
    }
    with np.errstate(all="ignore"):
        for (lo, hi), want in cases.items():
            for inv in (False, True):
                mask = check_filtered(ctx, fx, "AGE", fields=fields, stride=16, kind="attr_range", attr=A.AGE.id, lo=lo, hi=hi, invert=inv)
                np.testing.assert_array_equal(mask, want != inv, err_msg=f"[{lo:08x}, {hi:08x}] invert={inv}")
    ctx.close()


# ---- lists ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [10_000, 135_245])
def test_permuted_partial_list_after_a_die_off(cap):
    ctx, fx = burst_then_die_off(cap)
    alive = fx.alive_list()
    assert 0 < len(alive) < cap and not np.array_equal(alive, np.arange(len(alive)))
    fields = [(A.ID.id, 0), (A.POSITION.id, 4), (A.AGE.id, 16)]
    for flt in (HALF, dict(HALF, invert=True), dict(kind="sphere", sphere=cloud_sphere(fx, 0.3)), dict(kind="attr_range", attr=A.LIFETIME.id, lo=1.0, hi=1.15)):
        mask = check_filtered(ctx, fx, f"die-off at {cap}", fields=fields, stride=20, **flt)
        assert 0 < mask.sum() < len(alive)
    ex = run_filtered(Export(fields, 20, cap), fx, **HALF)
    ctx.synchronize()
    ids = ex.words()[: ex.counts()[0] * 5].reshape(-1, 5)[:, 0]
    np.testing.assert_array_equal(ids, alive[filter_mask(fx, alive, **HALF)])                       # record order is list order: the slots, in the list's sequence
    ctx.close()


def test_permuted_list_of_a_rate_spawner_churn():
    cap = 135_245
    ctx, fx = make(cap, effects.firework_trails(cap, spawner=bh.SpawnerSettings.rate(3000.0)))
    rng = np.random.default_rng(5)
    for f in range(60):
        step(ctx, fx, f, int(rng.integers(1000, 6000)), dt=1 / 20)
    alive = fx.alive_list()
    assert 4 * TILE < len(alive) < cap and not np.array_equal(alive, np.sort(alive))
    fields = [(A.ID.id, 0), (A.POSITION.id, 4)]
    for flt in (HALF, dict(kind="sphere", sphere=cloud_sphere(fx), invert=True), dict(kind="attr_range", attr=A.AGE.id, lo=0.1, hi=0.5)):
        mask = check_filtered(ctx, fx, "churn", fields=fields, stride=16, **flt)
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
    ages = fx.read_attr(A.AGE.id).reshape(-1)[before]
    mid = float(np.median(ages))
    for flt in (dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=mid), dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=mid, invert=True), ALL):
        mask = check_filtered(ctx, fx, "ring", fields=fields, stride=24, **flt)
        assert mask.any()
    assert 0.2 < filter_mask(fx, before, kind="attr_range", attr=A.AGE.id, lo=0.0, hi=mid).mean() < 0.8
    np.testing.assert_array_equal(fx.alive_list(), before)              # the list is what it was
    m2 = _device_meta(fx)
    assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


# ---- clamp and counts -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [3000, 10_000])
def test_clamp_counts_and_sentinels(cap):
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0)
    ctx.synchronize()
    rec, mask = expected_filtered(fx, POS_AGE_LIFE_VEL, 32, **HALF)
    kept = len(rec)
    assert 256 < kept < cap - 256
    for K in (0, 1, kept - 1, kept, kept + 1):
        ex = run_filtered(Export(POS_AGE_LIFE_VEL, 32, K, slack=64), fx, **HALF)
        ctx.synchronize()
        assert ex.counts() == [min(K, kept), kept], (K, ex.counts())
        assert_export(ex, rec, f"first {K} kept rows", alive_rows=kept)    # the first K kept rows of list order, sentinels behind them
    # out_count NULL: accepted, the records are the same
    ex = Export(POS_AGE_LIFE_VEL, 32, cap)
    fx.export_filtered(ex.fields, ex.dst.data_ptr(), 32, cap, None, **HALF)
    ctx.synchronize()
    assert ex.counts() == [SENTINEL, SENTINEL]
    np.testing.assert_array_equal(ex.words()[: kept * 8].reshape(kept, 8), rec)
    assert (ex.words()[kept * 8:] == SENTINEL).all()
    ctx.close()


# ---- stale AGE, no disturbance --------------------------------------------------------------------------------------------------------------------
def test_stale_age_is_current_as_field_and_as_source_and_nothing_later_changes():
    """LEAN cohorts: the AGE plane is stale until something materialises it. The filtered export does - when AGE is a record field, and when it is
    only the source of the range (no AGE among the fields); a twin context that never exports ends the run in the same state."""
    cap = 100_000
    with_age = [(A.AGE.id, 0), (A.LIFETIME.id, 4), (A.POSITION.id, 8)]
    without_age = [(A.LIFETIME.id, 0), (A.POSITION.id, 4)]
    pairs = [make(cap, age_cohort=1) for _ in range(2)]
    (ctx, fx), (tctx, twin) = pairs
    assert fx.device_view().stale_attr_mask == 1 << A.AGE.id
    dt = F32(1 / 60)
    keep = []
    for f in range(5):
        for c, e in pairs:
            step(c, e, f, 70_000 if f == 0 else 3000, dt=1 / 60)
        if f >= 3:                                                       # no materialise call in front of them
            keep.append((f, run_filtered(Export(with_age, 20, cap), fx, **HALF), run_filtered(Export(without_age, 16, cap), fx, kind="attr_range", attr=A.AGE.id, lo=float(dt), hi=float(dt + dt + dt))))
    ctx.synchronize()
    f, by_field, by_source = keep[-1]                                    # the last frame's two, against the read-back (which materialises for itself)
    rec, mask = expected_filtered(fx, with_age, 20, **HALF)
    assert len(np.unique(rec[:, 0])) == 5                                # five cohorts of ages, all current
    assert_export(by_field, rec, "stale AGE as a field", alive_rows=int(mask.sum()))
    rec, mask = expected_filtered(fx, without_age, 16, kind="attr_range", attr=A.AGE.id, lo=float(dt), hi=float(dt + dt + dt))
    assert int(mask.sum()) == 3 * 3000, int(mask.sum())                  # the bursts of frames 4, 3 and 2 are one, two and three ticks old (a particle ages in its first frame)
    assert_export(by_source, rec, "stale AGE as the source", alive_rows=int(mask.sum()))
    assert keep[0][2].counts() == [3 * 3000] * 2                         # a frame earlier: the bursts of frames 1, 2 and 3
    for f in range(5, 12):
        for c, e in pairs:
            step(c, e, f, 0, dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    d = fx.compare(twin)
    assert d["equal"] == 1, d
    assert fx.check()["ok"] == 1
    ctx.close(); tctx.close()


def test_filtered_export_disturbs_nothing():
    """A twin that never exports is bit-identical after further frames; a plain export behind a filtered one is in list order; a sorted export behind
    it, and a filtered one behind that, are right: the two scratch allocations do not alias."""
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
    sort = dict(key="depth", v=(0.3, -0.5, 0.8), descending=True)
    first = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    f1 = run_filtered(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **HALF)
    second = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    s1 = run_sorted(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **sort)
    f2 = run_filtered(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **dict(HALF, invert=True))
    s2 = run_sorted(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **sort)
    ctx.synchronize()
    rec = expected_records(fx, POS_AGE_LIFE_VEL, 32)
    half = filter_mask(fx, alive, **HALF)
    assert_export(first, rec, "plain export in front")
    assert_export(second, rec, "plain export behind: list order")
    assert_export(f1, rec[half], "filtered", alive_rows=int(half.sum()))
    assert_export(f2, rec[~half], "filtered behind a sorted export", alive_rows=int((~half).sum()))
    srt = expected_sorted(fx, POS_AGE_LIFE_VEL, 32, **sort)[0]
    assert_export(s1, srt, "sorted behind a filtered export")
    assert_export(s2, srt, "sorted behind another")
    np.testing.assert_array_equal(fx.alive_list(), alive)
    np.testing.assert_array_equal(fx.dead_list(), dead)
    for f in range(5, 25):
        for r in (a, b):
            step(r.ctx, r.fx, f, 300 if f % 4 == 0 else 0, dt=1 / 20)
    a.ctx.synchronize(); b.ctx.synchronize()
    assert_same_state(b.state(), a.state(), "the twin that never exported")
    assert fx.compare(b.fx)["equal"] == 1
    a.ctx.close(); b.ctx.close()


def test_back_to_back_exports_share_the_scratch_in_stream_order():
    """Three filters into three destinations with no synchronisation between the calls, on an effect of each launch path in one context."""
    ctx = bh.Context(0)
    fxs = []
    for cap in (TILE, 10_000):
        prog = ctx.create_program(bh.lower(effects.firework_trails(cap)))
        fxs += [prog.create_effect(), prog.create_effect()]
    ctx.frame_begin(1 / 60, 0.0)
    for i, fx in enumerate(fxs):
        fx.set_frame(fx.capacity - 100 * i, frame_seed(i))
    ctx.simulate()
    filters = [HALF, dict(kind="sphere", sphere=(0, 0, 0, 1e-4), invert=True), dict(kind="attr_range", attr=A.LIFETIME.id, lo=0.8, hi=1.0), NONE, dict(HALF, invert=True)]
    runs = []
    for fx in fxs:                                                      # five exports per effect, twenty in all, nothing waits in between
        for flt in filters:
            runs.append((fx, flt, run_filtered(Export(POS_AGE_LIFE_VEL, 32, fx.capacity), fx, **flt)))
    ctx.synchronize()
    for fx, flt, ex in runs:
        rec, mask = expected_filtered(fx, POS_AGE_LIFE_VEL, 32, **flt)
        assert_export(ex, rec, f"capacity {fx.capacity}, effect {fx.index()}, {flt}", alive_rows=int(mask.sum()))
    ctx.close()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    """Every refusal of the contract but one: PLANES / SPHERE on a layout without POSITION cannot be reached from here, because the lowering refuses
    an asset whose layout lacks POSITION - no program of that kind can be created to export from."""
    cap = 1000
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    step(ctx, fx, 0, cap)
    ex = Export(POS_AGE_LIFE_VEL, 32, cap)
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
            fx.export_filtered(kw.get("fields", POS_AGE_LIFE_VEL), kw.get("dst", ex.dst.data_ptr()), kw.get("stride", 32), cap, ex.cnt.data_ptr(), **HALF)
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    inf, nan = float("inf"), float("nan")
    bad_filter = {
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
    for what, flt in bad_filter.items():
        with pytest.raises(bh.HanabiError) as ei:
            fx.export_filtered(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, cap, ex.cnt.data_ptr(), **flt)
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    lib = runtime.load_library()
    d = runtime.export_desc(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, cap, ex.cnt.data_ptr())
    flt = runtime.export_filter(**HALF)
    assert lib.hnb_effect_export_filtered(fx._h, C.byref(d), None) == -1 and lib.hnb_effect_export_filtered(fx._h, None, C.byref(flt)) == -1
    for field, value in (("struct_size", 124), ("reserved", 1)):
        keep = getattr(flt, field)
        setattr(flt, field, value)
        assert lib.hnb_effect_export_filtered(fx._h, C.byref(d), C.byref(flt)) == -1 and len(lib.hnb_last_error()) > 8, field
        setattr(flt, field, keep)
    for field, value in (("struct_size", 64), ("flags", 1)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert lib.hnb_effect_export_filtered(fx._h, C.byref(d), C.byref(flt)) == -1, field
        setattr(d, field, keep)
    ctx.synchronize()
    assert ex.untouched()
    assert lib.hnb_effect_export_filtered(fx._h, C.byref(d), C.byref(flt)) == 0       # ... and the same arguments, unbroken, are accepted
    ctx.synchronize()
    rec, mask = expected_filtered(fx, POS_AGE_LIFE_VEL, 32, **HALF)
    assert_export(ex, rec, "after the refusals", alive_rows=int(mask.sum()))
    ctx.close()


# ---- every form on one context ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [4097, 300], ids=["two_sort_tiles", "one_workgroup"])
def test_every_export_form_interleaved_on_one_context(cap):
    """One context, one program of three instances with 37, 0 and `cap` particles alive: the five entry points enqueued behind each other with no
    synchronisation between them, then the first three again on another instance and with records of other sizes. Every result is the host's
    restatement bit for bit: the forms share one table of kernel handles over three code objects, one launch plan and the scratch buffers, and
    none of that may carry over from a call into the next. 4097: two tiles of the sort and the filter, the second of one row; 300: the
    one-workgroup paths."""
    bases = [0, 10_000, 20_000]
    ctx, prog, fxs = pes.make(cap, 3, slot_bases=bases)
    pes.step(ctx, fxs, 0, [37, 0, cap])
    for f in (1, 2, 3):
        pes.step(ctx, fxs, f, [0, 0, 0])
    F, ID = POS_AGE_LIFE_VEL, pes.POS_AGE_ID
    by_depth, by_distance = dict(key="depth", v=DIR), dict(key="distance", v=(1, 2, 3), descending=True)
    full, few = fxs[2], fxs[0]
    calls = [("plain effect", Export(F, 32, cap).run(full)),
             ("program sorted, program scope", pes.run_sorted(Export(ID, 20, 3 * cap), prog, "program", **by_depth)),
             ("filtered effect", run_filtered(Export(F, 32, cap), full, **HALF)),
             ("program plain", Export(ID, 20, 3 * cap, n_offsets=4).run(prog)),
             ("effect sorted", run_sorted(Export(F, 32, cap), full, **by_distance)),
             ("program sorted, instance scope", pes.run_sorted(Export(ID, 20, 3 * cap, n_offsets=4), prog, "instance", **by_distance)),
             ("plain effect again", Export(F, 256, cap).run(few)),
             ("program sorted, program scope, again", pes.run_sorted(Export(ID, 72, 3 * cap), prog, "program", **by_distance)),
             ("filtered effect again", run_filtered(Export(F, 48, cap), few, invert=True, **HALF))]
    ctx.synchronize()
    counts = [fx.alive_count() for fx in fxs]
    assert counts == [37, 0, cap]
    offsets = np.concatenate([[0], np.cumsum(counts)])
    filtered_full, mask_full = expected_filtered(full, F, 32, **HALF)
    filtered_few, mask_few = expected_filtered(few, F, 48, invert=True, **HALF)
    assert 0 < mask_full.sum() < cap
    want = [expected_records(full, F, 32),
            pes.expected_program(fxs, ID, 20, "program", bases, **by_depth)[0],
            filtered_full,
            np.concatenate([expected_records(fx, ID, 20, slot_base=b) for fx, b in zip(fxs, bases)]),
            expected_sorted(full, F, 32, **by_distance)[0],
            pes.expected_program(fxs, ID, 20, "instance", bases, **by_distance)[0],
            expected_records(few, F, 256),
            pes.expected_program(fxs, ID, 72, "program", bases, **by_distance)[0],
            filtered_few]
    for (what, ex), rec in zip(calls, want):
        assert_export(ex, rec, what, alive_rows=len(rec))
        if ex.offsets is not None:
            np.testing.assert_array_equal(ex.offsets.cpu().numpy().view(np.uint32), offsets, err_msg=what)
    ctx.close()
