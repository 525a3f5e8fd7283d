"""hnb_program_export_filtered on the GPU (include/hanabi_amd.h "Packed output", Filtered export, program form): the layout of hnb_program_export,
instance k's segment byte for byte what hnb_effect_export_filtered(effect k, the filter of k) writes. The expected buffer of every case IS that:
the per-effect calls' records, read back and concatenated. The kept sets are checked independently against the numpy binary32 restatement of
hnb_filter_pred.h (tests/test_export_filtered_abi.py). Everything is compared bit for bit: there is no tolerance anywhere. Every case but the
deliberate keep-all / keep-none ones asserts that some instance keeps part of what is alive."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, frame_seed
from test_export_filtered_abi import EDGE_BITS, FMA_P, FMA_PLANE, FMA_SPHERE, FMA_SPHERE_P
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, _device_meta, assert_export, expected_records
from test_gpu_export_filtered import ALL, HALF, NONE, cloud_sphere, filter_mask, run_filtered
from test_gpu_export_sorted import DIR
import test_gpu_program_export_sorted as pes
from test_gpu_program_export_sorted import POS_AGE_ID, make, step

pytestmark = pytest.mark.gpu

TILE = 4096
CAPS = (300, 4096, 4097, 10_000)        # one partial tile | exactly one tile | two tiles, the second of one row | three tiles, the last partial, more than one scan input
F32 = np.float32
BASES = [0, 100_000, 200_000, 300_000, 400_000]


def run_prog(ex, prog, flt):
    prog.export_filtered(ex.fields, ex.dst.data_ptr(), ex.stride, ex.capacity, ex.cnt.data_ptr(), ex.offsets.data_ptr() if ex.offsets is not None else None, filter=flt)
    return ex


def filters_of(flt, n):
    return list(flt) if isinstance(flt, (list, tuple)) else [flt] * n


def expected_prog(ctx, fxs, fields, stride, flt, verify=None):
    """-> (records, kept counts, alive counts): the concatenation of hnb_effect_export_filtered per instance, read back (synchronises). The kept
    set of every instance in `verify` (default: all) is held against the restated predicate, and its records against the host's read-back."""
    sdw = stride // 4
    singles = [run_filtered(Export(fields, stride, fx.capacity), fx, **f) for fx, f in zip(fxs, filters_of(flt, len(fxs)))]
    ctx.synchronize()
    recs, kept, alive = [], [], []
    for k, (fx, f, single) in enumerate(zip(fxs, filters_of(flt, len(fxs)), singles)):
        written, found = single.counts()
        assert written == found <= fx.capacity
        rec = single.words()[: found * sdw].reshape(found, sdw)
        n_alive = fx.alive_count()
        if verify is None or k in verify:
            mask = filter_mask(fx, fx.alive_list(), **f)
            assert int(mask.sum()) == found, (k, f, int(mask.sum()), found)
            np.testing.assert_array_equal(rec, expected_records(fx, fields, stride, slot_base=fx_slot_base(fx))[mask], err_msg=f"instance {k}")
        recs.append(rec); kept.append(found); alive.append(n_alive)
    return np.concatenate(recs), kept, alive


def fx_slot_base(fx):
    return getattr(fx, "slot_base_given", 0)


def make_based(cap, n, asset=None, **options):
    ctx, prog, fxs = make(cap, n, asset, slot_bases=BASES[:n] if n <= len(BASES) else None, **options)
    for k, fx in enumerate(fxs):
        fx.slot_base_given = BASES[k] if n <= len(BASES) else 0
    return ctx, prog, fxs


def check(ctx, prog, fxs, what, flt, fields=POS_AGE_ID, stride=20, capacity=None, offsets=True, partial=True, verify=None):
    """the program call in FRONT of the per-effect ones (nothing before it has materialised or computed anything for it), then compare"""
    n = len(fxs)
    ex = run_prog(Export(fields, stride, sum(fx.capacity for fx in fxs) if capacity is None else capacity, n_offsets=n + 1 if offsets else 0), prog, flt)
    rec, kept, alive = expected_prog(ctx, fxs, fields, stride, flt, verify)
    assert_export(ex, rec, f"{what}: {flt}", alive_rows=sum(kept))
    if offsets:
        np.testing.assert_array_equal(ex.offsets.cpu().numpy().view(np.uint32), np.concatenate([[0], np.cumsum(kept)]), err_msg=what)
    if partial:
        assert any(0 < k < a for k, a in zip(kept, alive)), (what, flt, kept, alive)
    return ex, kept, alive


def spawns_for(cap, n):
    return [cap, 0, cap // 3, 37, cap - 1][:n] if n > 1 else [cap]


# ---- states, shapes and the three kinds with a shared filter ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("cap", CAPS)
def test_burst_frozen_and_died_off_instances_with_a_shared_filter(cap, n):
    """After a burst: identity lists, one instance empty. Then one instance is frozen and the others lose particles: permuted partial lists next to
    a full frozen one. All three kinds, each with invert; ID fields with distinct slot bases at a stride of 20 bytes (segments start off a 16-byte
    boundary); out_offsets given and NULL. With a filter that keeps everything the call is hnb_program_export byte for byte."""
    ctx, prog, fxs = make_based(cap, n)
    spawns = spawns_for(cap, n)
    step(ctx, fxs, 0, spawns)
    ex, kept, alive = check(ctx, prog, fxs, "burst", HALF)
    assert alive == spawns
    check(ctx, prog, fxs, "burst", dict(HALF, invert=True), offsets=False)
    frozen = 2 if n >= 3 else None
    if frozen is not None:
        fxs[frozen].set_simulated(False)
    for f in (1, 2, 3):
        step(ctx, fxs, f, [0] * n, dt=0.3)
    ctx.synchronize()
    counts = [fx.alive_count() for fx in fxs]
    assert 0 < counts[0] < cap and (frozen is None or counts[frozen] == spawns[frozen])
    sph = cloud_sphere(fxs[0])
    for i, flt in enumerate((HALF, dict(kind="sphere", sphere=sph), dict(kind="sphere", sphere=sph, invert=True),
                             dict(kind="attr_range", attr=A.LIFETIME.id, lo=0.9, hi=1.1), dict(kind="attr_range", attr=A.LIFETIME.id, lo=0.9, hi=1.1, invert=True))):
        check(ctx, prog, fxs, f"capacity {cap}, {n} instances", flt, offsets=i % 2 == 0)
    # the identity
    everything = run_prog(Export(POS_AGE_ID, 20, n * cap, n_offsets=n + 1), prog, ALL)
    plain = Export(POS_AGE_ID, 20, n * cap, n_offsets=n + 1).run(prog)
    ctx.synchronize()
    np.testing.assert_array_equal(everything.words(), plain.words())
    np.testing.assert_array_equal(everything.offsets.cpu().numpy(), plain.offsets.cpu().numpy())
    assert everything.counts() == plain.counts() == [sum(counts)] * 2
    ctx.close()


# ---- a filter per instance ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [32, 256])
@pytest.mark.parametrize("cap", CAPS)
def test_a_filter_per_instance(cap, stride):
    """Five instances, five filters of one kind: different plane counts, different spheres, different ranges and inverts - one instance keeps
    everything and one nothing in the same call."""
    n = 5
    ctx, prog, fxs = make_based(cap, n)
    step(ctx, fxs, 0, [cap, cap // 2, cap, cap - 1, max(cap // 3, 64)])
    for f in (1, 2):
        step(ctx, fxs, f, [0] * n, dt=0.3)
    ctx.synchronize()
    p = fxs[2].read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fxs[2].alive_list()]
    q = lambda c, f: float(np.quantile(p[:, c], f))
    box = [(1, 0, 0, -q(0, 0.15)), (-1, 0, 0, q(0, 0.85)), (0, 1, 0, -q(1, 0.1)), (0, -1, 0, q(1, 0.9)), (0, 0, 1, -q(2, 0.1)), (0, 0, -1, q(2, 0.9))]
    planes = [ALL, NONE, dict(kind="planes", planes=box), dict(kind="planes", planes=box[:2], invert=True), HALF]
    spheres = [dict(kind="sphere", sphere=(0, 0, 0, 3e38)), dict(kind="sphere", sphere=(1e6, 0, 0, 0.0)), dict(kind="sphere", sphere=cloud_sphere(fxs[2])),
               dict(kind="sphere", sphere=cloud_sphere(fxs[3], 0.5), invert=True), dict(kind="sphere", sphere=cloud_sphere(fxs[4], -0.3))]
    L = A.LIFETIME.id
    ranges = [dict(kind="attr_range", attr=L, lo=0.0, hi=10.0), dict(kind="attr_range", attr=L, lo=5.0, hi=10.0), dict(kind="attr_range", attr=L, lo=0.9, hi=1.1),
              dict(kind="attr_range", attr=L, lo=1.0, hi=1.05, invert=True), dict(kind="attr_range", attr=L, lo=0.0, hi=1.0)]
    for flts in (planes, spheres, ranges):
        ex, kept, alive = check(ctx, prog, fxs, f"capacity {cap}, stride {stride}", flts, POS_AGE_LIFE_VEL, stride)
        assert kept[0] == alive[0] > 0 and kept[1] == 0 < alive[1]
    ctx.close()


# ---- churn, an empty instance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_permuted_lists_of_a_rate_spawner_churn(cap):
    n = 3
    ctx, prog, fxs = make_based(cap, n, effects.firework_trails(cap, spawner=bh.SpawnerSettings.rate(cap / 2.0)))
    rng = np.random.default_rng(cap)
    for f in range(40):
        step(ctx, fxs, f, [int(rng.integers(cap // 80 + 1, cap // 25 + 2)), 0, int(rng.integers(cap // 80 + 1, cap // 25 + 2))], dt=1 / 20)
    ctx.synchronize()
    lists = [fx.alive_list() for fx in fxs]
    assert len(lists[1]) == 0 and 0 < len(lists[0]) < cap and not np.array_equal(lists[0], np.sort(lists[0]))      # dead particles, a permuted list
    ages = fxs[0].read_attr(A.AGE.id).reshape(-1)[lists[0]]
    mid = float(np.median(ages))
    check(ctx, prog, fxs, "churn", dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=mid))
    check(ctx, prog, fxs, "churn", [dict(kind="sphere", sphere=cloud_sphere(fxs[0])), dict(kind="sphere", sphere=(0, 0, 0, 1)), dict(kind="sphere", sphere=cloud_sphere(fxs[2], 0.4), invert=True)],
          POS_AGE_LIFE_VEL, 32, offsets=False)
    ctx.close()


def test_three_hundred_instances_take_a_second_round_of_the_offsets_scan():
    cap, n = 300, 300
    ctx, prog, fxs = make(cap, n)
    step(ctx, fxs, 0, [(k * 7) % (cap + 1) for k in range(n)])
    ex, kept, alive = check(ctx, prog, fxs, "300 x 300", HALF, POS_AGE_LIFE_VEL, 32, verify=range(0, n, 37))
    assert alive == [(k * 7) % (cap + 1) for k in range(n)] and sum(kept) > 10_000
    r2 = np.median((fxs[299].read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fxs[299].alive_list()].astype(np.float64) ** 2).sum(1))
    flts = [dict(kind="sphere", sphere=(0.0, 0.0, 0.0, float(F32(r2 * (0.25 + (k % 9) / 4))))) for k in range(n)]
    check(ctx, prog, fxs, "300 x 300, a sphere each", flts, POS_AGE_ID, 20, verify=range(3, n, 41))
    ctx.close()


# ---- ring lists -----------------------------------------------------------------------------------------------------------------------------------
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
    check(ctx, prog, fxs, "ring, shared", dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=mids[0]), fields, 24)
    check(ctx, prog, fxs, "ring, a range each", [dict(kind="attr_range", attr=A.AGE.id, lo=0.0, hi=m, invert=bool(k & 1)) for k, m in enumerate(mids)], fields, 24)
    for fx, b, m in zip(fxs, before, metas):                             # the lists are what they were
        np.testing.assert_array_equal(fx.alive_list(), b)
        m2 = _device_meta(fx)
        assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


# ---- stale AGE; nothing later changes ---------------------------------------------------------------------------------------------------------------
def test_stale_age_as_field_and_as_source_and_a_twin_that_never_exports():
    """LEAN cohorts: the AGE plane is stale until something materialises it. The program call does, for all instances - when AGE is a record field
    and when it is only the range's source - and runs here in front of anything else that would. A twin context that never exports ends the run
    bit-identical."""
    cap, n = 10_000, 3
    with_age = [(A.AGE.id, 0), (A.LIFETIME.id, 4), (A.POSITION.id, 8)]
    without_age = [(A.LIFETIME.id, 0), (A.POSITION.id, 4)]
    (ctx, prog, fxs), (tctx, tprog, twins) = [make(cap, n, age_cohort=1) for _ in range(2)]
    assert fxs[0].device_view().stale_attr_mask == 1 << A.AGE.id
    dt = F32(1 / 60)
    young = dict(kind="attr_range", attr=A.AGE.id, lo=float(dt), hi=float(dt + dt + dt))
    for f in range(6):
        for c, e in ((ctx, fxs), (tctx, twins)):
            step(c, e, f, [6000, 3000, 0] if f == 0 else [300, 0, 200], dt=1 / 60)
        if f == 4:
            ex, kept, alive = check(ctx, prog, fxs, "stale AGE as a field", HALF, with_age, 20)
            assert len(np.unique(ex.words()[: kept[0] * 5].reshape(-1, 5)[:, 0])) == 5       # five cohorts of ages, all current
        if f == 5:
            ex, kept, alive = check(ctx, prog, fxs, "stale AGE as the source", young, without_age, 16)
            assert kept == [3 * 300, 0, 3 * 200]                         # the bursts of the last three frames are one, two and three ticks old
    for f in range(6, 14):
        for c, e in ((ctx, fxs), (tctx, twins)):
            step(c, e, f, [0, 100, 0], dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    for fx, twin in zip(fxs, twins):
        d = fx.compare(twin)
        assert d["equal"] == 1, d
        assert fx.check()["ok"] == 1
    ctx.close(); tctx.close()


# ---- exact operands -------------------------------------------------------------------------------------------------------------------------------
def test_edge_operand_lattice_and_the_fused_evaluation_triple():
    """The 4096 positions of edge operands of tests/test_export_filtered_abi.py and the two points a fused multiply-add would decide the other way,
    written into POSITION of every instance; plane sets and spheres of that test, one per instance."""
    pos = np.concatenate([np.array(list(itertools.product(EDGE_BITS, repeat=3)), np.uint32).view(F32), FMA_P[None], FMA_SPHERE_P[None]])
    cap, n = len(pos), 3
    assert cap == 4098
    ctx, prog, fxs = make(cap, n)
    step(ctx, fxs, 0, [cap] * n)
    ctx.synchronize()
    for fx in fxs:
        plane = np.zeros((cap, 3), F32)
        plane[fx.alive_list()] = pos                                     # list row r holds pos[r]
        fx.write_attr(A.POSITION.id, plane)
    rng = np.random.default_rng(3)
    t = lambda rows: [tuple(float(c) for c in r) for r in rows]
    planes = [dict(kind="planes", planes=t([[1, 0, 0, -1]])), dict(kind="planes", planes=t(np.concatenate([rng.uniform(-2, 2, (5, 4)).astype(F32), FMA_PLANE[None]]))),
              dict(kind="planes", planes=t(FMA_PLANE[None]), invert=True)]
    spheres = [dict(kind="sphere", sphere=(0, 0, 0, 1)), dict(kind="sphere", sphere=t(FMA_SPHERE[None])[0]), dict(kind="sphere", sphere=(1, -1, 0.5, 3), invert=True)]
    for flts in (planes, spheres, planes[0], spheres[1]):
        check(ctx, prog, fxs, "lattice", flts, [(A.POSITION.id, 0), (A.ID.id, 12)], 16)
    ex, kept, _ = check(ctx, prog, fxs, "the triple", [planes[2], dict(planes[2], invert=False), planes[0]], [(A.ID.id, 0)], 4)
    ids = ex.words()[: sum(kept)]
    fma_slot = int(fxs[0].alive_list()[4096])
    assert fma_slot in ids[: kept[0]] and int(fxs[1].alive_list()[4096]) not in ids[kept[0]: kept[0] + kept[1]]      # operation by operation the row fails the plane
    ex, kept, _ = check(ctx, prog, fxs, "the triple", spheres[1], [(A.ID.id, 0)], 4)
    assert int(fxs[0].alive_list()[4097]) in ex.words()[: kept[0]]        # ... and sits exactly at the radius
    ctx.close()


# ---- clamp ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [20, 32])
def test_global_clamp_counts_and_sentinels(stride):
    cap, n = 4097, 3
    ctx, prog, fxs = make_based(cap, n)
    step(ctx, fxs, 0, [cap, 1000, cap])
    ctx.synchronize()
    fields = POS_AGE_ID if stride == 20 else POS_AGE_LIFE_VEL
    rec, kept, alive = expected_prog(ctx, fxs, fields, stride, HALF)
    total = sum(kept)
    assert all(0 < k < a for k, a in zip(kept, alive))
    for K in (0, 1, kept[0] + kept[1] // 2, total - 1, total, total + 1):      # nothing | inside instance 0 | inside instance 1 | all but one | exactly | room to spare
        ex = run_prog(Export(fields, stride, K, slack=64, n_offsets=n + 1), prog, HALF)
        ctx.synchronize()
        assert ex.counts() == [min(K, total), total], (K, ex.counts())
        assert_export(ex, rec, f"the first {K} records", alive_rows=total)
        np.testing.assert_array_equal(ex.offsets.cpu().numpy().view(np.uint32), np.concatenate([[0], np.cumsum(kept)]))      # the offsets are those of the kept rows, cut or not
    ex = Export(fields, stride, n * cap)                                 # out_count NULL, out_offsets NULL
    prog.export_filtered(ex.fields, ex.dst.data_ptr(), stride, n * cap, None, None, filter=HALF)
    ctx.synchronize()
    assert ex.counts() == [SENTINEL, SENTINEL]
    np.testing.assert_array_equal(ex.words()[: total * stride // 4].reshape(total, -1), rec)
    assert (ex.words()[total * stride // 4:] == SENTINEL).all()
    ctx.close()


# ---- state and lifetime ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [300, 4097])
def test_scratch_is_reused_regrown_and_apart_from_the_other_exports(cap):
    ctx, prog, fxs = make_based(cap, 2)
    step(ctx, fxs, 0, [cap, cap // 2])
    check(ctx, prog, fxs, "two instances", HALF)
    check(ctx, prog, fxs, "two instances again", [HALF, dict(HALF, invert=True)])           # the scratch of the first call
    fx3 = prog.create_effect(slot_base=BASES[2])
    fx3.slot_base_given = BASES[2]
    fxs = fxs + [fx3]
    step(ctx, fxs, 1, [0, 0, cap - 1])
    check(ctx, prog, fxs, "a third instance", [dict(HALF, invert=True), HALF, HALF])        # regrown
    check(ctx, prog, fxs, "a third instance", HALF)
    # interleaved with the effect form and the sorted program form on the same program, nothing synchronises in between
    sort = dict(key="depth", v=DIR)
    a = run_prog(Export(POS_AGE_ID, 20, 3 * cap, n_offsets=4), prog, HALF)
    e = run_filtered(Export(POS_AGE_ID, 20, cap), fxs[0], **dict(HALF, invert=True))
    s = pes.run_sorted(Export(POS_AGE_ID, 20, 3 * cap, n_offsets=4), prog, "instance", **sort)
    b = run_prog(Export(POS_AGE_ID, 20, 3 * cap, n_offsets=4), prog, [ALL, NONE, HALF])
    e2 = run_filtered(Export(POS_AGE_ID, 20, cap), fxs[2], **HALF)
    s2 = pes.run_sorted(Export(POS_AGE_ID, 20, 3 * cap), prog, "program", **sort)
    ctx.synchronize()
    rec, kept, _ = expected_prog(ctx, fxs, POS_AGE_ID, 20, HALF)
    assert_export(a, rec, "program filtered in front", alive_rows=sum(kept))
    rec, kept, _ = expected_prog(ctx, fxs, POS_AGE_ID, 20, [ALL, NONE, HALF])
    assert_export(b, rec, "program filtered behind the others", alive_rows=sum(kept))
    for ex, fx, flt in ((e, fxs[0], dict(HALF, invert=True)), (e2, fxs[2], HALF)):
        mask = filter_mask(fx, fx.alive_list(), **flt)
        assert_export(ex, expected_records(fx, POS_AGE_ID, 20, slot_base=fx_slot_base(fx))[mask], "effect filtered in between", alive_rows=int(mask.sum()))
    bases = [fx_slot_base(fx) for fx in fxs]
    assert_export(s, pes.expected_program(fxs, POS_AGE_ID, 20, "instance", bases, **sort)[0], "program sorted in between")
    assert_export(s2, pes.expected_program(fxs, POS_AGE_ID, 20, "program", bases, **sort)[0], "program sorted behind")
    ctx.close()


@pytest.mark.parametrize("cap", [300, 10_000])
def test_ten_calls_with_other_filters_each_and_no_synchronisation_between_them(cap):
    """The staging buffer of the per-instance filters is rewritten by every call: each call's copy must have left it first."""
    n = 3
    ctx, prog, fxs = make_based(cap, n)
    step(ctx, fxs, 0, [cap, cap - 1, cap // 2])
    step(ctx, fxs, 1, [0] * n, dt=0.3)
    ctx.synchronize()
    cx, cy, cz, r2 = cloud_sphere(fxs[0])                                # round the cloud's median point, the median squared distance from it
    calls = []
    for i in range(10):
        flts = [dict(kind="sphere", sphere=(cx + 0.01 * i * (k + 1), cy, cz, float(F32(r2 * (0.3 + 0.17 * ((i + 2 * k) % 7))))), invert=bool((i + k) % 3 == 0)) for k in range(n)]
        calls.append((flts, run_prog(Export(POS_AGE_ID, 20, n * cap, n_offsets=n + 1), prog, flts)))
    ctx.synchronize()
    seen = set()
    for i, (flts, ex) in enumerate(calls):
        rec, kept, alive = expected_prog(ctx, fxs, POS_AGE_ID, 20, flts)
        assert_export(ex, rec, f"call {i}", alive_rows=sum(kept))
        np.testing.assert_array_equal(ex.offsets.cpu().numpy().view(np.uint32), np.concatenate([[0], np.cumsum(kept)]))
        assert any(0 < k < a for k, a in zip(kept, alive))
        seen.add(tuple(kept))
    assert len(seen) >= 8                                                # the calls did differ
    ctx.close()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    cap, n = 1000, 3
    ctx, prog, fxs = make_based(cap, n)
    step(ctx, fxs, 0, [cap, 10, cap // 2])
    ex = Export(POS_AGE_LIFE_VEL, 32, n * cap, n_offsets=n + 1)
    call = lambda flt, fields=POS_AGE_LIFE_VEL, dst=None, stride=32, offsets=None: prog.export_filtered(
        fields, ex.dst.data_ptr() if dst is None else dst, stride, n * cap, ex.cnt.data_ptr(), ex.offsets.data_ptr() if offsets is None else offsets, filter=flt)
    inf = float("inf")
    L = A.LIFETIME.id
    bad = {
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
    for what, flt in bad.items():
        with pytest.raises(bh.HanabiError) as ei:
            call(flt)
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    for i, broken in itertools.product(range(n), (dict(kind="planes", planes=[(1, 0, 0, inf)]), dict(kind="planes", planes=[(1, 0, 0, 0)], invert=2))):
        flts = [HALF] * n
        flts[i] = broken
        with pytest.raises(bh.HanabiError) as ei:
            call(flts)
        assert ei.value.code == -1 and f"filters[{i}]" in str(ei.value), (i, str(ei.value))      # the text names the filter
    bad_desc = {       # what hnb_program_export rejects
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
    lib = runtime.load_library()
    d = runtime.export_desc(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, n * cap, ex.cnt.data_ptr())
    flt = runtime.export_filter(**HALF)
    assert lib.hnb_program_export_filtered(prog._h, C.byref(d), None, 1, None) == -1 and b"NULL" in lib.hnb_last_error()
    for field, value in (("struct_size", 124), ("reserved", 1)):
        keep = getattr(flt, field)
        setattr(flt, field, value)
        assert lib.hnb_program_export_filtered(prog._h, C.byref(d), C.byref(flt), 1, None) == -1 and b"filters[0]" in lib.hnb_last_error(), field
        setattr(flt, field, keep)
    ctx.synchronize()
    assert ex.untouched() and (ex.offsets.cpu().numpy().view(np.uint32) == SENTINEL).all()
    call(HALF)                                                           # ... and the same arguments, unbroken, are accepted
    rec, kept, _ = expected_prog(ctx, fxs, POS_AGE_LIFE_VEL, 32, HALF)
    assert_export(ex, rec, "after the refusals", alive_rows=sum(kept))
    ctx.close()
