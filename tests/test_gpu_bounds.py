"""hnb_effect_bounds / hnb_program_bounds on the GPU (include/hanabi_amd.h "Bounds"): per component of one f32 attribute the stored value with the
smallest and the largest sort key among the alive particles, the alive and the NaN particles counted. The expectation is always numpy over
read_attr + alive_list() with the key rule (tests/test_bounds_abi.py np_bounds), compared as uint32 words: there is no tolerance anywhere. The
destination is a torch tensor pre-filled with a sentinel, so a record written where none belongs is seen."""
import ctypes as C

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, frame_seed
from test_bounds_abi import NEG_INF, POS_INF, np_bounds, np_union, trails_vec4
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, _device_meta, step
from test_gpu_export_filtered import HALF, run_filtered
from test_gpu_export_sorted import burst_then_die_off, make
import test_gpu_program_export_sorted as pes

pytestmark = pytest.mark.gpu

W = 12                                          # words of a record
F32 = np.float32
# 1 slot | a wave less one, a wave | a workgroup's lanes less one, plus one | one tile less one slot, exactly one tile (the one-workgroup path's last
# capacity) | the first two-tile capacity, its second tile one slot | two full tiles | ... and a slot | three tiles and a ragged fourth whose last
# quad is one slot | 73 tiles and 999 slots, no multiple of 4
CAPS = (1, 63, 64, 255, 257, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 5, 300_007)
EMPTY3 = [POS_INF] * 3 + [0] + [NEG_INF] * 3 + [0] * 5


class Dst:
    """The destination of one call: `records` records it may write and `slack` more behind them, all sentinel"""

    def __init__(self, records=1, slack=2):
        self.records = records
        self.t = torch.full(((records + slack) * W,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                # (the fill runs on torch's stream, the call on the simulation's)

    def ptr(self):
        return self.t.data_ptr()

    def words(self):
        return self.t.cpu().numpy().view(np.uint32)

    def untouched(self):
        return bool((self.words() == SENTINEL).all())


def run(target, attr, records=1, capacity_records=None):
    d = Dst(records)
    target.bounds(int(attr), d.ptr(), records if capacity_records is None else capacity_records)
    return d


def alive_mask(fx):
    m = np.zeros(fx.capacity, bool)
    m[fx.alive_list()] = True
    return m


def expected(fx, attr):
    """the record from the host's read-back of the same effect (synchronises; read_attr materialises stale planes for itself)"""
    return np_bounds(fx.read_attr(int(attr)).view(np.uint32), alive_mask(fx))


def assert_records(d, recs, what):
    recs = np.asarray(recs, np.uint32).reshape(-1, W)
    got = d.words()
    np.testing.assert_array_equal(got[: len(recs) * W].reshape(-1, W), recs, err_msg=what)
    assert (got[len(recs) * W:] == SENTINEL).all(), f"{what}: words behind record {len(recs)} were written"


# ---- capacities, component counts, states ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_capacities_all_alive_and_after_a_die_off(cap):
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=1 / 60)               # (positions leave the origin)
    attrs = (A.POSITION, A.LIFETIME, A.F32X4_0)
    runs = [run(fx, a.id) for a in attrs]        # enqueued behind the frames: nothing synchronises in front of them
    ctx.synchronize()
    assert fx.alive_count() == cap
    for a, d in zip(attrs, runs):
        rec = expected(fx, a.id)
        assert rec[8] == cap and rec[9] == 0
        assert_records(d, rec, f"capacity {cap}, all alive, {a.name}")
    if cap > 1:
        assert runs[0].words()[0] != runs[0].words()[4]                  # a box, not a point
    for f in range(2, 6):                                               # lifetimes are 0.8 .. 1.2 s: a second later part of the burst is gone
        step(ctx, fx, f, 0, dt=0.25)
    attrs = (A.POSITION, A.AGE, A.F32X4_0)
    runs = [run(fx, a.id) for a in attrs]
    ctx.synchronize()
    n = fx.alive_count()
    assert 0 < n < cap or cap < 63, n                                   # (a handful of particles may all live or all be gone)
    for a, d in zip(attrs, runs):
        rec = expected(fx, a.id)
        assert rec[8] == n
        assert_records(d, rec, f"capacity {cap}, {n} alive, {a.name}")
    assert fx.check()["ok"] == 1
    ctx.close()


@pytest.mark.parametrize("cap", [255, 4097, 3 * 4096 + 5, 300_007])
def test_dead_slots_do_not_enter(cap):
    """Every slot that is not alive holds (3e38, -3e38, NaN): a walk that ignores the alive byte, or reads the tail as alive, reports them"""
    ctx, fx = burst_then_die_off(cap)
    alive = alive_mask(fx)
    assert 0 < alive.sum() < cap
    pos = fx.read_attr(A.POSITION.id).copy()
    want = np_bounds(pos.view(np.uint32), alive)
    pos[~alive] = np.array([3e38, -3e38, np.nan], F32)
    fx.write_attr(A.POSITION.id, pos)
    d = run(fx, A.POSITION.id)
    ctx.synchronize()
    np.testing.assert_array_equal(np_bounds(fx.read_attr(A.POSITION.id).view(np.uint32), alive), want)
    assert want[9] == 0 and want[8] == alive.sum()
    assert np.abs(want[:8].view(F32)).max() < 1e6
    assert_records(d, want, f"capacity {cap}: dead slots poisoned")
    ctx.close()


@pytest.mark.parametrize("cap", [300, 10_000])
def test_edge_values_in_alive_slots(cap):
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    ctx.synchronize()
    rng = np.random.default_rng(cap)
    nan, neg_nan = np.uint32(0x7FC00000), np.uint32(0xFFC00001)
    # x: NaNs of both signs but for two zeros; y: finite values and both infinities; z: a NaN in every particle
    pos = rng.normal(0, 10, (cap, 3)).astype(F32).view(np.uint32)
    pos[:, 0] = np.where(rng.random(cap) < 0.5, nan, neg_nan)
    pos[cap // 3, 0], pos[cap - 1, 0] = 0x00000000, 0x80000000
    pos[7, 1], pos[cap // 2, 1] = NEG_INF, POS_INF
    pos[:, 2] = nan
    fx.write_attr(A.POSITION.id, pos.view(F32))
    d = run(fx, A.POSITION.id)
    ctx.synchronize()
    rec = expected(fx, A.POSITION.id)
    assert list(rec[[0, 4, 1, 5, 2, 6]]) == [0x80000000, 0x00000000, NEG_INF, POS_INF, POS_INF, NEG_INF]      # -0 < +0; infinite in y; z empty
    assert rec[8] == cap and rec[9] == cap
    assert_records(d, rec, "zeros, infinities, a component that is a NaN everywhere")
    # NaNs in one component only of some particles: that component skips them, the others take them; counted once per particle
    pos = rng.normal(0, 10, (cap, 3)).astype(F32)
    extreme = np.argmax(pos[:, 1])
    pos[extreme, 0] = np.nan                                            # its y is the largest and still counts
    in_x, in_y = rng.random(cap) < 0.2, rng.random(cap) < 0.2
    in_y[extreme] = False
    pos[in_x, 0] = np.nan
    pos[in_y, 1] = np.nan
    fx.write_attr(A.POSITION.id, pos)
    d = run(fx, A.POSITION.id)
    ctx.synchronize()
    rec = expected(fx, A.POSITION.id)
    both = int((in_x & in_y).sum())
    assert both > 0 and rec[9] == int((in_x | in_y).sum()) + (0 if in_x[extreme] else 1) and rec[5] == pos[extreme, 1].view(np.uint32)
    assert_records(d, rec, "NaNs in single components")
    ctx.close()


@pytest.mark.parametrize("cap", [300, 10_000])
def test_nothing_alive(cap):
    ctx, fx = make(cap)
    d = run(fx, A.POSITION.id)                                          # before the first frame
    ctx.synchronize()
    assert_records(d, EMPTY3, "before the first frame")
    step(ctx, fx, 0, cap)
    for f in range(1, 5):
        step(ctx, fx, f, 0, dt=0.5)                                     # every lifetime is over
    d, d1 = run(fx, A.POSITION.id), run(fx, A.AGE.id)
    ctx.synchronize()
    assert fx.alive_count() == 0
    assert_records(d, EMPTY3, "after everything has died")
    assert_records(d1, [POS_INF, 0, 0, 0, NEG_INF] + [0] * 7, "after everything has died, one component")
    ctx.close()


# ---- program form ---------------------------------------------------------------------------------------------------------------------------------
def check_program(ctx, prog, fxs, attr, what):
    """the program call in FRONT of the per-effect ones, then: records == the per-effect calls' == numpy; the union == the numpy fold"""
    n = len(fxs)
    d = run(prog, attr, n + 1)
    singles = Dst(n, slack=0)
    for k, fx in enumerate(fxs):
        fx.bounds(int(attr), singles.ptr() + k * W * 4, 1)
    ctx.synchronize()
    recs = np.stack([expected(fx, attr) for fx in fxs])
    np.testing.assert_array_equal(singles.words().reshape(n, W), recs, err_msg=f"{what}: per-effect calls")
    union = np_union(recs, runtime.ATTR_COMPONENTS[int(attr)])
    bits = np.concatenate([fx.read_attr(int(attr)).view(np.uint32) for fx in fxs])
    np.testing.assert_array_equal(union, np_bounds(bits, np.concatenate([alive_mask(fx) for fx in fxs])))      # the fold of records is the fold of particles
    assert_records(d, np.concatenate([recs, union[None]]), what)
    return recs


@pytest.mark.parametrize("cap", [300, 4096, 4097, 10_000])
def test_program_of_five_instances_one_empty_one_frozen(cap):
    n = 5
    ctx, prog, fxs = pes.make(cap, n)
    spawns = [cap, 0, cap // 3, 37, cap - 1]
    pes.step(ctx, fxs, 0, spawns)
    pes.step(ctx, fxs, 1, [0] * n, dt=1 / 60)
    recs = check_program(ctx, prog, fxs, A.POSITION.id, f"capacity {cap}, burst")
    assert list(recs[:, 8]) == spawns and list(recs[1]) == EMPTY3
    fxs[2].set_simulated(False)
    for f in (2, 3, 4):
        pes.step(ctx, fxs, f, [0] * n, dt=0.3)
    frozen = recs[2].copy()
    recs = check_program(ctx, prog, fxs, A.POSITION.id, f"capacity {cap}, die-off")
    assert 0 < recs[0, 8] < cap and (recs[2] == frozen).all()           # the frozen instance reports the state it was frozen in
    check_program(ctx, prog, fxs, A.LIFETIME.id, f"capacity {cap}, die-off, LIFETIME")
    # dst_capacity_records == n_instances: refused, nothing written
    d = Dst(n + 1)
    with pytest.raises(bh.HanabiError, match="dst_capacity_records"):
        prog.bounds(A.POSITION.id, d.ptr(), n)
    ctx.synchronize()
    assert d.untouched()
    ctx.close()


def test_program_of_300_instances_of_300_slots():
    """k_bounds_union past one wave, and past one round of its 256 lanes, of instances"""
    n, cap = 300, 300
    ctx, prog, fxs = pes.make(cap, n)
    pes.step(ctx, fxs, 0, [(k * 7) % (cap + 1) for k in range(n)])
    pes.step(ctx, fxs, 1, [0] * n, dt=1 / 30)
    recs = check_program(ctx, prog, fxs, A.POSITION.id, "300 x 300")
    assert list(recs[:, 8]) == [(k * 7) % (cap + 1) for k in range(n)] and len({int(x) for x in recs[:, 4]}) > 250
    ctx.close()


# ---- ring lists, stale AGE ------------------------------------------------------------------------------------------------------------------------
def test_ribbon_program_with_a_ring_list():
    cap = 10_000
    asset = effects.ribbon(cap)
    ctx, fx = make(cap, asset, ring_lists=1)
    sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
    for f in range(90):
        dt = 1 / 60
        ctx.frame_begin(dt, f * dt)
        fx.set_frame(sp.tick(dt, rng), frame_seed(f))
        ctx.simulate()
    runs = [(a, run(fx, a.id)) for a in (A.AGE, A.POSITION, A.SIZE)]
    ctx.synchronize()
    m = _device_meta(fx)
    assert (m.list_column >> 1) != 0 and 256 < m.alive_count < cap        # kept as a ring, the head somewhere inside the column
    before = fx.alive_list().copy()
    for a, d in runs:
        rec = expected(fx, a.id)
        assert rec[8] == m.alive_count
        assert_records(d, rec, f"ring list, {a.name}")
    assert runs[0][1].words()[0] != runs[0][1].words()[4]                # the ages differ
    np.testing.assert_array_equal(fx.alive_list(), before)
    ctx.close()


def test_stale_age_is_materialised_first_and_nothing_later_changes():
    """LEAN cohorts: the AGE plane is stale until something materialises it; the call does. A twin context that never calls ends bit-identical."""
    cap = 100_000
    pairs = [make(cap, age_cohort=1) for _ in range(2)]
    (ctx, fx), (tctx, twin) = pairs
    assert fx.device_view().stale_attr_mask == 1 << A.AGE.id
    dt = F32(1 / 60)
    keep = []
    for f in range(5):
        for c, e in pairs:
            step(c, e, f, 70_000 if f == 0 else 3000, dt=1 / 60)
        if f >= 3:                                                       # no materialise call in front of them
            keep.append((run(fx, A.AGE.id), run(fx, A.POSITION.id)))
    ctx.synchronize()
    rec = expected(fx, A.AGE.id)                                         # (the read-back materialises for itself - behind the calls above)
    assert rec[8] == 70_000 + 4 * 3000 and rec[0].view(F32) == dt and rec[4].view(F32) > F32(4.5) * dt      # the youngest burst is one tick old, the first five
    assert_records(keep[-1][0], rec, "stale AGE")
    assert_records(keep[-1][1], expected(fx, A.POSITION.id), "POSITION next to it")
    assert keep[0][0].words()[8] == 70_000 + 3 * 3000 and keep[0][0].words()[0] == rec[0]
    for f in range(5, 12):
        for c, e in pairs:
            step(c, e, f, 0, dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    d = fx.compare(twin)
    assert d["equal"] == 1, d
    assert fx.check()["ok"] == 1
    ctx.close(); tctx.close()


# ---- in the stream, next to the exports -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [3000, 10_000])
def test_ten_calls_interleaved_with_frames_and_exports_without_a_synchronisation(cap):
    """Ten program calls and ten effect calls into twenty destinations, a frame between two of them, a filtered effect export and a sorted program
    export in between, and no synchronisation of the context until the end. The expected records of call i come from a replica context that runs
    the same frames and is read back after each; hnb_effect_compare proves at the end that the replica is the calling context's state. Then the
    program gains an instance: the scratch is regrown, and the next call is right."""
    n = 2
    (ctx, prog, fxs), (rctx, rprog, rfxs) = pes.make(cap, n), pes.make(cap, n)
    calls, want, exports = [], [], []                                   # (exports: their destinations stay allocated until the stream has run them)
    for f in range(10):
        spawns = [cap if f == 0 else 0, 50 * f]
        for c, e in ((ctx, fxs), (rctx, rfxs)):
            pes.step(c, e, f, spawns, dt=1 / 600 if f == 0 else 0.12)
        calls.append((run(prog, A.POSITION.id, n + 1), run(fxs[1], A.AGE.id)))
        exports.append(run_filtered(Export(POS_AGE_LIFE_VEL, 32, cap), fxs[0], **HALF))
        if f % 3 == 0:
            exports.append(pes.run_sorted(Export(pes.POS_AGE_ID, 20, n * cap, n_offsets=n + 1), prog, "instance", key="depth", v=(0.3, -0.5, 0.8)))
        rctx.synchronize()
        recs = np.stack([expected(fx, A.POSITION.id) for fx in rfxs])
        want.append((np.concatenate([recs, np_union(recs, 3)[None]]), expected(rfxs[1], A.AGE.id)))
    ctx.synchronize()
    for f, ((dp, de), (wp, we)) in enumerate(zip(calls, want)):
        assert_records(dp, wp, f"program call behind frame {f}")
        assert_records(de, we, f"effect call behind frame {f}")
    assert 0 < want[-1][0][0, 8] < cap and want[-1][0][1, 8] > 0          # the burst is dying off, the trickle is alive
    for a, b in zip(fxs, rfxs):
        assert a.compare(b)["equal"] == 1
    fxs.append(prog.create_effect())
    pes.step(ctx, fxs, 10, [0, 0, cap // 2])
    check_program(ctx, prog, fxs, A.POSITION.id, "after an instance was added")
    ctx.close(); rctx.close()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    """Every refusal of the contract but one: more than 65535 instances, which no test here creates."""
    cap = 5000
    ctx, prog, fxs = pes.make(cap, 2)
    pes.step(ctx, fxs, 0, [cap, 100])
    empty_prog = ctx.create_program(bh.lower(effects.firework_trails(300)))
    fx = fxs[0]
    lib = runtime.load_library()
    d = Dst(3)
    good = lambda: runtime.bounds_desc(A.POSITION.id, d.ptr(), 3)

    def refused(call, handle, desc, text):
        assert call(handle, C.byref(desc)) == -1, text
        assert text.encode() in lib.hnb_last_error(), (text, lib.hnb_last_error())

    for call, handle, is_prog in ((lib.hnb_effect_bounds, fx._h, False), (lib.hnb_program_bounds, prog._h, True)):
        x = good(); x.struct_size = 28
        refused(call, handle, x, "struct_size")
        x = good(); x.flags = 1
        refused(call, handle, x, "flags")
        x = good(); x.reserved = 1
        refused(call, handle, x, "reserved")
        x = good(); x.dst = None
        refused(call, handle, x, "16-byte aligned")
        x = good(); x.dst = d.ptr() + 4
        refused(call, handle, x, "16-byte aligned")
        x = good(); x.dst_capacity_records = 2 if is_prog else 0
        refused(call, handle, x, "dst_capacity_records")
        x = good(); x.attr = A.SIZE3.id
        refused(call, handle, x, "not part of the particle layout")
        x = good(); x.attr = A.COLOR.id                                  # in the layout, packed u32
        refused(call, handle, x, "not an f32 attribute")
        for attr in (A.ID.id, A.PARTICLE_COUNTER.id, 9999):
            x = good(); x.attr = attr
            refused(call, handle, x, "no plane")
    x = runtime.bounds_desc(A.POSITION.id, d.ptr(), 3)
    refused(lib.hnb_program_bounds, empty_prog._h, x, "0 instances")
    ctx.synchronize()
    assert d.untouched()
    prog.bounds(A.POSITION.id, d.ptr(), 3)                               # ... and the same destination takes a good call
    ctx.synchronize()
    recs = np.stack([expected(f, A.POSITION.id) for f in fxs])
    np.testing.assert_array_equal(d.words()[: 3 * W].reshape(3, W), np.concatenate([recs, np_union(recs, 3)[None]]))
    ctx.close()
