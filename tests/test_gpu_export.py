"""hnb_effect_export / hnb_program_export on the GPU (include/hanabi_amd.h "Packed output"): record r of the caller's buffer = the particle in row r
of the alive list. The destination is a torch tensor pre-filled with a sentinel; the expected records are built on the host with numpy from
read_attr + alive_list() - the host read-back path, itself pinned to the oracle by the parity tests."""
import ctypes as C

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, frame_seed
from test_export_abi import aos_layout

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EA7BEEF
POS_AGE_LIFE_VEL = [(A.POSITION.id, 0), (A.AGE.id, 12), (A.LIFETIME.id, 16), (A.VELOCITY.id, 20)]   # stride 32


class Export:
    """One enqueued export: the sentinel-filled destination (`slack` records more than the capacity it declares), the count words, the layout."""

    def __init__(self, fields, stride, capacity_records, slack=8, n_offsets=0):
        self.fields, self.stride, self.capacity = [(int(a), int(o)) for a, o in fields], stride, capacity_records
        self.dst = torch.full(((capacity_records + slack) * stride // 4 + 4,), SENTINEL, dtype=torch.int32, device="cuda")
        self.cnt = torch.full((2,), SENTINEL, dtype=torch.int32, device="cuda")
        self.offsets = torch.full((n_offsets,), SENTINEL, dtype=torch.int32, device="cuda") if n_offsets else None
        torch.cuda.synchronize()            # (the fills run on torch's stream, the export on the simulation's)

    def run(self, target, dst_ptr=None, **kw):
        if self.offsets is not None:
            kw["offsets_ptr"] = self.offsets.data_ptr()
        target.export(self.fields, self.dst.data_ptr() if dst_ptr is None else dst_ptr, self.stride, self.capacity, self.cnt.data_ptr(), **kw)
        return self

    def words(self):
        return self.dst.cpu().numpy().view(np.uint32)

    def counts(self):
        return [int(x) for x in self.cnt.cpu().numpy().view(np.uint32)]

    def untouched(self):
        return bool((self.words() == SENTINEL).all()) and self.counts() == [SENTINEL, SENTINEL]


def expected_records(fx, fields, stride, slot_base=0):
    """[alive, stride / 4] words: what the export must have written, from the host's read-back of the same effect (synchronises)."""
    alive = fx.alive_list()
    rec = np.zeros((len(alive), stride // 4), dtype=np.uint32)
    for attr, off in fields:
        if attr == A.ID.id:
            rec[:, off // 4] = np.uint32(slot_base) + alive
        else:
            nc = runtime.ATTR_COMPONENTS[attr]
            rec[:, off // 4: off // 4 + nc] = fx.read_attr(attr).view(np.uint32).reshape(-1, nc)[alive]
    return rec


def assert_export(ex, rec, what, alive_rows=None):
    """records bit-exact, out_count, sentinels behind the last written record"""
    n_alive = len(rec) if alive_rows is None else alive_rows
    n = min(len(rec), ex.capacity)
    sdw = ex.stride // 4
    got = ex.words()
    assert ex.counts() == [n, n_alive], (what, ex.counts(), n, n_alive)
    np.testing.assert_array_equal(got[: n * sdw].reshape(n, sdw), rec[:n], err_msg=what)
    assert (got[n * sdw:] == SENTINEL).all(), f"{what}: words behind record {n} were written"


def step(ctx, fx, f, spawn, dt=1 / 600):
    ctx.frame_begin(dt, f * dt)
    fx.set_frame(spawn, frame_seed(f))
    ctx.simulate()


def test_tile_edges_records_counts_and_sentinels():
    """Capacity 10,000 (a multiple of neither the 256-row tile nor a 4096-slot chunk): nothing alive, one particle, a full tile, a tile and a row,
    everything, and a partially died-off list in the other column."""
    cap = 10_000
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    seen = []
    f = 0
    for spawn, want in ((None, 0), (1, 1), (255, 256), (1, 257), (cap - 257, cap)):
        if spawn is not None:
            step(ctx, fx, f, spawn)
            f += 1
        ex = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)           # enqueued behind the frame: nothing synchronises in front of it
        ctx.synchronize()
        rec = expected_records(fx, POS_AGE_LIFE_VEL, 32)
        assert len(rec) == want
        assert_export(ex, rec, f"{want} alive")
        seen.append(len(rec))
    for _ in range(4):                                           # lifetimes are 0.8 .. 1.2 s: a second later part of the burst is gone
        step(ctx, fx, f, 0, dt=0.25)
        f += 1
    ex = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    ctx.synchronize()
    rec = expected_records(fx, POS_AGE_LIFE_VEL, 32)
    assert 0 < len(rec) < cap and not np.array_equal(fx.alive_list(), np.arange(len(rec)))    # a permuted, partial list
    assert_export(ex, rec, "after the partial die-off")
    ctx.close()


def test_padding_is_zeroed_and_fields_sit_at_odd_dword_offsets():
    """Stride 48, a vec3 at byte 4, a scalar at 44: the dwords of a written record that no field covers are zero (expected_records starts from
    zeros), whatever the buffer held before."""
    cap = 10_000
    fields = [(A.POSITION.id, 4), (A.COLOR.id, 20), (A.VELOCITY.id, 28), (A.AGE.id, 44)]
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    step(ctx, fx, 0, 777)
    ex = Export(fields, 48, cap).run(fx)
    ctx.synchronize()
    rec = expected_records(fx, fields, 48)
    assert len(rec) == 777 and (rec[:, [0, 4, 6, 10]] == 0).all() and rec[:, 1:4].any()
    assert_export(ex, rec, "stride 48")
    # a record of 256 bytes (the largest; tiles of 128 rows) with one field at its very end, and one of a single dword
    for fields, stride in (([(A.LIFETIME.id, 252), (A.POSITION.id, 0)], 256), ([(A.LIFETIME.id, 0)], 4)):
        ex = Export(fields, stride, cap).run(fx)
        ctx.synchronize()
        assert_export(ex, expected_records(fx, fields, stride), f"stride {stride}")
    ctx.close()


@pytest.mark.parametrize("order", ["spawn", "slot"])
def test_permuted_list_and_column_flips_exported_behind_every_frame(order):
    """A rate spawner with deaths, 40 frames, an export behind EVERY frame and no synchronisation of the exporting context in between (export,
    simulate, export, ...). The expected records of frame f come from a replica context that runs the same frames and is read back after each;
    hnb_effect_compare proves at the end that the replica is the exporting effect's state, and the last frame is also held against the exporting
    effect's own read-back."""
    cap, frames, dt = 5_000, 40, 1 / 20
    main, rep = bh.Context(0), bh.Context(0)
    fxs = []
    for c in (main, rep):
        c.set_list_order(order)
        fxs.append(c.create_program(bh.lower(effects.firework_trails(cap, spawner=bh.SpawnerSettings.rate(3000.0)))).create_effect())
    fx, fr = fxs
    exports = [Export(POS_AGE_LIFE_VEL, 32, cap, slack=1) for _ in range(frames)]
    expected = []
    rng = np.random.default_rng(5)
    for f in range(frames):
        spawn = int(rng.integers(50, 400))
        step(main, fx, f, spawn, dt)
        exports[f].run(fx)
        step(rep, fr, f, spawn, dt)
        expected.append(expected_records(fr, POS_AGE_LIFE_VEL, 32))      # (synchronises the replica's context only)
    main.synchronize()
    assert fx.compare(fr)["equal"] == 1
    for f in range(frames):
        assert_export(exports[f], expected[f], f"{order} order, frame {f}")
    assert_export(exports[-1], expected_records(fx, POS_AGE_LIFE_VEL, 32), "last frame, own read-back")
    counts = [len(e) for e in expected]
    assert max(counts) > 1000 and any(b < a for a, b in zip(counts, counts[1:])), counts        # particles died on the way
    lists = fx.alive_list()
    assert order == "slot" or not np.array_equal(lists, np.sort(lists))                       # spawn order: a permuted list
    main.close(); rep.close()


def _device_meta(fx):
    """the effect's HnbDeviceMeta row, copied from the device (after a synchronisation)"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    m = runtime.DeviceMeta()
    assert hip.hipMemcpy(C.byref(m), C.c_void_p(fx.device_view().meta), C.sizeof(m), 2) == 0
    return m


def test_ring_list_with_a_wrapped_head():
    """The ribbon example keeps its list as a ring (HNB_OPT_RING_LISTS): rows start at a head that moves towards the front of the column and wraps
    round its end. Exported while the head is non-zero, before and after it has wrapped."""
    cap = 4096
    fields = [(A.AGE.id, 0), (A.POSITION.id, 4), (A.RIBBON_ID.id, 16), (A.SIZE.id, 20)]
    ctx = bh.Context(0)
    ctx.set_option("ring_lists", 1)
    asset = effects.ribbon(cap)
    fx = ctx.create_program(bh.lower(asset)).create_effect()
    sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
    heads, wrapped_rows = [], 0
    for f in range(150):
        dt = 1 / 60
        ctx.frame_begin(dt, f * dt)
        fx.set_frame(sp.tick(dt, rng), frame_seed(f))
        ctx.simulate()
        if f % 10 != 9:
            continue
        ex = Export(fields, 24, cap).run(fx)
        ctx.synchronize()
        m = _device_meta(fx)
        heads.append(m.list_column >> 1)
        if (m.list_column >> 1) + m.alive_count > cap:
            wrapped_rows += 1                                    # the list itself runs across the end of the column
        assert_export(ex, expected_records(fx, fields, 24), f"frame {f}, head {m.list_column >> 1}")
    assert any(h != 0 for h in heads), heads                                                  # list_column >> 1 != 0: the list is kept as a ring
    assert any(b > a for a, b in zip(heads, heads[1:])), heads                                # the head, which moves down, came round the end
    assert wrapped_rows > 0, heads
    ctx.close()


@pytest.mark.parametrize("cohort", [1, 3, 0], ids=["lean", "auto", "off"])
def test_stale_age_is_exported_current_without_a_materialise_call(cohort):
    cap = 300_007
    ctx = bh.Context(0)
    ctx.set_option("age_cohort", cohort)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    assert fx.device_view().stale_attr_mask == ((1 << A.AGE.id) if cohort == 1 else 0)
    for f in range(6):
        step(ctx, fx, f, cap if f == 0 else 0, dt=1 / 60)
    fields = [(A.AGE.id, 0), (A.LIFETIME.id, 4)]
    ex = Export(fields, 8, cap).run(fx)                          # no materialise in front of it
    ctx.synchronize()
    rec = expected_records(fx, fields, 8)                        # (the host read materialises for itself)
    assert len(rec) == cap
    age = np.float32(0.0)
    for _ in range(6):
        age = age + np.float32(1 / 60)
    assert (rec[:, 0].view(np.float32) == age).all()             # six ticks of 1/60 s, added in binary32
    assert_export(ex, rec, f"age cohort mode {cohort}")
    ctx.close()


@pytest.mark.parametrize("cohort", [1, 3, 0], ids=["lean", "auto", "off"])
def test_exporting_changes_nothing_later_frames_compute(cohort):
    """A twin context runs the same 30 frames and never exports; this one exports every third frame (AGE included: the export materialises it
    under the cohort modes). Bit for bit the same state at the end."""
    cap = 70_000
    ctxs = [bh.Context(0), bh.Context(0)]
    fxs = []
    for c in ctxs:
        c.set_option("age_cohort", cohort)
        fxs.append(c.create_program(bh.lower(effects.firework_trails(cap))).create_effect())
    keep = []
    for f in range(30):
        spawn = cap if f == 0 else (cap // 3 if f == 20 else 0)
        for c, fx in zip(ctxs, fxs):
            step(c, fx, f, spawn, dt=1 / 20)
        if f % 3 == 0:
            keep.append(Export(POS_AGE_LIFE_VEL, 32, cap).run(fxs[0]))
    for c in ctxs:
        c.synchronize()
    d = fxs[0].compare(fxs[1])
    assert d["equal"] == 1, d
    assert fxs[0].check()["ok"] == 1 and 0 < fxs[0].alive_count() < cap
    assert keep[0].counts() == [cap, cap] and keep[-1].counts()[1] == keep[-1].counts()[0] < cap
    for c in ctxs:
        c.close()


def test_clamp_against_the_destination_capacity():
    cap = 10_000
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    step(ctx, fx, 0, cap)
    ex = Export(POS_AGE_LIFE_VEL, 32, 100, slack=400).run(fx)
    ctx.synchronize()
    rec = expected_records(fx, POS_AGE_LIFE_VEL, 32)
    assert len(rec) == cap
    assert ex.counts() == [100, cap]
    assert_export(ex, rec, "100 of 10,000", alive_rows=cap)       # exactly 100 records; the sentinel at record 100 and behind is intact
    ex0 = Export(POS_AGE_LIFE_VEL, 32, 0, slack=16).run(fx)       # no room at all: counts only
    ctx.synchronize()
    assert ex0.counts() == [0, cap] and (ex0.words() == SENTINEL).all()
    ctx.close()


def test_id_of_a_capacity_slab():
    cap, base = 10_000, 70_000
    fields = [(A.ID.id, 0), (A.AGE.id, 4)]
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect(slot_base=base)
    step(ctx, fx, 0, 3000)
    for f in range(1, 5):
        step(ctx, fx, f, 100, dt=0.25)                           # some die, others take their slots: the list is no identity
    ex = Export(fields, 8, cap).run(fx)
    ctx.synchronize()
    alive = fx.alive_list()
    rec = expected_records(fx, fields, 8, slot_base=base)
    assert 0 < len(alive) and not np.array_equal(alive, np.arange(len(alive)))
    np.testing.assert_array_equal(rec[:, 0], base + alive)
    assert_export(ex, rec, "ID = slot_base + slot")
    ctx.close()


def test_program_export_packs_every_instance_back_to_back():
    """Five instances in different states - one empty, one frozen (hnb_effect_set_simulated(fx, 0)) - behind ONE gather launch: out_offsets is the
    exclusive scan of their alive counts, every segment equals the instance's own hnb_effect_export and the host's read-back. A stride of 20 bytes:
    the segments start at any dword, not at 16-byte boundaries."""
    cap, n_inst = 4096, 5
    fields = [(A.POSITION.id, 0), (A.AGE.id, 12), (A.ID.id, 16)]
    ctx = bh.Context(0)
    prog = ctx.create_program(bh.lower(effects.instancing(cap, rate=cap / 0.25)))
    fxs = [prog.create_effect(slot_base=1000 * k) for k in range(n_inst)]
    spawns = [37, 0, 700, 301, 1234]                             # instance 1 stays empty
    for f in range(6):
        ctx.frame_begin(1 / 60, f / 60)
        if f == 3:
            fxs[2].set_simulated(False)                          # frozen from here on: its state of frame 2 is what is exported
        for k, fx in enumerate(fxs):
            fx.set_frame(spawns[k] if f < 4 else 0, frame_seed(f * n_inst + k))
        ctx.simulate()
    total_cap = n_inst * cap
    ex = Export(fields, 20, total_cap, n_offsets=n_inst + 1).run(prog)
    singles = [Export(fields, 20, cap).run(fx) for fx in fxs]
    ctx.synchronize()
    counts = [fx.alive_count() for fx in fxs]
    assert counts[1] == 0 and counts[2] == 3 * 700 and len(set(counts)) == n_inst
    offs = ex.offsets.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(offs, np.concatenate([[0], np.cumsum(counts)]))
    total = int(offs[-1])
    assert ex.counts() == [total, total]
    got = ex.words()
    for k, fx in enumerate(fxs):
        assert fx.index() == k
        seg = got[offs[k] * 5: offs[k + 1] * 5].reshape(-1, 5)
        np.testing.assert_array_equal(seg, singles[k].words()[: counts[k] * 5].reshape(-1, 5), err_msg=f"instance {k}: its own hnb_effect_export")
        assert_export(singles[k], expected_records(fx, fields, 20, slot_base=1000 * k), f"instance {k}")
    assert (got[total * 5:] == SENTINEL).all()
    # the clamp is global: room for the first two and a half instances, no offsets asked for
    room = counts[0] + counts[1] + counts[2] // 2
    exc = Export(fields, 20, room, slack=total).run(prog)
    ctx.synchronize()
    assert exc.counts() == [room, total]
    np.testing.assert_array_equal(exc.words()[: room * 5], got[: room * 5])
    assert (exc.words()[room * 5:] == SENTINEL).all()
    ctx.close()


def test_reference_layout_gives_the_references_particle_array():
    """Fields and stride from hnb_asset_particle_layout_aos: the buffer is the reference's array<Particle> in list order - a numpy structured array
    with the ParticleLayout's offsets, padding zero."""
    cap = 10_000
    asset = effects.firework_trails(cap)
    fields, stride = aos_layout(asset)
    layout = asset.reference_particle_layout()
    assert stride == layout.min_binding_size() == 48
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(asset)).create_effect()
    step(ctx, fx, 0, 3001)
    ex = Export(fields, stride, cap).run(fx)
    ctx.synchronize()
    alive = fx.alive_list()
    names, formats, offsets = [], [], []
    for name, off in layout.entries():
        if name == "pad":
            continue
        attr = bh.Attribute.from_name(name)
        names.append(name); offsets.append(off)
        formats.append((np.float32 if runtime.ATTR_IS_FLOAT[attr.id] else np.uint32, (runtime.ATTR_COMPONENTS[attr.id],)))
    particles = np.zeros(len(alive), dtype=np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": stride}))
    for name in names:
        particles[name] = fx.read_attr(bh.Attribute.from_name(name).id)[alive]
    n = len(alive)
    assert n == 3001 and ex.counts() == [n, n]
    got = ex.dst.cpu().numpy().view(np.uint8)
    np.testing.assert_array_equal(got[: n * stride], particles.view(np.uint8).reshape(-1))
    assert (ex.words()[n * stride // 4:] == SENTINEL).all()
    ctx.close()


def test_argument_errors_enqueue_nothing():
    cap = 1000
    ctx = bh.Context(0)
    prog = ctx.create_program(bh.lower(effects.firework_trails(cap)))
    fx = prog.create_effect()
    step(ctx, fx, 0, cap)
    ex = Export(POS_AGE_LIFE_VEL, 32, cap)
    bad = {
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
    for what, kw in bad.items():
        for target, extra in ((fx, {}), (prog, {"offsets_ptr": None})):
            with pytest.raises(bh.HanabiError) as ei:
                target.export(kw.get("fields", POS_AGE_LIFE_VEL), kw.get("dst", ex.dst.data_ptr()), kw.get("stride", 32), cap, ex.cnt.data_ptr(), **extra)
            assert ei.value.code == -1 and len(str(ei.value)) > 8, what      # HNB_ERR_INVALID_ARG, with text
    d = runtime.export_desc(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, cap, ex.cnt.data_ptr())
    lib = runtime.load_library()
    for field, value in (("struct_size", 64), ("flags", 1)):
        setattr(d, field, value)
        assert lib.hnb_effect_export(fx._h, C.byref(d)) == -1 and lib.hnb_program_export(prog._h, C.byref(d), None) == -1, field
        setattr(d, field, C.sizeof(runtime.ExportDesc) if field == "struct_size" else 0)
    ctx.synchronize()
    assert ex.untouched()
    assert lib.hnb_effect_export(fx._h, C.byref(d)) == 0        # ... and the same description, unbroken, is accepted
    ctx.synchronize()
    assert ex.counts() == [cap, cap]
    ctx.close()
