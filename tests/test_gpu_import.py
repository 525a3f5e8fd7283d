"""hnb_effect_import on the GPU (include/hanabi_amd_import.h): records on the device go into the planes of the particles they belong to, and later
frames compute what they would after hnb_effect_write_attr of the same values. Expectations come from numpy over read_attr and alive_list() - the
planes as they were, with the records' fields put where the list (ROWS) or the ID field (IDS) says - and from a twin context driven through
read_attr + numpy + hnb_effect_write_attr. Everything is compared as uint32 words, with assert_same_state and hnb_effect_compare: every result is
uniquely determined, there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, assert_same_state, frame_seed, stored_attrs
from test_gpu_export import SENTINEL, Export, _device_meta, step

pytestmark = pytest.mark.gpu

ROWS, IDS = runtime.IMPORT_ROWS, runtime.IMPORT_IDS
F32, U32 = np.float32, np.uint32
POS_VEL = [(A.POSITION.id, 0), (A.VELOCITY.id, 16)]          # stride 32: dwords 3 and 7 are covered by no field
TRAIL_ATTRS = [A.POSITION.id, A.VELOCITY.id, A.AGE.id, A.LIFETIME.id, A.COLOR.id]
DEAD = 0x0DEAD0DE                                            # what every dead slot holds before an import, in every plane


def make(cap, asset=None, slot_base=0, **options):
    ctx = bh.Context(0)
    for o, v in options.items():
        ctx.set_option(o, v)
    asset = asset if asset is not None else effects.firework_trails(cap)
    fx = ctx.create_program(bh.lower(asset)).create_effect(slot_base=slot_base)
    return ctx, fx


def planes(fx, attrs=TRAIL_ATTRS):
    """attribute id -> [capacity, ncomp] words, from the host's read-back (synchronises)"""
    return {int(a): fx.read_attr(int(a)).view(U32).reshape(fx.capacity, -1).copy() for a in attrs}


def alive_mask(fx):
    m = np.zeros(fx.capacity, bool)
    m[fx.alive_list()] = True
    return m


def mark_dead_slots(fx, attrs=TRAIL_ATTRS):
    """every dead slot of every plane holds DEAD (through hnb_effect_write_attr): a write to a slot that is not addressed shows"""
    dead = ~alive_mask(fx)
    for a, p in planes(fx, attrs).items():
        p[dead] = DEAD
        fx.write_attr(a, p)
    return dead


def state_of(fx, asset):
    m = fx.metadata()
    keys = ["capacity", "alive_count", "max_update", "max_spawn", "indirect_write_index", "particle_counter", "instance_count", "dead_count"]
    return {"counters": {k: m[k] for k in keys}, "alive": fx.alive_list(), "dead": fx.dead_list(),
            "attrs": {a.name: fx.read_attr(a.id).view(U32) for a in stored_attrs(asset)}}


class Source:
    """Records on the device: `rec` [k, stride / 4] words at a 16-byte aligned address, the optional device count, and four sentinel-filled words of
    which the call may write the first two."""

    def __init__(self, rec, count=None):
        rec = np.ascontiguousarray(rec, U32)
        self.rec = rec
        self.buf = torch.from_numpy(np.concatenate([rec.reshape(-1), np.full(4, SENTINEL, U32)]).view(np.int32)).cuda()
        self.cnt = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
        self.n = None if count is None else torch.from_numpy(np.array([count], U32).view(np.int32)).cuda()
        torch.cuda.synchronize()            # (the fills run on torch's stream, the import on the simulation's)
        assert self.buf.data_ptr() % 16 == 0

    def counts(self):
        w = [int(x) for x in self.cnt.cpu().numpy().view(U32)]
        assert w[2:] == [SENTINEL, SENTINEL], "words behind out_count[1] were written"
        return w[:2]


def expect(before, fields, rec, slots, ok):
    """the planes after an import: `before` with the payload fields of the records rec[ok] at slots[ok] (no slot twice)"""
    assert len(np.unique(slots[ok])) == int(ok.sum())
    out = {a: p.copy() for a, p in before.items()}
    for attr, off in fields:
        if attr != A.ID.id:
            nc = runtime.ATTR_COMPONENTS[attr]
            out[attr][slots[ok]] = rec[ok, off // 4: off // 4 + nc]
    return out


def check_import(ctx, fx, fields, stride, rec, what, mode=ROWS, capacity=None, count=None, attrs=TRAIL_ATTRS, slot_base=0, src=None):
    """One import of the device records `rec` (every record the buffer holds: those at and past n are bait), synchronise, and hold every plane, the
    counts and the lists against the numpy model. -> (applied, skipped)"""
    fields = [(int(a), int(o)) for a, o in fields]
    before, alive, mask = planes(fx, attrs), fx.alive_list(), alive_mask(fx)
    src = Source(rec, count) if src is None else src
    cap_records = len(rec) if capacity is None else capacity
    fx.import_records(fields, src.buf.data_ptr(), stride, cap_records, mode, None if src.n is None else src.n.data_ptr(), src.cnt.data_ptr())
    ctx.synchronize()
    n = cap_records if count is None else min(cap_records, count)
    if mode == ROWS:
        n = min(n, len(alive))
        slots, ok = alive[:n], np.ones(n, bool)
    else:
        id_dw = next(o for a, o in fields if a == A.ID.id) // 4
        slots = (rec[:n, id_dw].astype(np.uint64) + 2 ** 32 - slot_base).astype(np.uint64) % 2 ** 32
        ok = slots < fx.capacity
        ok[ok] = mask[slots[ok].astype(np.int64)]
        slots = slots.astype(np.int64)
    want = expect(before, fields, rec[:n], slots, ok)
    after = planes(fx, attrs)
    for a in attrs:
        np.testing.assert_array_equal(after[int(a)], want[int(a)], err_msg=f"{what}: attribute {a}")
    assert src.counts() == [int(ok.sum()), n - int(ok.sum())], (what, src.counts(), int(ok.sum()), n)
    np.testing.assert_array_equal(fx.alive_list(), alive, err_msg=f"{what}: the list")
    return int(ok.sum()), n - int(ok.sum())


def exported_and_changed(fx, cap_records, slack=8):
    """{POSITION, VELOCITY} records of the alive list, changed ON THE DEVICE: y negated, 0.5 added to the x velocity. -> (the Export whose buffer holds
    them, their words on the host: the slack records keep the sentinel)"""
    ex = Export(POS_VEL, 32, cap_records, slack=slack).run(fx)
    torch.cuda.synchronize()                     # (the change runs on torch's stream)
    v = ex.dst[: cap_records * 8].view(torch.float32).view(-1, 8)
    n = ex.counts()[0]
    v[:n, 1].neg_()
    v[:n, 4] += 0.5
    torch.cuda.synchronize()
    return ex, ex.words()[: (cap_records + slack) * 8].reshape(-1, 8).copy()


# ---- tile and list edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 255, 256, 257, 4096, 4097, 10_000, 300_007])
def test_tile_and_list_edges_in_rows_mode(cap):
    """Nothing alive, 1, 256 and 257 alive, everything alive, and a permuted partial list in the other column after a die-off: {POSITION, VELOCITY}
    records, exported and changed on the device, come back; the addressed slots hold the new bits, every dead slot keeps the sentinel it was given,
    AGE, LIFETIME and COLOR keep every bit, out_count is {n, 0}."""
    ctx, fx = make(cap)
    f, have = 0, 0
    states = [c for c in (0, 1, 256, 257) if c <= cap] + [cap, "die-off"]
    for want in dict.fromkeys(states):
        if want == "die-off":
            for _ in range(4):                                   # lifetimes are 0.8 .. 1.2 s: a second later part of the burst is gone
                step(ctx, fx, f, 0, dt=0.25)
                f += 1
        elif want > have:
            step(ctx, fx, f, want - have)
            f += 1
            have = want
        dead = mark_dead_slots(fx)
        ex, rec = exported_and_changed(fx, cap)
        alive = fx.alive_list()
        n = len(alive)
        if want == "die-off":
            assert cap < 255 or (0 < n < cap and not np.array_equal(alive, np.arange(n)))               # a permuted, partial list
        else:
            assert n == want
        # the change as numpy makes it, from the planes: the device's records are these bits
        p = planes(fx, [A.POSITION.id, A.VELOCITY.id])
        pos, vel = p[A.POSITION.id][alive].view(F32).copy(), p[A.VELOCITY.id][alive].view(F32).copy()
        pos[:, 1] = -pos[:, 1]
        vel[:, 0] = vel[:, 0] + F32(0.5)
        np.testing.assert_array_equal(rec[:n, 0:3], pos.view(U32))
        np.testing.assert_array_equal(rec[:n, 4:7], vel.view(U32))
        assert (rec[n:] == SENTINEL).all()
        src = Source(rec)
        src.buf = ex.dst                                           # the exported buffer itself goes back
        applied, skipped = check_import(ctx, fx, POS_VEL, 32, rec, f"capacity {cap}, {want}", capacity=cap, src=src)
        assert (applied, skipped) == (n, 0)
        after = planes(fx)
        for a in TRAIL_ATTRS:
            assert (after[a][dead] == DEAD).all(), f"capacity {cap}, {want}: a dead slot of attribute {a} was written"
    assert fx.check()["ok"] == 1
    ctx.close()


# ---- strides and placement ----------------------------------------------------------------------------------------------------------------------------
def trails_mixed(capacity):
    """The firework's trails with a 4-component and a 2-component f32 attribute in the layout"""
    w = bh.ExprWriter()
    direction = w.rand(bh.VectorType.VEC3F).mul(w.lit(2.0)).sub(w.lit(1.0)).normalized()
    mods = [bh.SetAttributeModifier(A.POSITION, w.lit((0.0, 0.0, 0.0)).expr()),
            bh.SetAttributeModifier(A.VELOCITY, (direction * w.lit(40.0).uniform(w.lit(60.0))).expr()),
            bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr()),
            bh.SetAttributeModifier(A.LIFETIME, w.lit(0.8).uniform(w.lit(1.2)).expr()),
            bh.SetAttributeModifier(A.F32X4_0, (w.rand(bh.VectorType.VEC4F) * w.lit(8.0) - w.lit(4.0)).expr()),
            bh.SetAttributeModifier(A.F32X2_0, (w.rand(bh.VectorType.VEC2F) * w.lit(2.0)).expr())]
    asset = bh.EffectAsset(capacity, bh.SpawnerSettings.once(float(capacity)), w.finish()).with_name("trail42")
    for m in mods:
        asset = asset.init(m)
    return asset


SPECIAL = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF],
                   U32)   # NaNs of both signs (quiet, signalling, all ones), -0, +0, the infinities, the smallest denormals, the largest finite values


def garbage_records(rng, n, stride):
    """random words everywhere - the uncovered dwords too -, the special bit patterns through the first rows"""
    rec = rng.integers(0, 2 ** 32, (n, stride // 4), dtype=np.uint64).astype(U32)
    k = min(n, 3 * len(SPECIAL))
    rec[:k] = np.resize(SPECIAL, (k, stride // 4)) if k else rec[:k]
    rec[:k:3] = np.roll(rec[:k:3], 1, axis=1)
    return rec


STRIDE_CASES = [
    (4, [(A.LIFETIME.id, 0)]),                                                             # one scalar
    (12, [(A.POSITION.id, 0)]),
    (36, [(A.VELOCITY.id, 4), (A.COLOR.id, 20), (A.AGE.id, 32)]),                          # odd dword offsets, uncovered dwords 0, 4, 6, 7
    (48, [(A.POSITION.id, 4), (A.COLOR.id, 20), (A.VELOCITY.id, 28), (A.AGE.id, 44)]),
    (132, [(A.POSITION.id, 4), (A.LIFETIME.id, 128)]),                                     # the 128-row tile
    (256, [(A.LIFETIME.id, 252), (A.POSITION.id, 0)]),                                     # a field in the last dword of the largest record
]


@pytest.mark.parametrize("stride,fields", STRIDE_CASES, ids=[str(s) for s, _ in STRIDE_CASES])
def test_strides_and_placement_copy_bits_and_ignore_uncovered_dwords(stride, fields):
    cap, n = 1000, 777                                             # several tiles of either size, the last partial
    ctx, fx = make(cap)
    step(ctx, fx, 0, n)
    rng = np.random.default_rng(stride)
    mark_dead_slots(fx)
    assert check_import(ctx, fx, fields, stride, garbage_records(rng, n + 5, stride), f"stride {stride}") == (n, 0)
    ids = (fields + [(A.ID.id, 0 if stride == 36 else stride - 8)]) if stride in (36, 48, 132) else None        # ... and by id, the ID in an uncovered dword
    if ids:
        rec = garbage_records(rng, n, stride)
        order = rng.permutation(fx.alive_list())
        rec[:, ids[-1][1] // 4] = order
        assert check_import(ctx, fx, ids, stride, rec, f"stride {stride}, by id", mode=IDS) == (n, 0)
    ctx.close()


def test_integer_and_four_and_two_component_attributes_arrive_as_their_bits():
    cap, n = 600, 517
    asset = trails_mixed(cap)
    attrs = [a.id for a in stored_attrs(asset)]
    assert {runtime.ATTR_COMPONENTS[a] for a in attrs} == {1, 2, 3, 4}
    ctx, fx = make(cap, asset)
    step(ctx, fx, 0, n)
    rng = np.random.default_rng(42)
    mark_dead_slots(fx, attrs)
    fields = [(A.F32X4_0.id, 4), (A.F32X2_0.id, 24), (A.POSITION.id, 32)]                 # stride 48: the vec4 at an odd dword of the record
    assert check_import(ctx, fx, fields, 48, garbage_records(rng, n, 48), "vec4 + vec2 + vec3", attrs=attrs) == (n, 0)
    fields = [(A.ID.id, 0), (A.F32X4_0.id, 4), (A.F32X2_0.id, 20)]                        # stride 28
    rec = garbage_records(rng, n, 28)
    rec[:, 0] = rng.permutation(fx.alive_list())
    assert check_import(ctx, fx, fields, 28, rec, "vec4 + vec2 by id", mode=IDS, attrs=attrs) == (n, 0)
    ctx.close()
    ctx, fx = make(cap)                                            # COLOR: an integer attribute
    step(ctx, fx, 0, n)
    assert not runtime.ATTR_IS_FLOAT[A.COLOR.id]
    rec = garbage_records(rng, n, 8)
    assert check_import(ctx, fx, [(A.COLOR.id, 4)], 8, rec, "COLOR") == (n, 0)
    np.testing.assert_array_equal(fx.read_attr(A.COLOR.id).reshape(-1)[fx.alive_list()], rec[:, 1])
    ctx.close()


# ---- counts -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [ROWS, IDS], ids=["rows", "ids"])
def test_counts_and_clamps_never_read_a_record_at_or_past_n(mode):
    cap, n = 1000, 600
    ctx, fx = make(cap)
    step(ctx, fx, 0, n)
    mark_dead_slots(fx)
    rng = np.random.default_rng(7)
    fields, stride = ([(A.POSITION.id, 0), (A.AGE.id, 12)], 16) if mode == ROWS else ([(A.POSITION.id, 0), (A.ID.id, 12), (A.AGE.id, 16)], 20)

    def records(k):                                                # k records of alive particles (each one once); in IDS mode the bait behind n names alive slots too
        rec = garbage_records(rng, k, stride)
        if mode == IDS:
            rec[:, 3] = np.resize(rng.permutation(fx.alive_list()), k)
        return rec

    for what, k, capacity, count, applied in (
            ("*src_count below alive_count", n + 40, n + 40, 257, 257),
            ("*src_count equal to alive_count", n + 40, n + 40, n, n),
            ("*src_count above alive_count", n + 40, n + 40, n + 33, n if mode == ROWS else None),
            ("src_capacity_records the smaller clamp", n + 40, 129, 400, 129),
            ("src_capacity_records alone", n + 40, 255, None, 255),
            ("*src_count of 0", n, n, 0, 0),
            ("src_capacity_records of 0", n, 0, None, 0),
            ("*src_count of 0xFFFFFFFF", n, n, 2 ** 32 - 1, n)):
        if applied is None:                                        # IDS reads n + 33 records: no id twice
            k = capacity = n
            applied = n
        got = check_import(ctx, fx, fields, stride, records(k), f"{what}", mode=mode, capacity=capacity, count=count)
        assert got == (applied, 0), (what, got)
    ctx.close()


# ---- IDS mode -----------------------------------------------------------------------------------------------------------------------------------------
ID_POS_VEL = [(A.ID.id, 0), (A.POSITION.id, 4), (A.VELOCITY.id, 16)]     # stride 28


@pytest.mark.parametrize("cap", [300, 4097])
def test_ids_mode_takes_the_sorted_filtered_and_binned_exports_straight_back(cap):
    """An effect whose slot_base is not 0, on torch's stream: export (sorted | filtered | binned) -> a change on the device -> import, with no
    synchronisation in between; the filtered export's device out_count is the import's src_count. Then a subset, skipped records and the ID alone."""
    base = 70_000
    ctx, fx = make(cap, slot_base=base)
    step(ctx, fx, 0, cap)
    for f in range(1, 5):
        step(ctx, fx, f, 0, dt=0.25)                               # lifetimes are 0.8 .. 1.2 s: part of the burst is gone, dead slots exist
    ctx.synchronize()
    alive = fx.alive_list()
    n = len(alive)
    assert 0 < n < cap
    dead = mark_dead_slots(fx)
    life = fx.read_attr(A.LIFETIME.id).reshape(-1)
    lo, hi = F32(0.0), np.sort(life[alive])[n // 2]
    kept = int(((life[alive] >= lo) & (life[alive] <= hi)).sum())
    assert 0 < kept < n
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    table = torch.zeros(8 + 2 + 8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    exports = {"sorted": lambda ex: fx.export_sorted(ex.fields, ex.dst.data_ptr(), 28, cap, ex.cnt.data_ptr(), key="depth", v=(0.3, -0.5, 0.8)),
               "filtered": lambda ex: fx.export_filtered(ex.fields, ex.dst.data_ptr(), 28, cap, ex.cnt.data_ptr(), kind="attr_range", attr=A.LIFETIME.id, lo=float(lo), hi=float(hi)),
               "binned": lambda ex: fx.export_binned(ex.fields, ex.dst.data_ptr(), 28, cap, ex.cnt.data_ptr(), dims=(2, 2, 2), origin=(-100, -100, -100), inv_cell=(0.01, 0.01, 0.01),
                                                     cell_start_ptr=table.data_ptr())}
    for round_, (name, export) in enumerate(exports.items()):
        before = planes(fx)
        ex = Export(ID_POS_VEL, 28, cap)
        out = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            export(ex)
            v = ex.dst[: cap * 7].view(torch.float32).view(-1, 7)
            v[:, 2].neg_()                                          # y of every record the buffer can hold: the records behind the count are never applied
            v[:, 4] += float(round_ + 1)
            fx.import_records(ID_POS_VEL, ex.dst.data_ptr(), 28, cap, IDS, ex.cnt.data_ptr(), out.data_ptr())     # src_count: the export's out_count[0], still on the device
        ctx.synchronize()
        m = kept if name == "filtered" else n
        assert ex.counts()[0] == m and [int(x) for x in out.cpu().numpy().view(U32)] == [m, 0, SENTINEL, SENTINEL], (name, ex.counts(), out)
        rec = ex.words()[: m * 7].reshape(m, 7)
        slots = rec[:, 0].astype(np.int64) - base
        assert (np.sort(slots) == np.sort(alive)).all() if name != "filtered" else set(slots) < set(alive)
        want = expect(before, ID_POS_VEL, rec, slots, np.ones(m, bool))
        pos = before[A.POSITION.id][slots].view(F32).copy()
        pos[:, 1] = -pos[:, 1]
        np.testing.assert_array_equal(rec[:, 1:4], pos.view(U32), err_msg=name)                     # the records are the exported particles, changed
        after = planes(fx)
        for a in TRAIL_ATTRS:
            np.testing.assert_array_equal(after[a], want[a], err_msg=f"{name}: attribute {a}")
            assert (after[a][dead] == DEAD).all()
    ctx.set_stream(None)
    torch.cuda.synchronize()
    # a subset of the records, in any order
    rng = np.random.default_rng(cap)
    some = rng.permutation(alive)[: n // 3]
    rec = garbage_records(rng, len(some), 28)
    rec[:, 0] = some + base
    assert check_import(ctx, fx, ID_POS_VEL, 28, rec, "a subset", mode=IDS, slot_base=base) == (len(some), 0)
    # skipped records between applied ones: dead slots, slot_base + capacity, below slot_base, 0xFFFFFFFF, 0
    dead_slots = np.flatnonzero(dead)
    bad = np.concatenate([dead_slots[:5] + base, [base + cap, base + cap + 1, base - 1, 0, 2 ** 32 - 1, base + 2 ** 31]]).astype(np.uint64)
    good = rng.permutation(alive)[:40].astype(np.uint64) + base
    ids = rng.permutation(np.concatenate([bad, good]))
    rec = garbage_records(rng, len(ids), 28)
    rec[:, 0] = ids.astype(U32)
    assert check_import(ctx, fx, ID_POS_VEL, 28, rec, "skipped records", mode=IDS, slot_base=base) == (40, len(bad))
    # the ID as the only field: every plane is untouched (check_import compares them all), the ids are classified
    assert check_import(ctx, fx, [(A.ID.id, 4)], 8, rec[:, [1, 0]], "the ID alone", mode=IDS, slot_base=base) == (40, len(bad))
    after = planes(fx)
    for a in TRAIL_ATTRS:
        assert (after[a][dead] == DEAD).all()
    ctx.close()


# ---- the proofs are reset -----------------------------------------------------------------------------------------------------------------------------
AGE_LIFE = [(A.AGE.id, 0), (A.LIFETIME.id, 4)]


def run_stretch(pairs, f, assets, what):
    """30 frames on every (ctx, fx), a hnb_simulate_steps call of 8 among them; the states are compared after every stretch. -> the next frame"""
    dt = 1 / 30

    def compare(tag):
        for c, _ in pairs:
            c.synchronize()
        ref = state_of(pairs[0][1], assets)
        for c, fx in pairs[1:]:
            assert_same_state(ref, state_of(fx, assets), f"{what}, {tag}")
            d = pairs[0][1].compare(fx)
            assert d["equal"] == 1, (what, tag, d)

    for stretch, k in (("single", 11), ("steps", 8), ("single", 11)):
        for c, fx in pairs:
            if stretch == "steps":
                fx.set_frames_ahead([0] * k, [frame_seed(f + j) for j in range(k)])
                c.simulate_steps([(dt, (f + j) * dt) for j in range(k)])
            else:
                for j in range(k):
                    step(c, fx, f + j, 0, dt=dt)
        f += k
        compare(f"frame {f}")
    return f


def host_twin_write(fx, fields, rec, n):
    """what the import of rec[:n] in ROWS mode does, through the host path: read_attr + numpy + hnb_effect_write_attr"""
    alive = fx.alive_list()[:n]
    for attr, off in fields:
        nc = runtime.ATTR_COMPONENTS[attr]
        p = fx.read_attr(attr).view(U32).reshape(fx.capacity, nc).copy()
        p[alive] = rec[: len(alive), off // 4: off // 4 + nc]
        fx.write_attr(attr, p)


@pytest.mark.parametrize("cohort", [1, 3, 0], ids=["lean", "auto", "off"])
def test_later_frames_compute_what_they_would_after_write_attr(cohort):
    """70,000 slots, past the 65,536 threshold of HNB_AGE_COHORT_AUTO. LIFETIME values shorter than the chunks' published bounds and AGE values that
    include negative ones, imported behind frames that published those bounds; the twin makes the same writes through the host path."""
    cap = 70_000
    asset = effects.firework_trails(cap)
    (ca, fa), (cb, fb) = [make(cap, age_cohort=cohort) for _ in range(2)]
    for f in range(6):
        for c, fx in ((ca, fa), (cb, fb)):
            step(c, fx, f, cap if f == 0 else 0, dt=1 / 30)
    f = 6
    rng = np.random.default_rng(cohort)
    n = cap - 4099                                                  # the last rows keep their values
    rec = np.zeros((n, 2), U32)
    rec[:, 0] = rng.uniform(-0.2, 0.3, n).astype(F32).view(U32)      # ages, a part of them negative
    rec[:, 1] = rng.uniform(0.31, 0.9, n).astype(F32).view(U32)      # lifetimes from 0.31 s: below the bound of 0.8 s every chunk published, so particles die from the next frames on
    rec[::7, 1] = F32(0.05).view(U32)                                # ... and some at once: age >= lifetime in the next update
    src = Source(rec)
    fa.import_records(AGE_LIFE, src.buf.data_ptr(), 8, n, ROWS, None, src.cnt.data_ptr())            # no synchronisation in front or behind
    host_twin_write(fb, AGE_LIFE, rec, n)
    f = run_stretch([(ca, fa), (cb, fb)], f, asset, f"cohort {cohort}")
    assert src.counts() == [n, 0]
    alive = fa.alive_count()
    assert 0 < alive < cap and fa.check()["ok"] == 1                 # particles died on the way, in both
    ca.close(); cb.close()


@pytest.mark.parametrize("cohort", [1, 3, 0], ids=["lean", "auto", "off"])
def test_round_trip_and_partial_imports_under_the_age_cohorts(cohort):
    cap = 70_000
    asset = effects.firework_trails(cap)
    (ca, fa), (cb, fb) = [make(cap, age_cohort=cohort) for _ in range(2)]
    for f in range(6):
        for c, fx in ((ca, fa), (cb, fb)):
            step(c, fx, f, cap if f == 0 else 0, dt=1 / 30)
    f = 6
    # records imported unchanged: equal to a twin that never imported, at once and 30 frames later
    fields = [(A.POSITION.id, 0), (A.AGE.id, 12), (A.LIFETIME.id, 16), (A.VELOCITY.id, 20)]
    ex = Export(fields, 32, cap).run(fa)
    out = torch.full((4,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fa.import_records(fields, ex.dst.data_ptr(), 32, cap, ROWS, ex.cnt.data_ptr(), out.data_ptr())
    ca.synchronize(); cb.synchronize()
    assert [int(x) for x in out.cpu().numpy().view(U32)][:2] == [cap, 0]
    assert_same_state(state_of(fb, asset), state_of(fa, asset), "round trip, at once")
    f = run_stretch([(ca, fa), (cb, fb)], f, asset, f"round trip, cohort {cohort}")
    ca.close(); cb.close()
    # only POSITION imported: AGE read afterwards is unchanged. Only AGE imported for half the rows: the other half's ages are what materialise shows.
    (ca, fa), (cb, fb) = [make(cap, age_cohort=cohort) for _ in range(2)]
    for f in range(6):
        for c, fx in ((ca, fa), (cb, fb)):
            step(c, fx, f, cap if f == 0 else 0, dt=1 / 30)
    assert fa.device_view().stale_attr_mask == ((1 << A.AGE.id) if cohort == 1 else 0)
    age = F32(0.0)
    for _ in range(6):
        age = age + F32(1 / 30)
    rng = np.random.default_rng(3)
    pos = rng.uniform(-5, 5, (cap, 3)).astype(F32).view(U32)
    src = Source(pos)
    fa.import_records([(A.POSITION.id, 0)], src.buf.data_ptr(), 12, cap, ROWS, None, src.cnt.data_ptr())
    host_twin_write(fb, [(A.POSITION.id, 0)], pos, cap)
    ca.synchronize()
    got = fa.read_attr(A.AGE.id).reshape(-1)
    assert (got == age).all() and src.counts() == [cap, 0]
    half = cap // 2
    ages = rng.uniform(0.0, 0.1, (half, 1)).astype(F32).view(U32)
    src = Source(ages)
    fa.import_records([(A.AGE.id, 0)], src.buf.data_ptr(), 4, half, ROWS, None, src.cnt.data_ptr())
    host_twin_write(fb, [(A.AGE.id, 0)], ages, half)
    fa.materialise([A.AGE.id])
    ca.synchronize()
    alive = fa.alive_list()
    got = fa.read_attr(A.AGE.id).reshape(-1)
    np.testing.assert_array_equal(got[alive[:half]].view(U32), ages[:, 0])
    assert (got[alive[half:]] == age).all() and src.counts() == [half, 0]
    run_stretch([(ca, fa), (cb, fb)], 6, asset, f"partial imports, cohort {cohort}")
    ca.close(); cb.close()


# ---- a ribbon program with a ring list ----------------------------------------------------------------------------------------------------------------
def test_age_imported_through_a_non_zero_ring_head_then_frames_with_the_sort():
    cap = 4096
    asset = effects.ribbon(cap)
    pairs = []
    for _ in range(2):
        ctx = bh.Context(0)
        ctx.set_option("ring_lists", 1)
        pairs.append((ctx, ctx.create_program(bh.lower(asset)).create_effect(), bh.EffectSpawner(asset.spawner), bh.Pcg32()))

    def frames(first, count):
        for f in range(first, first + count):
            for ctx, fx, sp, rng in pairs:
                ctx.frame_begin(1 / 60, f / 60)
                fx.set_frame(sp.tick(1 / 60, rng), frame_seed(f))
                ctx.simulate()

    (ca, fa, _, _), (cb, fb, _, _) = pairs
    done = 0
    for done in range(100, 200, 7):                                    # until the head stands somewhere inside the column
        frames(done - (100 if done == 100 else 7), 100 if done == 100 else 7)
        ca.synchronize(); cb.synchronize()
        m = _device_meta(fa)
        if m.list_column >> 1 != 0:
            break
    n = m.alive_count
    assert m.list_column >> 1 != 0 and n > 64                          # the list is kept as a ring and its head has moved
    rng = np.random.default_rng(9)
    alive = fa.alive_list()
    age = fa.read_attr(A.AGE.id).reshape(-1)[alive]
    new = (age * rng.uniform(0.2, 1.0, n).astype(F32)).astype(F32)
    new[::5] = -new[::5] - F32(0.01)                                   # negative ages: they change key order when they cross zero later
    rec = new.view(U32).reshape(-1, 1)
    src = Source(rec)
    fa.import_records([(A.AGE.id, 0)], src.buf.data_ptr(), 4, n + 3, ROWS, None, src.cnt.data_ptr())
    host_twin_write(fb, [(A.AGE.id, 0)], rec, n)
    ca.synchronize()
    assert src.counts() == [n, 0]
    np.testing.assert_array_equal(fa.read_attr(A.AGE.id).reshape(-1)[alive].view(U32), rec[:, 0])
    for k in range(4):
        frames(done + 5 * k, 5)
        ca.synchronize(); cb.synchronize()
        assert_same_state(state_of(fb, asset), state_of(fa, asset), f"ribbon, frame {done + 5 * k + 5}")     # the lists bit for bit
    ca.close(); cb.close()


# ---- stream order -------------------------------------------------------------------------------------------------------------------------------------
def test_twenty_rounds_of_simulate_export_change_import_without_a_synchronisation():
    """The context runs on torch's stream: simulate -> export -> a change of the records in torch -> import -> simulate, 20 rounds into ONE buffer and
    nothing synchronises the importing context in between. The replica does every round through the host path and is compared at the end."""
    cap, rounds, dt = 5_000, 20, 1 / 20
    asset = effects.firework_trails(cap, spawner=bh.SpawnerSettings.rate(3000.0))
    (ca, fa), (cb, fb) = [make(cap, asset) for _ in range(2)]
    stream = torch.cuda.Stream()
    ex = Export(POS_VEL, 32, cap)
    out = torch.full((rounds, 2), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ca.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(5)
    spawns = [int(rng.integers(50, 400)) for _ in range(2 * rounds)]
    counts = []
    for r in range(rounds):
        with torch.cuda.stream(stream):
            step(ca, fa, 2 * r, spawns[2 * r], dt)
            ex.run(fa)
            v = ex.dst[: cap * 8].view(torch.float32).view(-1, 8)
            v[:, 5].neg_()                                          # the y velocity
            v[:, 0] += 0.25                                         # the x position
            fa.import_records(POS_VEL, ex.dst.data_ptr(), 32, cap, ROWS, ex.cnt.data_ptr(), out[r].data_ptr())
            step(ca, fa, 2 * r + 1, spawns[2 * r + 1], dt)
        step(cb, fb, 2 * r, spawns[2 * r], dt)
        alive = fb.alive_list()
        counts.append(len(alive))
        pos, vel = fb.read_attr(A.POSITION.id), fb.read_attr(A.VELOCITY.id)
        vel[alive, 1] = -vel[alive, 1]
        pos[alive, 0] = pos[alive, 0] + F32(0.25)
        fb.write_attr(A.POSITION.id, pos)
        fb.write_attr(A.VELOCITY.id, vel)
        step(cb, fb, 2 * r + 1, spawns[2 * r + 1], dt)
    ca.synchronize(); cb.synchronize()
    assert_same_state(state_of(fb, asset), state_of(fa, asset), "after 20 rounds")
    assert [[int(x) for x in row] for row in out.cpu().numpy().view(U32)] == [[c, 0] for c in counts]
    assert max(counts) > 1000 and any(b < a for a, b in zip(counts, counts[1:])), counts           # particles died on the way
    ca.set_stream(None)
    torch.cuda.synchronize()
    ca.close(); cb.close()


# ---- neighbours ---------------------------------------------------------------------------------------------------------------------------------------
def test_imports_into_one_instance_leave_the_other_instances_slabs_alone():
    cap, n_inst = 4096, 5
    attrs = [A.POSITION.id, A.VELOCITY.id, A.AGE.id, A.LIFETIME.id]
    ctx = bh.Context(0)
    prog = ctx.create_program(bh.lower(effects.instancing(cap, rate=cap / 0.25)))
    fxs = [prog.create_effect(slot_base=1000 * k) for k in range(n_inst)]
    spawns = [37, 0, 700, 301, 1234]                               # instance 1 stays empty
    for f in range(6):
        ctx.frame_begin(1 / 60, f / 60)
        if f == 3:
            fxs[3].set_simulated(False)                            # frozen from here on
        for k, fx in enumerate(fxs):
            fx.set_frame(spawns[k] if f < 4 else 0, frame_seed(f * n_inst + k))
        ctx.simulate()
    ctx.synchronize()
    rng = np.random.default_rng(11)
    snapshot = lambda: [(planes(fx, attrs), fx.alive_list(), fx.dead_list(), fx.metadata()["alive_count"]) for fx in fxs]
    for k, mode in ((2, ROWS), (3, IDS), (3, ROWS), (2, IDS)):      # instance 2, and the frozen one
        before = snapshot()
        n = before[k][3]
        assert n > 0
        fields, stride = (POS_VEL, 32) if mode == ROWS else ([(A.ID.id, 12), (A.POSITION.id, 0), (A.VELOCITY.id, 16)], 32)
        rec = garbage_records(rng, n, stride)
        if mode == IDS:
            rec[:, 3] = rng.permutation(before[k][1]) + 1000 * k
        assert check_import(ctx, fxs[k], fields, stride, rec, f"instance {k}", mode=mode, attrs=attrs, slot_base=1000 * k) == (n, 0)
        after = snapshot()
        for j in range(n_inst):
            if j != k:
                for a in attrs:
                    np.testing.assert_array_equal(after[j][0][a], before[j][0][a], err_msg=f"import into {k}: instance {j}, attribute {a}")
            np.testing.assert_array_equal(after[j][1], before[j][1]); np.testing.assert_array_equal(after[j][2], before[j][2])
            assert after[j][3] == before[j][3]
    # the empty instance: nothing is applied, by row or by id (ids that name its slots: all dead)
    before = snapshot()
    assert check_import(ctx, fxs[1], POS_VEL, 32, garbage_records(rng, 50, 32), "the empty instance", attrs=attrs) == (0, 0)
    rec = garbage_records(rng, 50, 32)
    rec[:, 3] = 1000 + np.arange(50)
    assert check_import(ctx, fxs[1], [(A.ID.id, 12), (A.POSITION.id, 0), (A.VELOCITY.id, 16)], 32, rec, "the empty instance by id", mode=IDS, attrs=attrs, slot_base=1000) == (0, 50)
    after = snapshot()
    for j in range(n_inst):
        for a in attrs:
            np.testing.assert_array_equal(after[j][0][a], before[j][0][a])
    # the frozen instance thaws and the program runs on
    fxs[3].set_simulated(True)
    for f in range(6, 10):
        ctx.frame_begin(1 / 60, f / 60)
        for k, fx in enumerate(fxs):
            fx.set_frame(0, frame_seed(f * n_inst + k))
        ctx.simulate()
    ctx.synchronize()
    assert all(fx.check()["ok"] == 1 for fx in fxs)
    ctx.close()


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_on_a_live_effect_enqueue_nothing():
    cap = 1000
    asset = effects.firework_trails(cap)
    (ca, fa), (cb, fb) = [make(cap) for _ in range(2)]
    for c, fx in ((ca, fa), (cb, fb)):
        step(c, fx, 0, cap)
        step(c, fx, 1, 0, dt=0.05)
    rng = np.random.default_rng(1)
    src = Source(garbage_records(rng, cap, 32))
    before = planes(fa)
    P, V, AGE, ID = A.POSITION.id, A.VELOCITY.id, A.AGE.id, A.ID.id
    ids = [(ID, 12), (P, 0), (V, 16)]
    bad = {
        "PARTICLE_COUNTER": dict(fields=[(A.PARTICLE_COUNTER.id, 0)]),
        "an attribute the layout lacks": dict(fields=[(P, 0), (A.SIZE.id, 12)]),
        "overlapping fields": dict(fields=[(P, 0), (AGE, 8)]),
        "a field past the stride": dict(fields=[(P, 0), (V, 24)]),
        "a field at an odd byte": dict(fields=[(AGE, 2)]),
        "a misaligned src": dict(src=src.buf.data_ptr() + 4),
        "a NULL src": dict(src=0),
        "no field": dict(fields=[]),
        "too many fields": dict(fields=[(AGE, 0)] * 17, stride=128),
        "a stride that is no multiple of 4": dict(stride=34),
        "a stride above 256": dict(fields=[(AGE, 0)], stride=260),
        "an unknown attribute id": dict(fields=[(39, 0)]),
        "an unknown mode": dict(mode=2),
        "the ID as a field of ROWS": dict(fields=ids),
        "IDS without an ID": dict(mode=IDS),
        "IDS with two IDs": dict(fields=ids + [(ID, 28)], mode=IDS),
        "IDS without src_count and more than 2^32 - 1 records": dict(fields=ids, mode=IDS, capacity=2 ** 32, count_ptr=None),
        "a misaligned out_count": dict(out=src.cnt.data_ptr() + 2),
    }
    count = torch.tensor([cap], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for what, kw in bad.items():
        with pytest.raises(bh.HanabiError) as ei:
            fa.import_records(kw.get("fields", POS_VEL), kw.get("src", src.buf.data_ptr()), kw.get("stride", 32), kw.get("capacity", cap), kw.get("mode", ROWS),
                              kw.get("count_ptr", count.data_ptr()), kw.get("out", src.cnt.data_ptr()))
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what      # HNB_ERR_INVALID_ARG, with text
    d = runtime.import_desc(POS_VEL, src.buf.data_ptr(), 32, cap, ROWS, count.data_ptr(), src.cnt.data_ptr())
    lib = runtime.load_library()
    for field, value in (("struct_size", 176), ("flags", 1), ("reserved", 1)):
        setattr(d, field, value)
        assert lib.hnb_effect_import(fa._h, C.byref(d)) == -1, field
        setattr(d, field, C.sizeof(runtime.ImportDesc) if field == "struct_size" else 0)
    d.fields[1].reserved = 1
    assert lib.hnb_effect_import(fa._h, C.byref(d)) == -1 and b"field 1" in lib.hnb_last_error()
    d.fields[1].reserved = 0
    ca.synchronize()
    after = planes(fa)
    for a in TRAIL_ATTRS:
        np.testing.assert_array_equal(after[a], before[a])
    assert [int(x) for x in src.cnt.cpu().numpy().view(U32)] == [SENTINEL] * 4
    for f in range(2, 12):                                         # ... and the following frames are the twin's, which was never asked
        for c, fx in ((ca, fa), (cb, fb)):
            step(c, fx, f, 0, dt=0.05)
    ca.synchronize(); cb.synchronize()
    assert_same_state(state_of(fb, asset), state_of(fa, asset), "after the refused calls")
    assert lib.hnb_effect_import(fa._h, C.byref(d)) == 0          # the same description, unbroken, is accepted
    ca.synchronize()
    n = fa.alive_count()
    assert src.counts() == [n, 0] and 0 < n
    ca.close(); cb.close()
