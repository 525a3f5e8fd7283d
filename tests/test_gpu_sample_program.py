"""hnb_program_sample on the GPU (include/hanabi_amd_sample_program.h): hnb_effect_sample for every instance of a program in one call. The expectation
is the numpy restatement of tests/test_sample_abi.py (np_sample / np_store, through tests/test_gpu_sample.py's `expected`) applied per instance over the
host's read-back of that instance's planes and alive list, with that instance's field; whole planes are compared bit for bit (dead slots, outside
particles and unnamed components included), and where the restatement gives a NaN the result must be a NaN. There is no tolerance anywhere. Every
instance is planted from its own seed, and unless a case is about the shared field every instance reads its own field: a kernel that mixes up
instances or fields cannot pass. The fields, the totals and the per-instance rows each sit between guard words filled with a sentinel; the padding
between two instances' fields holds NaNs that must reach no plane.

Before comparing, each main case asserts tests/test_gpu_sample.py's guard_conditions on the restatement alone, per instance: a quarter of the alive
particles are sampled with a clamped corner, the outside bin is not empty, more than half of the sampled particles change a destination's bits.
Instances with fewer than MIN_GUARDED alive particles (capacities 1, 3 and 4, and the smallest bursts) cannot hold three such populations at once; for
them the case asserts that over its instances at least one particle is sampled and changed (the seeds were chosen so, on the CPU)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, frame_seed
from test_bounds_abi import trails_vec4
from test_gpu_export import SENTINEL
from test_gpu_import import planes
import test_gpu_program_export_sorted as pes
from test_gpu_sample import ATTRS4, CH4, GUARD, HALF, assert_planes, expected, guard_conditions, plant, random_field
from test_sample_abi import ADD, NEAREST, SET, TILE, TRILINEAR
from test_sample_program_abi import program_sample_plan

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
MODES = (NEAREST, TRILINEAR)
CAPS = (1, 3, 4, 255, 4096, 4097, 8193)          # a lone tail, a full tile, a tile plus 1..3 slots
DIMS = (5, 4, 3)
MIN_GUARDED = 100
SENT = U32(SENTINEL & 0xFFFFFFFF)


def guarded(n_words):
    return torch.full((n_words + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")


class ProgField:
    """The fields of one call - values[i]: [n_cells, k] of instance i, `stride` f32 elements apart (0: values[0] for every instance) - the totals and
    the per-instance rows, each between guard words. The words between two instances' fields are NaNs."""

    def __init__(self, dims, values, n_inst, stride, totals=True, rows=True, origin=(-HALF,) * 3, inv_cell=None):
        self.dims = tuple(int(d) for d in dims)
        self.n_cells = self.dims[0] * self.dims[1] * self.dims[2]
        self.origin = np.asarray(origin, F32)
        self.inv_cell = np.asarray(inv_cell if inv_cell is not None else [d / (2 * HALF) for d in self.dims], F32)
        self.values = [np.ascontiguousarray(v, F32).reshape(self.n_cells, -1) for v in values]
        self.k = self.values[0].shape[1]
        self.n_inst, self.stride = n_inst, stride
        row = self.n_cells * self.k
        assert len(self.values) == (1 if stride == 0 else n_inst) and (stride == 0 or (stride % 4 == 0 and stride >= row))
        body = np.full(row if stride == 0 else (n_inst - 1) * stride + row, np.nan, F32)
        for i, v in enumerate(self.values):
            body[i * stride: i * stride + row] = v.reshape(-1)
        words = np.full(body.size + 2 * GUARD, SENTINEL, np.int64).astype(U32)
        words[GUARD: GUARD + body.size] = body.view(U32)
        self.words = words
        self.buf = torch.from_numpy(words.view(np.int32)).cuda()
        self.totals = guarded(4) if totals else None
        self.rows = guarded(4 * n_inst) if rows else None
        torch.cuda.synchronize()                 # (the copies run on torch's stream, the call on the simulation's)

    def args(self):
        return dict(dims=self.dims, origin=self.origin, inv_cell=self.inv_cell, field_ptr=self.buf.data_ptr() + 4 * GUARD, field_instance_stride=self.stride,
                    stats_ptr=self.totals.data_ptr() + 4 * GUARD if self.totals is not None else None,
                    instance_stats_ptr=self.rows.data_ptr() + 4 * GUARD if self.rows is not None else None)

    def field_ptr_of(self, i):
        return self.buf.data_ptr() + 4 * GUARD + 4 * i * self.stride

    def of(self, i):
        """what tests/test_gpu_sample.py's `expected` reads of a Field, for instance i"""
        v = self.values[0 if self.stride == 0 else i]
        return types.SimpleNamespace(dims=self.dims, origin=self.origin, inv_cell=self.inv_cell, cells=lambda: v)

    def read_stats(self):
        """-> (totals [4] or None, rows [n_inst, 4] or None), and asserts the guard words on both sides of each and the whole field buffer"""
        np.testing.assert_array_equal(self.buf.cpu().numpy().view(U32), self.words, err_msg="the fields or the words next to them were written")
        out = []
        for t, n in ((self.totals, 4), (self.rows, 4 * self.n_inst)):
            if t is None:
                out.append(None)
                continue
            raw = t.cpu().numpy().view(U32)
            assert (raw[:GUARD] == SENT).all() and (raw[GUARD + n:] == SENT).all(), "words next to a stats buffer were written"
            out.append(raw[GUARD: GUARD + n].reshape(-1, 4) if t is self.rows else raw[GUARD: GUARD + 4])
        return out

    def untouched(self):
        ok = bool((self.buf.cpu().numpy().view(U32) == self.words).all())
        return ok and all(t is None or bool((t.cpu().numpy().view(U32) == SENT).all()) for t in (self.totals, self.rows))


def fields_for(dims, k, n_inst, seed, stride=None, **kw):
    """a field per instance from its own seed; stride None: exactly n_cells * k rounded up to 4"""
    n = dims[0] * dims[1] * dims[2]
    if stride is None:
        stride = -(-n * k // 4) * 4
    return ProgField(dims, [random_field(dims, k, seed + 17 * i) for i in range(1 if stride == 0 else n_inst)], n_inst, stride, **kw)


def check_program_sample(ctx, prog, fxs, pf, channels, mode, scale, what, attrs=ATTRS4, guards=True):
    """one call against the restatement per instance: planes, totals, rows, guard words -> (stats [n_inst, 4], infos)"""
    exp = [expected(fx, pf.of(i), channels, mode, scale, attrs) for i, fx in enumerate(fxs)]
    small_changed = 0
    for i, (_, _, _, info) in enumerate(exp):
        if not guards:
            continue
        if int(info["alive"].sum()) >= MIN_GUARDED:
            guard_conditions(info)
        else:
            assert not (info["changed"] & ~info["wr"]).any()
            small_changed += int((info["changed"] & info["wr"]).sum())
    prog.sample_all(channels=channels, mode=mode, scale=scale, **pf.args())
    ctx.synchronize()
    for i, (fx, (_, want, _, info)) in enumerate(zip(fxs, exp)):
        assert_planes(fx, want, info, f"{what}, instance {i}")
    stats = np.array([e[2] for e in exp], U32).reshape(len(fxs), 4)
    totals, rows = pf.read_stats()
    if totals is not None:
        np.testing.assert_array_equal(totals, stats.astype(np.uint64).sum(axis=0).astype(U32), err_msg=f"{what}: out_stats")
    if rows is not None:
        np.testing.assert_array_equal(rows, stats, err_msg=f"{what}: out_instance_stats")
    return stats, [e[3] for e in exp], small_changed


def spawns_of(cap, n):
    """a burst per instance, every count different where the capacity allows: the whole capacity, then less and less"""
    return [max(1, cap - k * (cap // 6) - (k > 0)) for k in range(n)]


# ---- capacities x instance counts x modes, all alive and after a die-off ------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_capacities_with_1_2_and_5_instances_all_alive_and_after_a_die_off(cap):
    for n in (1, 2, 5):
        ctx, prog, fxs = pes.make(cap, n, asset=trails_vec4(cap))
        spawns = spawns_of(cap, n)
        pes.step(ctx, fxs, 0, spawns)
        assert program_sample_plan(TRILINEAR, n, cap, 4, 0)[1:3] == (-(-cap // TILE), n)
        for state in ("all alive", "after a die-off"):
            if state == "after a die-off":
                for k, fx in enumerate(fxs):
                    fx.write_attr(A.VELOCITY.id, np.zeros((cap, 3), F32))
                    fx.write_attr(A.LIFETIME.id, np.random.default_rng(cap + k).uniform(0.8, 1.2, cap).astype(F32))       # (the calls above added to it)
                for f in range(1, 5):                                      # lifetimes are 0.8 .. 1.2 s: a second later part of every burst is gone
                    pes.step(ctx, fxs, f, [0] * n, dt=0.25)
            for mode in MODES:
                for k, fx in enumerate(fxs):
                    plant(fx, 2 + 1000 * cap + 10 * k + mode, DIMS)                  # (+ 2: the one particle of capacity 1 is inside in both modes)
                pf = fields_for(DIMS, 4, n, cap + 7 * mode + 100 * n)
                stats, _, small = check_program_sample(ctx, prog, fxs, pf, CH4, mode, -0.25, f"capacity {cap}, {n} instances, {state}, mode {mode}")
                counts = [fx.alive_count() for fx in fxs]
                assert list(stats[:, 0]) == counts
                if state == "all alive":
                    assert counts == spawns and counts[0] == cap
                    assert cap >= MIN_GUARDED or small > 0, "a small case samples and changes at least one particle"
                elif cap >= 255:
                    assert all(0 < c < s for c, s in zip(counts, spawns)), (counts, spawns)
                if cap >= 255 and n > 1:
                    assert len(set(counts)) == n, counts                  # the alive counts differ per instance
        for fx in fxs:
            fx.write_attr(A.LIFETIME.id, np.full(cap, 5.0, F32))           # (the calls added to the lifetimes: age < lifetime is the verifier's, not the call's)
            assert fx.check()["ok"] == 1                                   # lists, alive bytes and counters are as the frames left them
        ctx.close()


# ---- nothing alive ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [300, 4097])
def test_one_instance_of_five_with_nothing_alive_and_a_whole_program_with_nothing_alive(cap):
    n = 5
    ctx, prog, fxs = pes.make(cap, n, asset=trails_vec4(cap))
    before_any = fields_for(DIMS, 4, n, 1)
    prog.sample_all(channels=CH4, mode=TRILINEAR, **before_any.args())    # before the first frame: nothing is alive anywhere
    spawns = [cap, cap // 2, 0, 37, cap - 1]
    pes.step(ctx, fxs, 0, spawns)
    pes.step(ctx, fxs, 1, [0] * n, dt=1 / 60)
    for k, fx in enumerate(fxs):
        plant(fx, 50 + k, DIMS)                                            # the empty instance's planes hold values too: every bit of them is kept
    for mode in MODES:
        stats, infos, _ = check_program_sample(ctx, prog, fxs, fields_for(DIMS, 4, n, 3 + mode), CH4, mode, 1.0, f"capacity {cap}, one empty instance, mode {mode}")
        assert list(stats[2]) == [0, 0, 0, 0] and not infos[2]["alive"].any() and list(stats[:, 0]) == spawns
    for fx in fxs:
        fx.write_attr(A.LIFETIME.id, np.full(cap, 1.0, F32))               # (the calls above added to the lifetimes)
    for f in range(2, 6):
        pes.step(ctx, fxs, f, [0] * n, dt=0.5)                             # every lifetime is over
    ctx.synchronize()
    before = [planes(fx, ATTRS4) for fx in fxs]
    after_all = [fields_for(DIMS, 4, n, 9 + mode) for mode in MODES]
    for mode in MODES:
        prog.sample_all(channels=CH4, mode=mode, **after_all[mode].args())
    ctx.synchronize()
    for fx, b in zip(fxs, before):
        assert fx.alive_count() == 0
        for a, p in planes(fx, ATTRS4).items():
            np.testing.assert_array_equal(p, b[a])
    for pf in [before_any] + after_all:
        totals, rows = pf.read_stats()
        assert not totals.any() and not rows.any()                         # cleared, and nothing added
    ctx.close()


# ---- many small instances -------------------------------------------------------------------------------------------------------------------------------
def test_300_instances_of_capacity_64_in_one_call():
    cap, n = 64, 300
    ctx, prog, fxs = pes.make(cap, n, asset=trails_vec4(cap))
    rng = np.random.default_rng(64)
    spawns = rng.integers(0, cap + 1, n)
    spawns[:3] = (cap, 0, 1)
    pes.step(ctx, fxs, 0, spawns)
    for k, fx in enumerate(fxs):
        plant(fx, 7000 + k, DIMS)
    for mode in MODES:
        pf = fields_for(DIMS, 2, n, 300 + mode, stride=124)                # 120 words of field, a row of NaNs behind each
        ch = [(A.VELOCITY.id, 2, ADD), (A.F32X4_0.id, 1, SET)]
        stats, infos, small = check_program_sample(ctx, prog, fxs, pf, ch, mode, 0.5, f"300 x 64, mode {mode}")
        assert list(stats[:, 0]) == list(spawns) and small > n and 0 < stats[:, 2].sum() < stats[:, 1].sum()
        # over the whole program the guard conditions hold, as they cannot for 64 particles at a time
        alive = sum(int(i["alive"].sum()) for i in infos)
        assert 4 * sum(int(i["clamped"].sum()) for i in infos) >= alive and 2 * small > int(stats[:, 1].sum())
    ctx.close()


# ---- fields: shared, exact stride, padded stride; one to four channels ----------------------------------------------------------------------------------
def test_shared_field_exact_stride_and_padded_stride_with_one_to_four_channels():
    cap, n = 4097, 3
    ctx, prog, fxs = pes.make(cap, n, asset=trails_vec4(cap))
    pes.step(ctx, fxs, 0, [cap, cap - 1000, 2500])
    pes.step(ctx, fxs, 1, [0] * n, dt=1 / 60)
    fxs[1].set_simulated(False)                                            # frozen instances accept the call
    pes.step(ctx, fxs, 2, [0] * n, dt=1 / 60)
    # a component of a 3-vector, the last of a 4-vector, a scalar, POSITION itself; SET and ADD mixed
    dests = [(A.VELOCITY.id, 1, ADD), (A.F32X4_0.id, 3, SET), (A.LIFETIME.id, 0, ADD), (A.POSITION.id, 2, SET)]
    n_cells = DIMS[0] * DIMS[1] * DIMS[2]
    for k in range(1, 5):
        for mode in MODES:
            for what, stride in (("shared", 0), ("exact", n_cells * k), ("padded", n_cells * k + 8 * k)):      # (60 k is a multiple of 4 for every k)
                for i, fx in enumerate(fxs):
                    plant(fx, 100 * k + 10 * i + mode, DIMS)
                pf = fields_for(DIMS, k, n, 40 * k + mode, stride=stride)
                check_program_sample(ctx, prog, fxs, pf, dests[:k], mode, 1.0, f"{k} channels, mode {mode}, {what} stride")
    ctx.close()


# ---- stats: totals alone, rows alone, both, neither; rows are what hnb_effect_sample reports on a twin ------------------------------------------------
def make_pair(cap, n, spawns, frames=1, asset=None, **options):
    """two programs from the same blob in contexts of their own, stepped with the same seeds -> [(ctx, prog, fxs)] * 2"""
    pair = [pes.make(cap, n, asset=asset if asset is not None else trails_vec4(cap), **options) for _ in range(2)]
    for f in range(frames):
        for ctx, _, fxs in pair:
            pes.step(ctx, fxs, f, spawns if f == 0 else [0] * n, dt=1 / 600 if f == 0 else 1 / 30)
    return pair


def plant_pair(pair, seed, dims=DIMS):
    for _, _, fxs in pair:
        for k, fx in enumerate(fxs):
            plant(fx, seed + k, dims)


def sample_twin(tfxs, pf, channels, mode, scale, stats=None):
    """the effect form per instance, instance i from its own field; stats: a guarded [n, 4] tensor that takes instance i's four numbers, or None"""
    for i, fx in enumerate(tfxs):
        fx.sample(pf.dims, pf.origin, pf.inv_cell, pf.field_ptr_of(i), channels, mode, scale, stats.data_ptr() + 4 * GUARD + 16 * i if stats is not None else None)


def assert_pairs_equal(pair, what):
    for ctx, _, _ in pair:
        ctx.synchronize()
    for i, (a, b) in enumerate(zip(pair[0][2], pair[1][2])):
        d = a.compare(b)
        assert d["equal"] == 1, (what, f"instance {i}", d)


def test_stats_totals_alone_rows_alone_both_and_neither_against_a_twin():
    cap, n = 4097, 4
    pair = make_pair(cap, n, [cap, 3000, 0, 777])
    (ctx, prog, fxs), (tctx, _, tfxs) = pair
    for r, (totals, rows) in enumerate(((True, False), (False, True), (True, True), (False, False))):
        mode = MODES[r % 2]
        plant_pair(pair, 20 * r)
        pf = fields_for(DIMS, 4, n, r, totals=totals, rows=rows)
        twin_stats = guarded(4 * n)                                       # (the effect form clears its own four words, the empty instance's too)
        torch.cuda.synchronize()
        sample_twin(tfxs, pf, CH4, mode, 2.0, twin_stats)
        tctx.synchronize()
        stats, _, _ = check_program_sample(ctx, prog, fxs, pf, CH4, mode, 2.0, f"totals {totals}, rows {rows}")
        want = twin_stats.cpu().numpy().view(U32)[GUARD: GUARD + 4 * n].reshape(n, 4)
        np.testing.assert_array_equal(stats, want)                         # the restatement's rows are the effect form's ...
        got_totals, got_rows = pf.read_stats()
        if rows:
            np.testing.assert_array_equal(got_rows, want)                  # ... and so are the call's
        if totals:
            np.testing.assert_array_equal(got_totals, want.astype(np.uint64).sum(axis=0).astype(U32))
        assert_pairs_equal(pair, f"stats round {r}")
    ctx.close(); tctx.close()


# ---- equivalence with a twin sampled per instance by the effect form ----------------------------------------------------------------------------------
def run_frames(pair, f, k, steps):
    """k frames on both programs from frame f on: one by one, or as one hnb_simulate_steps call -> the next frame"""
    dt = 1 / 30
    for ctx, prog, fxs in pair:
        n = len(fxs)
        if steps:
            prog.set_frames_ahead(np.zeros((k, n), U32), np.array([[frame_seed((f + j) * 16 + i) for i in range(n)] for j in range(k)], np.uint64).astype(U32))
            ctx.simulate_steps([(dt, (f + j) * dt) for j in range(k)])
        else:
            for j in range(k):
                pes.step(ctx, fxs, f + j, [0] * n, dt=dt)
    return f + k


@pytest.mark.parametrize("mode", MODES, ids=["nearest", "trilinear"])
def test_a_twin_sampled_per_instance_by_the_effect_form_is_equal_after_the_call_after_frames_and_after_steps(mode):
    cap, n = 8193, 5
    pair = make_pair(cap, n, [cap, 5000, 0, 4097, 100], frames=3)
    (ctx, prog, fxs), (tctx, _, tfxs) = pair
    fxs[3].set_simulated(False); tfxs[3].set_simulated(False)
    plant_pair(pair, 300 + mode)
    assert_pairs_equal(pair, "planted")
    pf = fields_for(DIMS, 3, n, 5 + mode, stride=DIMS[0] * DIMS[1] * DIMS[2] * 3 + 4)
    ch = [(A.VELOCITY.id, 0, ADD), (A.VELOCITY.id, 2, ADD), (A.LIFETIME.id, 0, SET)]      # lifetimes from the field: N(0, 3) - particles die by it in the frames below
    prog.sample_all(channels=ch, mode=mode, scale=0.5, **pf.args())       # no synchronisation in front or behind
    sample_twin(tfxs, pf, ch, mode, 0.5)
    assert_pairs_equal(pair, "after the call")
    f = run_frames(pair, 3, 3, steps=False)
    assert_pairs_equal(pair, "3 frames later")
    f = run_frames(pair, f, 4, steps=True)
    assert_pairs_equal(pair, "after hnb_simulate_steps of 4")
    counts = [fx.alive_count() for fx in fxs]
    assert 0 < counts[0] < cap and counts[2] == 0 and counts[3] == 4097, counts      # particles died by the sampled lifetimes; the frozen instance kept its own
    pf.read_stats()
    ctx.close(); tctx.close()


# ---- the reset: later frames compute what they would after hnb_effect_write_attr ---------------------------------------------------------------------
@pytest.mark.parametrize("horizons", [True, False], ids=["death horizons", "lifetime culling alone"])
def test_later_frames_of_instance_2_of_3_compute_what_they_would_after_write_attr(horizons):
    """The LIFETIME scenario of tests/test_gpu_sample.py on instance 2 of 3: 70,000 slots, frames publish the chunks' lifetime bounds (and death
    horizons), the call then stores lifetimes below those bounds into every instance, so particles die from the next frame on. The twin program gets
    the same planes through hnb_effect_write_attr. A frame later the alive counts must be equal - they are not when the call leaves an instance's
    cached bounds standing - and 7 more frames, 4 of them through hnb_simulate_steps, must leave every pair equal.
    Which program is which: horizon_eligible is what hnb_program_kernel_info reports as "death horizons in use", and it requires lifetime culling
    (hnb_program.h: update_streams && cull_lifetime && !kills && !ribbons && !slot_order && the HNB_OPT_HORIZON option). The first case asserts that
    line for the default options; the second sets only HNB_OPT_HORIZON to 0 on the same asset, which removes that one term: the line is gone,
    lifetime culling stays, and the reset kernel clears the lifetime bounds alone.
    Observed once by hand with the reset launch taken out of run_program_sample, and once with its grid limited to instance 0: see DESIGN.md
    "Sample, program form"."""
    cap, n = 70_000, 3
    pair = make_pair(cap, n, [cap] * n, frames=6, asset=effects.firework_trails(cap), age_cohort=3, horizon=1 if horizons else 0)
    (ca, pa, fa), (cb, pb, fb) = pair
    assert ("death horizons in use" in pa.kernel_info()) == horizons
    rng = np.random.default_rng(4)
    n_cells = DIMS[0] * DIMS[1] * DIMS[2]
    values = [rng.uniform(0.31, 0.9, (n_cells, 1)).astype(F32) for _ in range(n)]      # from 0.31 s: below the bound of 0.8 s every chunk published
    for v in values:
        v[::7] = F32(0.05)                                                 # ... and some cells kill at once: age >= lifetime in the next update
    ca.synchronize()
    pos = fa[2].read_attr(A.POSITION.id).reshape(-1, 3)
    lo, hi = pos.min(axis=0), pos.max(axis=0)                              # the burst's box, a little narrower: some particles are outside
    pf = ProgField(DIMS, values, n, 64, origin=lo + 0.02 * (hi - lo), inv_cell=np.asarray(DIMS) / (0.96 * (hi - lo)))
    pa.sample_all(channels=[(A.LIFETIME.id, 0, SET)], mode=TRILINEAR, **pf.args())      # no synchronisation in front or behind
    for a, b in zip(fa, fb):
        b.write_attr(int(A.LIFETIME.id), a.read_attr(int(A.LIFETIME.id)))  # (the read-back waits for the call)
    _, rows = pf.read_stats()
    assert (rows[:, 0] == cap).all() and (0 < rows[:, 2]).all() and (rows[:, 2] < rows[:, 1]).all()
    f = run_frames(pair, 6, 1, steps=False)
    alive = [fx.alive_count() for fx in fa]                                # the cells of 0.05 s killed their particles in this frame, the others live on
    print("alive a frame later:", alive, "twin:", [fx.alive_count() for fx in fb])
    assert alive == [fx.alive_count() for fx in fb] and all(0 < c < cap for c in alive), (alive, [fx.alive_count() for fx in fb])
    assert_pairs_equal(pair, "a frame later")
    f = run_frames(pair, f, 3, steps=False)
    f = run_frames(pair, f, 4, steps=True)
    assert_pairs_equal(pair, "8 frames later")
    assert all(fx.alive_count() < c for fx, c in zip(fa, alive)) and all(fx.check()["ok"] == 1 for fx in fa)      # particles died on the way, in both
    ca.close(); cb.close()


# ---- the loop the call closes: program deposit -> a torch op on the grid -> program sample -------------------------------------------------------------
def test_five_rounds_of_program_deposit_torch_and_program_sample_with_a_splat_and_a_bounds_call_interleaved():
    cap, n, dims = 5000, 3, (8, 8, 8)
    n_cells = 512
    pair = make_pair(cap, n, [cap, 3000, 1234], frames=1)
    (ctx, prog, fxs), (tctx, tprog, tfxs) = pair
    b = dict(origin=np.full(3, -3.0, F32), inv_cell=np.full(3, 8 / 6.0, F32))       # [-3, 3)^3: part of the bursts leaves it
    ch = [(A.VELOCITY.id, 0, ADD), (A.F32X4_0.id, 2, SET)]
    keep = []                                                              # (destinations stay allocated until the streams have run the calls)
    changed = 0
    for r in range(5):
        f = run_frames(pair, 1 + r, 1, steps=False)
        grids = []
        for c, p in ((ctx, prog), (tctx, tprog)):
            count = torch.zeros(n_cells + 1, dtype=torch.int32, device="cuda")
            sums = torch.zeros((n_cells + 1, 2), dtype=torch.int64, device="cuda")
            splat_count, splat_sums = torch.zeros_like(count), torch.zeros_like(sums)
            bounds = torch.zeros((n + 1) * 16, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            p.deposit(dims, b["origin"], b["inv_cell"], count.data_ptr(), [(A.VELOCITY.id, 0, 12), (A.VELOCITY.id, 1, 12)], sums.data_ptr())
            p.splat(dims, b["origin"], b["inv_cell"], splat_count.data_ptr(), [(A.VELOCITY.id, 0, 12), (A.VELOCITY.id, 1, 12)], splat_sums.data_ptr())
            p.bounds(A.POSITION.id, bounds.data_ptr(), n + 1)
            c.synchronize()                                                # the torch op runs on torch's stream
            g = sums[:n_cells].to(torch.float32) * (2.0 ** -12 * -0.01)    # a drag towards the cell's mean velocity, per instance a little stronger
            g = torch.stack([g * (1.0 + 0.25 * i) for i in range(n)]).contiguous()
            torch.cuda.synchronize()
            grids.append(g)
            keep.append((count, sums, splat_count, splat_sums, bounds, g))
        assert torch.equal(grids[0], grids[1])                             # both programs deposited the same particles
        mode = MODES[r % 2]
        pf = ProgField(dims, list(grids[0].cpu().numpy()), n, n_cells * 2, **b)
        exp = [expected(fx, pf.of(i), ch, mode, 0.5, ATTRS4) for i, fx in enumerate(fxs)]
        a = pf.args(); a["field_ptr"] = grids[0].data_ptr(); a["field_instance_stride"] = n_cells * 2      # the torch tensor itself
        prog.sample_all(channels=ch, mode=mode, scale=0.5, **a)
        for i, fx in enumerate(tfxs):
            fx.sample(dims, b["origin"], b["inv_cell"], grids[1].data_ptr() + 4 * i * n_cells * 2, ch, mode, 0.5)
        ctx.synchronize()
        for i, (fx, (_, want, stats, info)) in enumerate(zip(fxs, exp)):
            assert_planes(fx, want, info, f"round {r}, mode {mode}, instance {i}")
            changed += int((info["changed"] & info["wr"]).sum())
        totals, rows = pf.read_stats()
        np.testing.assert_array_equal(rows, np.array([e[2] for e in exp], U32))
        assert_pairs_equal(pair, f"round {r}")
    assert changed > cap and rows[:, 2].sum() > 0 and all(fx.check()["ok"] == 1 for fx in fxs)
    ctx.close(); tctx.close()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    """Every refusal of the contract but a layout without POSITION and more than 65,535 instances, which the stand-alone program of
    tests/test_sample_program_abi.py holds"""
    cap, n, dims = 5000, 2, (4, 4, 4)
    ctx, prog, fxs = pes.make(cap, n, asset=trails_vec4(cap))
    pes.step(ctx, fxs, 0, [cap, 100])
    empty_prog = ctx.create_program(bh.lower(trails_vec4(300)))            # a program of 0 instances
    for k, fx in enumerate(fxs):
        plant(fx, 1 + k, dims)
    lib = runtime.load_library()
    pf = fields_for(dims, 2, n, 1)
    ch = [(A.VELOCITY.id, 1, ADD), (A.LIFETIME.id, 0, SET)]
    good = lambda: runtime.program_sample_desc(channels=ch, mode=TRILINEAR, scale=1.0, **pf.args())
    nan, inf = float("nan"), float("inf")
    ctx.synchronize()
    before = [planes(fx, ATTRS4) for fx in fxs]

    def refused(desc, text, target=prog):
        assert lib.hnb_program_sample(target._h, C.byref(desc)) == -1, text
        assert text.encode() in lib.hnb_last_error(), (text, lib.hnb_last_error())

    assert lib.hnb_program_sample(None, C.byref(good())) == -1 and b"NULL" in lib.hnb_last_error()
    assert lib.hnb_program_sample(prog._h, None) == -1 and b"NULL" in lib.hnb_last_error()
    # the outer description
    x = good(); x.struct_size = 136
    refused(x, "HnbProgramSampleDesc::struct_size")
    x = good(); x.flags = 1
    refused(x, "flags: 0")
    x = good(); x.reserved = 1
    refused(x, "reserved is not 0")
    for stride in (2, 64, 126, 130):                                       # 4 x 4 x 4 x 2 = 128 words
        x = good(); x.field_instance_stride = stride
        refused(x, "field_instance_stride: 0, or a multiple of 4")
    x = good(); x.out_instance_stats = pf.rows.data_ptr() + 4 * GUARD + 8
    refused(x, "out_instance_stats: NULL or")
    refused(good(), "the program has 0 instances", target=empty_prog)
    # the inner description: hnb_effect_sample's refusals, with its text
    x = good(); x.sample.struct_size = 132
    refused(x, "HnbSampleDesc::struct_size")
    x = good(); x.sample.flags = 1
    refused(x, "flags: 0")
    x = good(); x.sample.mode = 2
    refused(x, "mode: HNB_SAMPLE_NEAREST or")
    for d in ((0, 4, 4), (4096, 4096, 2)):
        x = good(); x.sample.dims = (C.c_uint32 * 3)(*d)
        refused(x, "HNB_BIN_MAX_CELLS")
    x = good(); x.sample.origin[1] = nan
    refused(x, "origin is not finite")
    for bad in (0.0, -1.0, inf, nan):
        x = good(); x.sample.inv_cell[2] = bad
        refused(x, "inv_cell is not finite and above 0")
    for k in (0, 5):
        x = good(); x.sample.n_channels = k
        refused(x, "n_channels is not 1..")
    for attr in (A.AGE.id, A.COLOR.id, A.SIZE3.id, A.ID.id, 9999):         # AGE; not in this layout (COLOR, SIZE3); not stored; no attribute
        x = good(); x.sample.channels[1].attr = attr
        refused(x, "channels[1]")
        assert b"not an f32 attribute" in lib.hnb_last_error()
    x = good(); x.sample.channels[0].comp = 3
    refused(x, "comp is at or past")
    x = good(); x.sample.channels[1].op = 2
    refused(x, "op: HNB_SAMPLE_SET or")
    x = good(); x.sample.channels[1].reserved = 1
    refused(x, "reserved is not 0")
    x = good(); x.sample.channels[1] = runtime.SampleChannel(int(A.VELOCITY.id), 1, SET, 0)
    refused(x, "an earlier channel's")
    x = good(); x.sample.channels[3].op = 1
    refused(x, "at or past n_channels")
    for bad in (nan, inf, -inf):
        x = good(); x.sample.scale = bad
        refused(x, "scale is not finite")
    x = good(); x.sample.field = None
    refused(x, "field: a 16-byte aligned")
    x = good(); x.sample.field = pf.buf.data_ptr() + 4 * GUARD + 8
    refused(x, "field: a 16-byte aligned")
    x = good(); x.sample.out_stats = pf.totals.data_ptr() + 4
    refused(x, "out_stats: NULL or")
    ctx.synchronize()
    assert pf.untouched()
    for fx, b in zip(fxs, before):
        for a, p in planes(fx, ATTRS4).items():
            np.testing.assert_array_equal(p, b[a])
    check_program_sample(ctx, prog, fxs, pf, ch, TRILINEAR, 1.0, "a good call behind the refusals")        # ... and the same destinations take a good call
    ctx.close()
