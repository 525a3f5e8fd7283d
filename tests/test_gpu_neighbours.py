"""hnb_effect_neighbours on the GPU (include/hanabi_amd_neighbours.h): for every alive particle inside a uniform grid, up to four fixed-point sums over
the particles within a radius and within one cell of it, stored or added into components of f32 attributes. The expectation is always the brute-force
numpy restatement (tests/test_neighbours_abi.py np_neighbours / np_store) over the host's read-back of the planes and the alive list, compared bit for
bit over WHOLE planes (dead slots, outside and crowded particles and unnamed components included). There is no tolerance anywhere. The stats sit
between guard words filled with a sentinel. Before comparing, each main case asserts on the restatement alone what makes the case worth running."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, frame_seed
from test_bounds_abi import trails_vec4
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, _device_meta, step
from test_gpu_export_binned import Grid, grid_around, run_binned
from test_gpu_import import make, planes, run_stretch
from test_neighbours_abi import ADD, DIFF, ONE, SET, W_ONE, W_U1, W_U2, W_U3, np_neighbours, np_store, one_source

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
GUARD = 4
ATTRS4 = [A.POSITION.id, A.VELOCITY.id, A.AGE.id, A.LIFETIME.id, A.F32X4_0.id]          # trails_vec4's layout, every plane of it
# a count, a density and a DIFF channel on POSITION.x
CH3 = [(ONE, 0, 0, 0, A.F32X4_0.id, 0, SET), (ONE, 0, 0, 30, A.F32X4_0.id, 1, SET), (A.POSITION.id, 0, DIFF, 16, A.VELOCITY.id, 1, ADD)]
OFFSETS26 = set(itertools.product((-1, 0, 1), repeat=3)) - {(0, 0, 0)}


class Stats:
    def __init__(self):
        self.buf = torch.full((8 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                 # (the fill runs on torch's stream, the call on the simulation's)

    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def read(self):
        raw = self.buf.cpu().numpy().view(U32)
        assert (raw[:GUARD] == U32(SENTINEL & 0xFFFFFFFF)).all() and (raw[GUARD + 8:] == U32(SENTINEL & 0xFFFFFFFF)).all(), "words next to out_stats were written"
        return raw[GUARD: GUARD + 8]

    def untouched(self):
        return bool((self.buf.cpu().numpy().view(U32) == U32(SENTINEL & 0xFFFFFFFF)).all())


def radius_of(grid, part=0.999):
    """the largest radius the coverage rule takes on this grid, times `part`"""
    r = F32(part / float(grid.inv_cell.max()))
    assert all(float(r) * float(i) <= 1.0 for i in grid.inv_cell)
    return float(r)


def expected(fx, grid, radius, weight, channels, limit, scale, attrs=ATTRS4):
    """The restatement over the host's read-back of the effect as it is (synchronises). -> (before, want: attribute -> [capacity, ncomp] words;
    stats [8]; ref: np_neighbours' result, with `alive`)"""
    before = planes(fx, attrs)
    alive = fx.alive_list()
    pos = before[int(A.POSITION.id)].view(F32)
    src = [one_source(fx.capacity) if ch[0] == ONE else before[int(ch[0])][:, ch[1]].copy() for ch in channels]
    ref = np_neighbours(pos, alive, src, (grid.dims, grid.origin, grid.inv_cell), radius, weight, channels, limit)
    g = ref["gathered"]
    want = {a: p.copy() for a, p in before.items()}
    for k, ch in enumerate(channels):
        out = np_store(ch[6], before[int(ch[4])][:, ch[5]].view(F32), ref["S"][:, k], ch[3], scale)
        want[int(ch[4])][g, ch[5]] = out.view(U32)[g]
    ref["alive"] = alive
    stats = np.array([len(alive), g.sum(), len(alive) - ref["inside"].sum(), ref["crowded"].sum(), ref["rejected"], 0, 0, 0], np.uint64).astype(U32)
    return before, want, stats, ref


def assert_planes(fx, want, ref, what):
    got = planes(fx, list(want))
    for a, w in want.items():
        ok = (got[a] == w) | (np.isnan(w.view(F32)) & np.isnan(got[a].view(F32)))
        bad = np.argwhere(~ok)
        assert not len(bad), (what, f"attribute {a}", len(bad), [(int(s), int(c), hex(int(got[a][s, c])), hex(int(w[s, c])), bool(ref["gathered"][s]), int(ref["nnb"][s])) for s, c in bad[:6]])


def check(ctx, fx, grid, radius, what, channels=CH3, weight=W_U3, limit=4096, scale=1.0, attrs=ATTRS4, conditions=None):
    """one call against the restatement: whole planes, stats, guard words -> (want, stats, ref)"""
    before, want, stats, ref = expected(fx, grid, radius, weight, channels, limit, scale, attrs)
    if conditions:
        conditions(ref)
    st = Stats()
    fx.neighbours(grid.dims, grid.origin, grid.inv_cell, radius, channels, weight, limit, scale, st.ptr())
    ctx.synchronize()
    assert_planes(fx, want, ref, what)
    np.testing.assert_array_equal(st.read(), stats, err_msg=f"{what}: out_stats")
    return want, stats, ref


# ---- capacities: the one-workgroup sort and the multi-tile one, a partial last tile; the burst state ------------------------------------------------
DIMS = {1: (3, 3, 3), 3: (3, 3, 3), 300: (4, 4, 4), 4096: (7, 7, 7), 4097: (7, 7, 7), 10_000: (9, 9, 9)}


@pytest.mark.parametrize("cap", [1, 3, 300, 4096, 4097, 10_000])
def test_capacities_on_the_burst_state(cap):
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    grid = grid_around(fx, DIMS[cap])
    radius = radius_of(grid)

    def conditions(ref):
        g = ref["gathered"]
        assert not ref["crowded"].any() and g.sum() == cap, "no particle is crowded or outside"
        if cap >= 300:
            assert 2 * int((ref["nnb"][g] >= 3).sum()) >= int(g.sum()), "at least half the gathered particles have three neighbours or more"
            assert OFFSETS26 <= ref["offsets"], ("a neighbour pair for every one of the 26 cell offsets", OFFSETS26 - ref["offsets"])

    want, stats, ref = check(ctx, fx, grid, radius, f"capacity {cap}", conditions=conditions)
    if cap == 1:                                                           # the empty neighbourhood: S = 0, and the formula is followed
        assert ref["nnb"].tolist() == [0] and want[int(A.F32X4_0.id)][0, :2].tolist() == [0, 0] and list(stats[:5]) == [1, 1, 0, 0, 0]
    if cap == 3:                                                           # three particles 2 .. 3 units from the centre: the counts are what the distances say, 0 included
        assert set(want[int(A.F32X4_0.id)][:, 0].view(F32).tolist()) <= {0.0, 1.0, 2.0} and int(ref["nnb"].sum()) % 2 == 0
    for weight in (W_ONE, W_U1, W_U2):                                     # the other weights on the same state (the planes as the call above left them)
        check(ctx, fx, grid, radius, f"capacity {cap}, weight {weight}", weight=weight, scale=-0.5)
    assert fx.check()["ok"] == 1
    ctx.close()


# ---- grid edges and the big grid ------------------------------------------------------------------------------------------------------------------
def test_a_grid_that_cuts_through_the_cloud_outside_sources_do_not_count():
    cap = 10_000
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    grid = grid_around(fx, (6, 6, 6), inner=0.6)
    radius = radius_of(grid)

    def conditions(ref):
        inside, alive = ref["inside"], ref["alive"]
        pos = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3).astype(np.float64)
        out = alive[~inside[alive]]
        assert len(out) > 0 and inside.sum() > 0, "there is an outside bin"
        ins = np.flatnonzero(inside)
        near = 0
        for o in out[:400]:                                                # outside particles within the radius of an inside one: they must not count
            near += int((((pos[ins] - pos[o]) ** 2).sum(axis=1) < 0.9 * radius * radius).sum())
        assert near > 0
        c = ref["cells"][ins]
        xyz = np.stack([c % 6, (c // 6) % 6, c // 36], axis=1)
        on_edge = ((xyz == 0) | (xyz == 5)).sum(axis=1)
        assert {1, 2, 3} <= set(on_edge.tolist()), "queries in face, edge and corner cells of the grid"

    check(ctx, fx, grid, radius, "inner 0.6", conditions=conditions)
    ctx.close()


def test_more_than_65536_cells_runs_the_upper_sort_digits():
    cap = 10_000
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    grid = grid_around(fx, (41, 41, 41))
    want, stats, ref = check(ctx, fx, grid, radius_of(grid), "41 x 41 x 41", weight=W_U2)
    assert ref["cells"][ref["alive"]].max() >= 65536 and stats[1] == cap and ref["nnb"].sum() > 0
    ctx.close()


def test_one_cell_that_holds_everything_all_pairs():
    cap = 300
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    grid = Grid((1, 1, 1), (-8, -8, -8), (1 / 16, 1 / 16, 1 / 16))
    want, stats, ref = check(ctx, fx, grid, 16.0, "1 x 1 x 1", limit=cap)
    assert (ref["nnb"] == cap - 1).all() and (want[int(A.F32X4_0.id)][:, 0].view(F32) == cap - 1).all()
    want, stats, ref = check(ctx, fx, grid, 16.0, "1 x 1 x 1, one below the count", limit=cap - 1)     # ... and with the limit one below: everything is crowded
    assert list(stats[:5]) == [cap, 0, 0, cap, 0]
    ctx.close()


# ---- crowding -------------------------------------------------------------------------------------------------------------------------------------
def test_crowded_queries_keep_every_bit_and_remain_sources():
    cap = 300
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    rng = np.random.default_rng(2)
    pos = np.empty((cap, 3), F32)
    pos[:200] = (1.5 + rng.uniform(-0.3, 0.3, (200, 3))).astype(F32)                       # 200 in cell (1, 1, 1) of a 5 x 4 x 4 grid of unit cells
    pos[200:220] = (np.array([2.1, 1.5, 1.5]) + rng.uniform(0, 0.3, (20, 3)) * (1, 1, 1)).astype(F32)       # 20 next to it, in (2, 1, 1): crowded as well
    pos[220:240] = (np.array([3.05, 1.5, 1.5]) + rng.uniform(0, 0.25, (20, 3))).astype(F32)                # 20 in (3, 1, 1): they see 40 candidates
    pos[240:] = (np.array([1.5, 3.5, 3.5]) + rng.uniform(-0.4, 0.4, (60, 3))).astype(F32)                   # and 60 far away
    fx.write_attr(A.POSITION.id, pos)
    grid = Grid((5, 4, 4), (0, 0, 0), (1, 1, 1))

    def conditions(ref):
        g, cr = ref["gathered"], ref["crowded"]
        assert cr.sum() == 220 and g.sum() == 80 and cr[:220].all()
        assert (ref["crowded_nb"][220:240] > 0).any(), "a gathered particle has crowded neighbours, which still contribute"

    want, stats, ref = check(ctx, fx, grid, 1.0, "crowding", limit=128, conditions=conditions)
    assert stats[3] == 220
    ctx.close()


# ---- non-finite and signed-zero positions; rejected contributions -----------------------------------------------------------------------------------
def test_non_finite_positions_land_outside_and_rejected_contributions_are_counted():
    cap = 4097
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    ctx.synchronize()
    pos = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3).copy()
    nan, inf = F32(np.nan), F32(np.inf)
    special = [(nan, 0.5, 0.5), (0.5, -nan, 0.5), (inf, 0.5, 0.5), (0.5, 0.5, -inf), (-0.0, -0.0, -0.0), (0.0, 0.0, 0.0), (-0.0, 0.5, 1.0)]
    rows = np.arange(7, 7 + 500 * len(special), 500)
    pos[rows] = np.array(special, F32)
    fx.write_attr(A.POSITION.id, pos)
    vel = fx.read_attr(A.VELOCITY.id).view(F32).reshape(-1, 3).copy()
    vel[::5, 2] = nan; vel[1::7, 2] = inf; vel[2::11, 2] = F32(1e30); vel[3::13, 2] = F32(1e-41)
    fx.write_attr(A.VELOCITY.id, vel)
    grid = Grid((4, 4, 4), (0, 0, 0), (1, 1, 1))                           # the origin at 0: -0 is inside; the cloud's negative half is outside
    ch = [(A.VELOCITY.id, 2, 0, 32, A.F32X4_0.id, 2, SET), (ONE, 0, 0, 0, A.F32X4_0.id, 0, SET), (A.VELOCITY.id, 0, DIFF, 8, A.LIFETIME.id, 0, ADD)]

    def conditions(ref):
        assert not ref["inside"][rows[:4]].any() and ref["inside"][rows[4:]].all(), "non-finite positions are outside, signed zeros inside"
        assert ref["rejected"] > 0 and ref["nnb"].sum() > ref["rejected"]

    want, stats, ref = check(ctx, fx, grid, 0.8, "special positions, rejected contributions", channels=ch, weight=W_U1, conditions=conditions)
    assert stats[4] == ref["rejected"] % (1 << 32) and 0 < stats[2] < stats[0]
    ctx.close()


# ---- hazard freedom ---------------------------------------------------------------------------------------------------------------------------------
def test_destinations_that_are_sources_see_the_state_before_the_call():
    cap = 4097
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    grid = grid_around(fx, (7, 7, 7))
    radius = radius_of(grid)
    check(ctx, fx, grid, radius, "POSITION.x into itself", channels=[(A.POSITION.id, 0, DIFF, 20, A.POSITION.id, 0, ADD)], weight=W_U2, scale=0.01)
    grid = grid_around(fx, (7, 7, 7))
    ch = [(A.VELOCITY.id, 0, 0, 10, A.VELOCITY.id, 1, SET), (A.VELOCITY.id, 1, DIFF, 10, A.POSITION.id, 2, ADD), (A.POSITION.id, 2, 0, 10, A.VELOCITY.id, 0, SET)]
    want, stats, ref = check(ctx, fx, grid, radius_of(grid), "a destination is another channel's source", channels=ch, weight=W_U1, scale=0.001)
    assert ref["nnb"].sum() > cap
    ctx.close()


# ---- list shapes ------------------------------------------------------------------------------------------------------------------------------------
def test_after_a_die_off_and_on_a_churn_list():
    cap = 10_000
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    for f in range(1, 5):
        step(ctx, fx, f, 0, dt=0.25)
    alive = fx.alive_list()
    assert 0 < len(alive) < cap and not np.array_equal(alive, np.arange(len(alive)))
    grid = grid_around(fx, (5, 5, 5), inner=0.9)                           # a second later the shell is 40 .. 60 units wide: sparse, and some of it outside
    want, stats, ref = check(ctx, fx, grid, radius_of(grid), "die-off")
    assert stats[0] == len(alive) and stats[2] > 0 and ref["nnb"].sum() > 0
    assert fx.check()["ok"] == 1
    ctx.close()
    cap = 8000
    ctx, fx = make(cap, effects.firework_trails(cap, spawner=bh.SpawnerSettings.rate(3000.0)))
    rng = np.random.default_rng(5)
    for f in range(40):
        step(ctx, fx, f, int(rng.integers(100, 600)), dt=1 / 20)
    alive = fx.alive_list()
    assert 256 < len(alive) < cap and not np.array_equal(alive, np.sort(alive))
    trail = [A.POSITION.id, A.VELOCITY.id, A.AGE.id, A.LIFETIME.id]
    grid = grid_around(fx, (4, 4, 4), inner=0.8)
    ch = [(ONE, 0, 0, 0, A.VELOCITY.id, 0, SET), (A.LIFETIME.id, 0, 0, 20, A.VELOCITY.id, 2, ADD)]
    want, stats, ref = check(ctx, fx, grid, radius_of(grid), "churn", channels=ch, weight=W_U1, attrs=trail, limit=8000)
    assert stats[1] > 0 and ref["nnb"].sum() > 0
    ctx.close()


def test_ring_list_is_read_through_its_head_and_left_alone():
    cap = 10_000
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
    fx.write_attr(A.POSITION.id, np.random.default_rng(3).uniform(-1, 1, (cap, 3)).astype(F32).view(np.uint32))     # (the ribbon's particles sit on one point: spread them)
    grid = grid_around(fx, (5, 4, 3), inner=0.8)
    ch = [(ONE, 0, 0, 0, A.SIZE.id, 0, SET)]
    want, stats, ref = check(ctx, fx, grid, radius_of(grid), "ring", channels=ch, weight=W_ONE, attrs=[A.POSITION.id, A.AGE.id, A.SIZE.id])
    assert stats[0] == m.alive_count and 0 < stats[2] < stats[0] and ref["nnb"].sum() > 0
    np.testing.assert_array_equal(fx.alive_list(), before)              # the list, and with it the ribbon's own sort order, is what it was
    m2 = _device_meta(fx)
    assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


# ---- stale AGE --------------------------------------------------------------------------------------------------------------------------------------
def test_stale_age_as_a_source_is_materialised_by_the_call():
    """LEAN cohorts: the AGE plane is stale until something materialises it. The test does not (a read-back of AGE would): it calls first and states the
    expectation from the read-back afterwards - AGE and POSITION are no destination, and a SET needs no earlier value."""
    cap = 10_000
    ctx, fx = make(cap, trails_vec4(cap), age_cohort=1)
    assert fx.device_view().stale_attr_mask == 1 << A.AGE.id
    for f in range(4):
        step(ctx, fx, f, 6000 if f == 0 else 1000, dt=1 / 60)
    grid = Grid((6, 6, 6), (-3, -3, -3), (1, 1, 1))
    ch = [(A.AGE.id, 0, 0, 24, A.F32X4_0.id, 3, SET), (A.AGE.id, 0, DIFF, 24, A.F32X4_0.id, 2, SET)]
    st = Stats()
    fx.neighbours(grid.dims, grid.origin, grid.inv_cell, 1.0, ch, W_U1, 8192, 1.0, st.ptr())
    ctx.synchronize()
    before, want, stats, ref = expected(fx, grid, 1.0, W_U1, ch, 8192, 1.0)
    ages = before[int(A.AGE.id)][ref["alive"], 0].view(F32)
    assert len(np.unique(ages)) == 4 and ref["nnb"].sum() > 0 and (ref["S"][:, 1] != 0).any()
    assert_planes(fx, want, ref, "stale AGE")                              # (idempotent here: the destinations hold what the call stored)
    np.testing.assert_array_equal(st.read(), stats)
    ctx.close()


# ---- the state after the call -----------------------------------------------------------------------------------------------------------------------
def test_later_frames_compute_what_they_would_after_write_attr():
    """Frames publish the chunks' lifetime bounds and death horizons; the call then stores lifetimes shorter than those bounds, so particles die from
    the next frames on. The twin gets the same planes through hnb_effect_write_attr. Both run 30 frames, 8 of them through hnb_simulate_steps; every
    plane, list and counter must agree - which they do not when the call leaves the cached bounds standing."""
    cap = 70_000
    asset = effects.firework_trails(cap)
    (ca, fa), (cb, fb) = [make(cap, age_cohort=3) for _ in range(2)]
    for f in range(6):
        for c, fx in ((ca, fa), (cb, fb)):
            step(c, fx, f, cap if f == 0 else 0, dt=1 / 30)
    grid = grid_around(fa, (12, 12, 12), inner=0.9)
    st = Stats()
    # lifetime = 0.3 s + 1 ms per neighbour (a few hundred of them): below the bound of 0.8 s every chunk published for all but the densest spots
    fa.write_attr(A.LIFETIME.id, np.full(cap, 0.3, F32)); fb.write_attr(A.LIFETIME.id, np.full(cap, 0.3, F32))
    for c, fx in ((ca, fa), (cb, fb)):
        step(c, fx, 6, 0, dt=1 / 300)                                      # (a frame behind the write: bounds and horizons are published again)
    ca.synchronize()
    lists = (fa.alive_list().copy(), fa.dead_list().copy(), fa.metadata())
    fa.neighbours(grid.dims, grid.origin, grid.inv_cell, radius_of(grid), [(ONE, 0, 0, 0, A.LIFETIME.id, 0, ADD)], W_ONE, 65536, 0.001, st.ptr())     # no synchronisation in front or behind
    fb.write_attr(A.LIFETIME.id, fa.read_attr(A.LIFETIME.id))              # (the read-back waits for the call)
    stats = st.read()
    assert stats[0] == cap and 0 < stats[2] < stats[1] and stats[3] == 0
    np.testing.assert_array_equal(fa.alive_list(), lists[0]); np.testing.assert_array_equal(fa.dead_list(), lists[1])
    assert fa.metadata() == lists[2], "lists, alive bytes and counters are untouched by the call"
    life = fa.read_attr(A.LIFETIME.id).view(F32)
    assert (life > F32(0.3)).sum() > cap // 2 and (life < F32(0.8)).sum() > cap // 2
    alive = fa.alive_count()
    run_stretch([(ca, fa), (cb, fb)], 7, asset, "lifetimes from neighbour counts")
    assert fa.alive_count() < alive and fa.check()["ok"] == 1              # particles died on the way, in both
    ca.close(); cb.close()


# ---- scratch reuse ----------------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_share_the_scratch_in_stream_order_between_a_binned_export_and_a_sample():
    cap = 4097
    ctx = bh.Context(0)
    prog = ctx.create_program(bh.lower(trails_vec4(cap)))
    fxs = [prog.create_effect(), prog.create_effect()]
    ctx.frame_begin(1 / 600, 0.0)
    for k, fx in enumerate(fxs):
        fx.set_frame(cap - 100 * k, frame_seed(k))
    ctx.simulate()
    ctx.frame_begin(0.05, 0.05)
    for k, fx in enumerate(fxs):
        fx.set_frame(0, frame_seed(7 + k))
    ctx.simulate()
    calls = [(0, (3, 3, 3), 0.9, W_ONE), (1, (9, 8, 7), 0.5, W_U3), (0, (12, 12, 12), 1.0, W_U2), (0, (2, 2, 2), 0.7, W_U1), (1, (41, 41, 41), 0.999, W_U3)]
    # the expectations one after the other on the host, each from the planes the one before left; then all the calls with no synchronisation between
    # them, a binned export and a sample of the same effect among them
    steps = []
    for which, dims, part, weight in calls:
        fx = fxs[which]
        grid = grid_around(fx, dims)
        before, want, stats, ref = expected(fx, grid, radius_of(grid, part), weight, CH3, 4096, 0.5)
        steps.append((fx, grid, radius_of(grid, part), weight, want, stats, ref))
        for a, w in want.items():
            fx.write_attr(a, w)
    assert any(s[5][1] > 0 and s[6]["nnb"].sum() > 0 for s in steps)
    ctx.close()
    # a fresh context reaches the same state deterministically: the calls run there without a synchronisation between them
    ctx = bh.Context(0)
    prog = ctx.create_program(bh.lower(trails_vec4(cap)))
    fys = [prog.create_effect(), prog.create_effect()]
    ctx.frame_begin(1 / 600, 0.0)
    for k, fx in enumerate(fys):
        fx.set_frame(cap - 100 * k, frame_seed(k))
    ctx.simulate()
    ctx.frame_begin(0.05, 0.05)
    for k, fx in enumerate(fys):
        fx.set_frame(0, frame_seed(7 + k))
    ctx.simulate()
    sts, keep = [], []
    fld = torch.zeros((27, 1), dtype=torch.float32, device="cuda")         # a sample that adds zero: it runs, and changes no bit of a finite plane
    torch.cuda.synchronize()
    for (which, dims, part, weight), (fx, grid, radius, w_, want, stats, ref) in zip(calls, steps):
        fy = fys[which]
        sts.append(Stats())
        table = Grid(grid.dims, grid.origin, grid.inv_cell)
        keep.append((table, run_binned(Export(POS_AGE_LIFE_VEL, 32, cap), fy, table)))   # (kept: their buffers stay allocated until the stream has run them)
        fy.neighbours(grid.dims, grid.origin, grid.inv_cell, radius, CH3, weight, 4096, 0.5, sts[-1].ptr())
        fy.sample((3, 3, 3), (-8, -8, -8), (3 / 16,) * 3, fld.data_ptr(), [(A.LIFETIME.id, 0, runtime.SAMPLE_ADD)], runtime.SAMPLE_NEAREST, 1.0)
    ctx.synchronize()
    for st, (fx, grid, radius, weight, want, stats, ref) in zip(sts, steps):
        np.testing.assert_array_equal(st.read(), stats)
    last = {}
    for (which, *_), s in zip(calls, steps):
        last[which] = s
    for which, (fx, grid, radius, weight, want, stats, ref) in last.items():
        assert_planes(fys[which], want, ref, f"effect {which} after every call")
    ctx.close()


# ---- argument errors --------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    """Every refusal class on a live effect but a layout without POSITION and an effect of too many slots, which the stand-alone program of
    tests/test_neighbours_abi.py holds"""
    cap = 5000
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    lib = runtime.load_library()
    grid = grid_around(fx, (6, 6, 6))
    radius = radius_of(grid)
    st = Stats()
    good = lambda: runtime.neighbour_desc(grid.dims, grid.origin, grid.inv_cell, radius, CH3, W_U3, 4096, 1.0, st.ptr())
    nan, inf = float("nan"), float("inf")
    ctx.synchronize()
    before = planes(fx, ATTRS4)

    def refused(desc, text):
        assert lib.hnb_effect_neighbours(fx._h, C.byref(desc)) == -1, text
        err = lib.hnb_last_error()
        assert err and text.encode() in err, (text, err)

    assert lib.hnb_effect_neighbours(None, C.byref(good())) == -1 and b"NULL" in lib.hnb_last_error()
    assert lib.hnb_effect_neighbours(fx._h, None) == -1 and b"NULL" in lib.hnb_last_error()
    x = good(); x.struct_size = 196
    refused(x, "struct_size")
    x = good(); x.flags = 1
    refused(x, "flags: 0")
    for d in ((0, 4, 4), (4096, 4096, 2)):
        x = good(); x.dims = (C.c_uint32 * 3)(*d)
        refused(x, "HNB_BIN_MAX_CELLS")
    x = good(); x.origin[1] = nan
    refused(x, "origin is not finite")
    for bad in (0.0, -1.0, inf, nan):
        x = good(); x.inv_cell[2] = bad
        refused(x, "inv_cell is not finite and above 0")
    for bad in (0.0, -1.0, inf, nan):
        x = good(); x.radius = bad
        refused(x, "radius is not finite and above 0")
    x = good(); x.radius = 1.01 * radius
    refused(x, "radius * inv_cell is above 1")
    x = good(); x.radius = 1e-20; x.inv_cell = (C.c_float * 3)(1e-30, 1e-30, 1e-30)
    refused(x, "not a normal number")
    x = good(); x.weight = 4
    refused(x, "weight: HNB_NEIGHBOUR_W_ONE")
    for bad in (0, 65537):
        x = good(); x.candidate_limit = bad
        refused(x, "candidate_limit is not 1..")
    for n in (0, 5):
        x = good(); x.n_channels = n
        refused(x, "n_channels is not 1..")
    for attr in (A.COLOR.id, A.SIZE3.id, A.ID.id, 9999):
        x = good(); x.channels[2].src_attr = attr
        refused(x, "channels[2]")
        assert b"src_attr is not HNB_SPLAT_ATTR_ONE" in lib.hnb_last_error()
    x = good(); x.channels[2].src_comp = 3
    refused(x, "src_comp is at or past")
    x = good(); x.channels[0].src_comp = 1
    refused(x, "src_comp is at or past")
    x = good(); x.channels[2].flags = 2
    refused(x, "flags: 0 or HNB_NEIGHBOUR_DIFF")
    x = good(); x.channels[1].flags = 1
    refused(x, "HNB_NEIGHBOUR_DIFF of HNB_SPLAT_ATTR_ONE")
    x = good(); x.channels[1].frac_bits = 33
    refused(x, "frac_bits is above 32")
    for attr in (A.AGE.id, A.COLOR.id, A.ID.id, 9999):
        x = good(); x.channels[1].dst_attr = attr
        refused(x, "dst_attr is not an f32 attribute")
    x = good(); x.channels[1].dst_comp = 4
    refused(x, "dst_comp is at or past")
    x = good(); x.channels[1].op = 2
    refused(x, "op: HNB_SAMPLE_SET or")
    x = good(); x.channels[1].reserved = 1
    refused(x, "reserved is not 0")
    x = good(); x.channels[1].dst_comp = 0
    refused(x, "an earlier channel's")
    x = good(); x.channels[3].op = 1
    refused(x, "at or past n_channels")
    for bad in (nan, inf, -inf):
        x = good(); x.scale = bad
        refused(x, "scale is not finite")
    x = good(); x.out_stats = st.ptr() + 4
    refused(x, "out_stats: NULL or")
    ctx.synchronize()
    assert st.untouched()
    after = planes(fx, ATTRS4)
    for a in before:
        np.testing.assert_array_equal(after[a], before[a])
    check(ctx, fx, grid, radius, "a good call behind the refusals")         # ... and the same effect takes a good call
    fx.neighbours(grid.dims, grid.origin, grid.inv_cell, radius, CH3)       # out_stats may be NULL
    ctx.synchronize()
    ctx.close()
