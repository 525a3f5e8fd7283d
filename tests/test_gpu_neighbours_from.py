"""hnb_effect_neighbours_from on the GPU (include/hanabi_amd_neighbours_from.h): for every alive particle of fx inside a uniform grid, up to four
fixed-point sums over the particles of ANOTHER effect of the same context within a radius and within one cell of it, stored or added into components of
f32 attributes of fx. The expectation is always the brute-force numpy restatement (tests/test_neighbours_from_abi.py np_neighbours_from, over
test_neighbours_abi's np_store) over the host's read-back of BOTH effects, compared bit for bit over WHOLE planes of fx (dead slots, outside and crowded
queries and unnamed components included) and over whole planes of the source before and after. There is no tolerance anywhere. The stats sit between
guard words filled with a sentinel. Before comparing, each main case asserts on the restatement alone what makes the case worth running."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, frame_seed
from test_bounds_abi import trails_vec4
from test_gpu_export import _device_meta
from test_gpu_export_binned import Grid
from test_gpu_import import planes
from test_gpu_neighbours import ATTRS4, CH3, DIMS, Stats, radius_of
from test_neighbours_abi import ADD, DIFF, ONE, SET, W_ONE, W_U1, W_U2, W_U3, np_store, one_source
from test_neighbours_from_abi import from_stats, np_neighbours_from

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
TRAIL = [A.POSITION.id, A.VELOCITY.id, A.AGE.id, A.LIFETIME.id]          # what firework_trails and trails_vec4 share
OFFSETS27 = set(itertools.product((-1, 0, 1), repeat=3))
COUNT = [(ONE, 0, 0, 0, A.F32X4_0.id, 0, SET)]
S_SEED = 500                                                              # the source's frames take other seeds than fx's


def make2(cap_q, cap_s, asset_q=None, asset_s=None, **options):
    """one context, two effects of two programs: fx (trails_vec4 unless given) and the source"""
    ctx = bh.Context(0)
    for o, v in options.items():
        ctx.set_option(o, v)
    fq = ctx.create_program(bh.lower(asset_q if asset_q is not None else trails_vec4(cap_q))).create_effect()
    fs = ctx.create_program(bh.lower(asset_s if asset_s is not None else trails_vec4(cap_s))).create_effect()
    return ctx, fq, fs


def step2(ctx, fq, fs, f, spawn_q, spawn_s, dt=1 / 600, seed_s=S_SEED):
    ctx.frame_begin(dt, f * dt)
    fq.set_frame(spawn_q, frame_seed(f))
    fs.set_frame(spawn_s, frame_seed(f + seed_s))
    ctx.simulate()


def burst2(cap_q, cap_s, asset_q=None, asset_s=None, seed_s=S_SEED, **options):
    """both burst from the origin and are stepped once with dt = 0.05: two overlapping shells 2 .. 3 units from it"""
    ctx, fq, fs = make2(cap_q, cap_s, asset_q, asset_s, **options)
    step2(ctx, fq, fs, 0, cap_q, cap_s, seed_s=seed_s)
    step2(ctx, fq, fs, 1, 0, 0, dt=0.05, seed_s=seed_s)
    return ctx, fq, fs


def grid_over(fxs, dims, inner=None):
    """test_gpu_export_binned.grid_around over the alive particles of several effects"""
    p = np.concatenate([fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)[fx.alive_list()] for fx in fxs]).astype(np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    lo, hi = (p.min(axis=0), p.max(axis=0)) if len(p) else (np.full(3, -1.0), np.full(3, 1.0))
    size = np.maximum(hi - lo, 1e-3)
    if inner is None:
        lo, size = lo - 0.01 * size, 1.02 * size
    else:
        lo, size = lo + 0.5 * (1 - inner) * size, inner * size
    return Grid(dims, lo, np.asarray(dims, np.float64) / size)


def expected(fq, fs, grid, radius, weight, channels, limit, scale, attrs_q=ATTRS4, attrs_s=ATTRS4):
    """The restatement over the host's read-back of both effects as they are (synchronises). -> (want: attribute -> [capacity, ncomp] words of fx;
    source: the same of the source, which must not change; stats [8]; ref: np_neighbours_from's result, with `alive_q` and `alive_s`)"""
    before_q, before_s = planes(fq, attrs_q), planes(fs, attrs_s)
    alive_q, alive_s = fq.alive_list(), fs.alive_list()
    src = [one_source(fs.capacity) if ch[0] == ONE else before_s[int(ch[0])][:, ch[1]].copy() for ch in channels]
    own = [before_q[int(ch[0])][:, ch[1]].copy() if ch[2] & DIFF else None for ch in channels]
    ref = np_neighbours_from(before_q[int(A.POSITION.id)].view(F32), alive_q, before_s[int(A.POSITION.id)].view(F32), alive_s, src, own,
                             (grid.dims, grid.origin, grid.inv_cell), radius, weight, channels, limit)
    g = ref["gathered"]
    want = {a: p.copy() for a, p in before_q.items()}
    for k, ch in enumerate(channels):
        out = np_store(ch[6], before_q[int(ch[4])][:, ch[5]].view(F32), ref["S"][:, k], ch[3], scale)
        want[int(ch[4])][g, ch[5]] = out.view(U32)[g]
    ref["alive_q"], ref["alive_s"] = alive_q, alive_s
    return want, before_s, from_stats(ref, len(alive_q)), ref


def assert_planes(fx, want, what, ref=None):
    got = planes(fx, list(want))
    for a, w in want.items():
        ok = (got[a] == w) | (np.isnan(w.view(F32)) & np.isnan(got[a].view(F32)))
        bad = np.argwhere(~ok)
        assert not len(bad), (what, f"attribute {a}", len(bad), [(int(s), int(c), hex(int(got[a][s, c])), hex(int(w[s, c])), ref and bool(ref["gathered"][s]), ref and int(ref["nnb"][s]))
                                                                 for s, c in bad[:6]])


def check(ctx, fq, fs, grid, radius, what, channels=CH3, weight=W_U3, limit=4096, scale=1.0, attrs_q=ATTRS4, attrs_s=ATTRS4, conditions=None):
    """one call against the restatement: whole planes of fx, whole planes of the source, stats, guard words -> (want, stats, ref)"""
    want, source, stats, ref = expected(fq, fs, grid, radius, weight, channels, limit, scale, attrs_q, attrs_s)
    if conditions:
        conditions(ref)
    st = Stats()
    fq.neighbours_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, channels, weight, limit, scale, st.ptr())
    ctx.synchronize()
    assert_planes(fq, want, what, ref)
    assert_planes(fs, source, what + ": the source")
    np.testing.assert_array_equal(st.read(), stats, err_msg=f"{what}: out_stats")
    return want, stats, ref


# ---- capacities: the one-workgroup sort and the multi-tile one on each side independently, a partial last tile --------------------------------------
CAPS = [(1, 1), (3, 300), (300, 3), (4096, 4097), (4097, 4096), (10_000, 300)]


@pytest.mark.parametrize("cap_q,cap_s", CAPS)
def test_capacities_on_the_burst_states(cap_q, cap_s):
    ctx, fq, fs = burst2(cap_q, cap_s)
    grid = grid_over([fq, fs], DIMS[min(cap_q, cap_s)])
    radius = radius_of(grid)

    def conditions(ref):
        g = ref["gathered"]
        assert not ref["crowded"].any() and g.sum() == cap_q and ref["s_inside"] == cap_s, "nobody is crowded or outside"
        if min(cap_q, cap_s) >= 300:
            assert 2 * int((ref["nnb"][g] >= 3).sum()) >= int(g.sum()), "at least half the gathered queries have three neighbours or more"
        if min(cap_q, cap_s) >= 4096:
            assert OFFSETS27 <= ref["offsets"], ("a pair for every one of the 27 cell offsets", OFFSETS27 - ref["offsets"])

    want, stats, ref = check(ctx, fq, fs, grid, radius, f"capacities {cap_q}, {cap_s}", conditions=conditions)
    assert list(stats) == [cap_q, cap_q, 0, 0, ref["rejected"], cap_s, cap_s, 0]
    if max(cap_q, cap_s) > 1:
        assert ref["nnb"].sum() > 0, "somebody has neighbours"
    for weight in (W_ONE, W_U1, W_U2):                                     # the other weights on the same state (fx's planes as the call above left them), a negative scale
        check(ctx, fq, fs, grid, radius, f"capacities {cap_q}, {cap_s}, weight {weight}", weight=weight, scale=-0.5)
    assert fq.check()["ok"] == 1 and fs.check()["ok"] == 1
    ctx.close()


# ---- a grid that cuts through both clouds -------------------------------------------------------------------------------------------------------------
def test_a_grid_that_cuts_through_both_clouds_outside_queries_keep_every_bit_outside_sources_count_for_nobody():
    ctx, fq, fs = burst2(10_000, 4097)
    grid = grid_over([fq, fs], (6, 6, 6), inner=0.6)
    radius = radius_of(grid)

    def conditions(ref):
        aq, as_ = ref["alive_q"], ref["alive_s"]
        assert 0 < ref["inside"].sum() < len(aq) and 0 < ref["s_inside"] < len(as_), "there is an outside bin on each side"
        pq = fq.read_attr(A.POSITION.id).view(F32).reshape(-1, 3).astype(np.float64)
        ps = fs.read_attr(A.POSITION.id).view(F32).reshape(-1, 3).astype(np.float64)
        cells_s = grid.cells(ps.astype(F32))
        out_s = as_[cells_s[as_] == grid.n_cells]
        ins_q = np.flatnonzero(ref["inside"])
        near = sum(int((((pq[ins_q] - ps[o]) ** 2).sum(axis=1) < 0.9 * radius * radius).sum()) for o in out_s[:400])
        assert near > 0, "outside sources within the radius of an inside query: they must not count"
        c = ref["cells"][ins_q]
        on_edge = ((np.stack([c % 6, (c // 6) % 6, c // 36], axis=1) == 0) | (np.stack([c % 6, (c // 6) % 6, c // 36], axis=1) == 5)).sum(axis=1)
        assert {1, 2, 3} <= set(on_edge.tolist()), "queries in face, edge and corner cells of the grid"

    want, stats, ref = check(ctx, fq, fs, grid, radius, "inner 0.6", conditions=conditions)
    assert 0 < stats[2] < stats[0] and stats[5] < stats[6] == 4097
    ctx.close()


# ---- crowding -----------------------------------------------------------------------------------------------------------------------------------------
def test_crowded_queries_keep_every_bit_and_the_count_is_exact():
    cap_q, cap_s = 300, 300
    ctx, fq, fs = burst2(cap_q, cap_s)
    rng = np.random.default_rng(2)
    ps = np.empty((cap_s, 3), F32)
    ps[:200] = (1.5 + rng.uniform(-0.3, 0.3, (200, 3))).astype(F32)        # 200 sources bunched into cell (1, 1, 1) of a 5 x 4 x 4 grid of unit cells
    ps[200:240] = (np.array([3.3, 1.5, 1.5]) + rng.uniform(0, 0.4, (40, 3))).astype(F32)      # 40 in (3, 1, 1)
    ps[240:] = (np.array([1.5, 3.5, 3.5]) + rng.uniform(-0.4, 0.4, (60, 3))).astype(F32)      # and 60 far away
    fs.write_attr(A.POSITION.id, ps)
    pq = np.empty((cap_q, 3), F32)
    pq[:100] = (np.array([0.5, 0.5, 0.5]) + rng.uniform(0, 2.4, (100, 3))).astype(F32)        # queries in the cells around (1, 1, 1): crowded by the sources alone
    pq[100:200] = (np.array([3.1, 1.1, 1.1]) + rng.uniform(0, 0.8, (100, 3))).astype(F32)     # 100 queries - more than the limit, and no candidates - in (3, 1, 1): 40 sources each
    pq[200:] = (np.array([4.5, 3.5, 0.5]) + rng.uniform(-0.4, 0.4, (100, 3))).astype(F32)     # and 100 with no source near
    fq.write_attr(A.POSITION.id, pq)
    grid = Grid((5, 4, 4), (0, 0, 0), (1, 1, 1))

    def conditions(ref):
        g, cr = ref["gathered"], ref["crowded"]
        assert cr[:100].all() and not cr[100:].any() and g[100:].all(), "crowding is decided by the sources: a hundred queries in one cell are not crowded by each other"
        assert (ref["cand"][100:200] == 40).all() and (ref["nnb"][100:200] > 0).all() and (ref["cand"][200:] == 0).all()

    want, stats, ref = check(ctx, fq, fs, grid, 1.0, "crowding", limit=64, conditions=conditions)
    assert stats[3] == 100 and stats[1] == 200
    ctx.close()


# ---- empty sides --------------------------------------------------------------------------------------------------------------------------------------
def test_a_source_that_never_spawned_and_an_fx_that_never_spawned():
    cap = 300
    ctx, fq, fs = make2(cap, cap)
    step2(ctx, fq, fs, 0, cap, 0)
    step2(ctx, fq, fs, 1, 0, 0, dt=0.05)
    assert fs.alive_count() == 0 and fq.alive_count() == cap
    grid = grid_over([fq], (4, 4, 4))
    ch = [(ONE, 0, 0, 0, A.F32X4_0.id, 0, SET), (ONE, 0, 0, 8, A.F32X4_0.id, 1, ADD), (A.POSITION.id, 0, DIFF, 16, A.VELOCITY.id, 1, ADD)]
    before = planes(fq, ATTRS4)
    want, stats, ref = check(ctx, fq, fs, grid, radius_of(grid), "no sources", channels=ch, scale=-2.0)
    assert list(stats) == [cap, cap, 0, 0, 0, 0, 0, 0]
    f4 = want[int(A.F32X4_0.id)]
    assert (f4[:, 0] == 0x80000000).all(), "SET stores the formula's value for S = 0: 0.0 * -2.0"
    np.testing.assert_array_equal(f4[:, 1], (before[int(A.F32X4_0.id)][:, 1].view(F32) + F32(-0.0)).view(U32))      # ... and ADD adds it
    # the other way round: an fx that never spawned - nothing is written, nobody is visited
    want, stats, ref = check(ctx, fs, fq, grid, radius_of(grid), "no queries", channels=ch)
    assert list(stats) == [0, 0, 0, 0, 0, cap, cap, 0]
    ctx.close()


# ---- deaths on both sides; the list forms -------------------------------------------------------------------------------------------------------------
def test_deaths_on_both_sides_suffix_lists_a_churn_list_and_after_a_re_spawn():
    cap_q, cap_s = 10_000, 8000
    ctx, fq, fs = make2(cap_q, cap_s, asset_s=effects.firework_trails(cap_s, spawner=bh.SpawnerSettings.rate(3000.0)))
    rng = np.random.default_rng(5)
    step2(ctx, fq, fs, 0, cap_q, 600)
    for f in range(1, 5):
        step2(ctx, fq, fs, f, 0, int(rng.integers(100, 600)), dt=0.25)
    aq, as_ = fq.alive_list(), fs.alive_list()
    assert 0 < len(aq) < cap_q and not np.array_equal(aq, np.arange(len(aq))), "part of fx has died"
    grid = grid_over([fq, fs], (5, 5, 5), inner=0.9)
    ch = [(ONE, 0, 0, 0, A.F32X4_0.id, 0, SET), (A.LIFETIME.id, 0, 0, 20, A.F32X4_0.id, 2, ADD), (A.AGE.id, 0, DIFF, 16, A.VELOCITY.id, 1, ADD)]
    want, stats, ref = check(ctx, fq, fs, grid, radius_of(grid), "die-off", channels=ch, weight=W_U1, attrs_s=TRAIL, limit=8000)
    assert stats[0] == len(aq) and stats[6] == len(as_) and stats[2] > 0
    for f in range(5, 40):                                                 # the source churns on; fx re-spawns into the slots its dead left
        step2(ctx, fq, fs, f, 300 if f % 4 == 0 else 0, int(rng.integers(100, 600)), dt=1 / 20)
    aq, as_ = fq.alive_list(), fs.alive_list()
    assert 256 < len(as_) < cap_s and not np.array_equal(as_, np.sort(as_)), "a churn list on the source"
    assert 256 < len(aq) < cap_q and not np.array_equal(aq, np.sort(aq)), "a list after deaths and re-spawns on fx"
    grid = grid_over([fq, fs], (4, 4, 4), inner=0.8)

    def conditions(ref):
        dead_s = np.setdiff1d(np.arange(cap_s), as_)
        assert len(dead_s) > 0 and ref["nnb"].sum() > 0 and ref["gathered"].sum() > 0
        ps = fs.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)
        cells = grid.cells(ps)
        assert (cells[dead_s] != grid.n_cells).any(), "dead source slots hold positions inside the grid: they count for nobody"

    want, stats, ref = check(ctx, fq, fs, grid, radius_of(grid), "churn and re-spawn", channels=ch, weight=W_U2, attrs_s=TRAIL, limit=8000, conditions=conditions)
    assert stats[0] == len(aq) and stats[6] == len(as_)
    assert fq.check()["ok"] == 1 and fs.check()["ok"] == 1
    ctx.close()


def test_a_ring_list_on_the_source_is_read_through_its_head_and_left_alone():
    cap_q, cap_s = 4097, 10_000
    asset = effects.ribbon(cap_s)
    ctx, fq, fs = make2(cap_q, cap_s, asset_s=asset, ring_lists=1)
    sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
    for f in range(90):
        dt = 1 / 60
        ctx.frame_begin(dt, f * dt)
        fq.set_frame(cap_q if f == 60 else 0, frame_seed(f))
        fs.set_frame(sp.tick(dt, rng), frame_seed(f + S_SEED))
        ctx.simulate()
    ctx.synchronize()
    m = _device_meta(fs)
    assert (m.list_column >> 1) != 0 and m.alive_count > 256               # kept as a ring, the head somewhere inside the column
    before = fs.alive_list().copy()
    fs.write_attr(A.POSITION.id, np.random.default_rng(3).uniform(-1, 1, (cap_s, 3)).astype(F32).view(np.uint32))     # (the ribbon's particles sit on one point: spread them)
    fq.write_attr(A.POSITION.id, np.random.default_rng(4).uniform(-1.2, 1.2, (cap_q, 3)).astype(F32).view(np.uint32))
    grid = grid_over([fs], (5, 4, 3), inner=0.8)
    ch = [(ONE, 0, 0, 0, A.F32X4_0.id, 0, SET), (A.SIZE.id, 0, 0, 16, A.F32X4_0.id, 1, SET)]
    want, stats, ref = check(ctx, fq, fs, grid, radius_of(grid), "ring", channels=ch, weight=W_ONE, attrs_s=[A.POSITION.id, A.AGE.id, A.SIZE.id])
    assert stats[6] == m.alive_count and 0 < stats[5] < stats[6] and 0 < stats[2] < stats[0] and ref["nnb"].sum() > 0
    np.testing.assert_array_equal(fs.alive_list(), before)                 # the list, and with it the ribbon's own sort order, is what it was
    m2 = _device_meta(fs)
    assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


# ---- non-finite positions on each side ----------------------------------------------------------------------------------------------------------------
def test_non_finite_positions_land_outside_on_either_side_and_rejected_contributions_are_counted():
    cap_q, cap_s = 4097, 4096
    ctx, fq, fs = burst2(cap_q, cap_s)
    ctx.synchronize()
    nan, inf = F32(np.nan), F32(np.inf)
    special = [(nan, 0.5, 0.5), (0.5, -nan, 0.5), (inf, 0.5, 0.5), (0.5, 0.5, -inf), (-0.0, -0.0, -0.0), (0.0, 0.0, 0.0), (-0.0, 0.5, 1.0)]
    rows = np.arange(7, 7 + 500 * len(special), 500)
    for fx in (fq, fs):
        pos = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3).copy()
        pos[rows] = np.array(special, F32)
        fx.write_attr(A.POSITION.id, pos)
    vel = fs.read_attr(A.VELOCITY.id).view(F32).reshape(-1, 3).copy()
    vel[::5, 2] = nan; vel[1::7, 2] = inf; vel[2::11, 2] = F32(1e30); vel[3::13, 2] = F32(1e-41)
    fs.write_attr(A.VELOCITY.id, vel)
    grid = Grid((4, 4, 4), (0, 0, 0), (1, 1, 1))                           # the origin at 0: -0 is inside; the clouds' negative halves are outside
    ch = [(A.VELOCITY.id, 2, 0, 32, A.F32X4_0.id, 2, SET), (ONE, 0, 0, 0, A.F32X4_0.id, 0, SET), (A.VELOCITY.id, 0, DIFF, 8, A.LIFETIME.id, 0, ADD)]

    def conditions(ref):
        assert not ref["inside"][rows[:4]].any() and ref["inside"][rows[4:]].all(), "non-finite query positions are outside, signed zeros inside"
        cells_s = grid.cells(fs.read_attr(A.POSITION.id).view(F32).reshape(-1, 3))
        assert (cells_s[rows[:4]] == grid.n_cells).all() and (cells_s[rows[4:]] != grid.n_cells).all(), "... and the same on the source"
        assert ref["nnb"][rows[4:6]].min() >= 2, "the queries at the origin count the sources at the origin: coincident, at equal slot numbers"
        assert ref["rejected"] > 0 and ref["nnb"].sum() > ref["rejected"]

    want, stats, ref = check(ctx, fq, fs, grid, 0.8, "special positions, rejected contributions", channels=ch, weight=W_U1, conditions=conditions)
    assert stats[4] == ref["rejected"] % (1 << 32) and 0 < stats[2] < stats[0] and 0 < stats[5] < stats[6]
    ctx.close()


# ---- hazard freedom -----------------------------------------------------------------------------------------------------------------------------------
def test_a_destination_that_is_fx_s_position_or_the_diff_operand_sees_the_state_before_the_call():
    ctx, fq, fs = burst2(4097, 4096)
    grid = grid_over([fq, fs], (7, 7, 7))
    want, stats, ref = check(ctx, fq, fs, grid, radius_of(grid), "POSITION.x into itself", channels=[(A.POSITION.id, 0, DIFF, 20, A.POSITION.id, 0, ADD)], weight=W_U2, scale=0.01)
    assert ref["nnb"].sum() > 4097 and (ref["S"][:, 0] != 0).any()
    grid = grid_over([fq, fs], (7, 7, 7))
    ch = [(A.VELOCITY.id, 0, DIFF, 10, A.VELOCITY.id, 0, SET), (A.VELOCITY.id, 1, DIFF, 10, A.POSITION.id, 2, ADD), (A.POSITION.id, 2, DIFF, 10, A.VELOCITY.id, 1, SET)]
    want, stats, ref = check(ctx, fq, fs, grid, radius_of(grid), "destinations that are DIFF operands", channels=ch, weight=W_U1, scale=0.001)
    assert ref["nnb"].sum() > 4097
    ctx.close()


# ---- stale AGE ----------------------------------------------------------------------------------------------------------------------------------------
def test_stale_age_as_a_diff_source_is_materialised_on_both_effects_by_the_call():
    """LEAN cohorts: the AGE planes are stale until something materialises them. The test does not (a read-back of AGE would): it calls first and
    states the expectation from the read-back afterwards - AGE and POSITION are no destination, and a SET needs no earlier value."""
    cap = 10_000
    ctx, fq, fs = make2(cap, cap, age_cohort=1)
    assert fq.device_view().stale_attr_mask == 1 << A.AGE.id and fs.device_view().stale_attr_mask == 1 << A.AGE.id
    for f in range(4):
        step2(ctx, fq, fs, f, 6000 if f == 0 else 1000, 5000 if f == 0 else 1500, dt=1 / 60)
    grid = Grid((6, 6, 6), (-3, -3, -3), (1, 1, 1))
    ch = [(A.AGE.id, 0, 0, 24, A.F32X4_0.id, 3, SET), (A.AGE.id, 0, DIFF, 24, A.F32X4_0.id, 2, SET)]
    st = Stats()
    fq.neighbours_from(fs, grid.dims, grid.origin, grid.inv_cell, 1.0, ch, W_U1, 8192, 1.0, st.ptr())
    ctx.synchronize()
    want, source, stats, ref = expected(fq, fs, grid, 1.0, W_U1, ch, 8192, 1.0)
    ages_q = want[int(A.AGE.id)][ref["alive_q"], 0].view(F32)
    ages_s = source[int(A.AGE.id)][ref["alive_s"], 0].view(F32)
    assert len(np.unique(ages_q)) == 4 and len(np.unique(ages_s)) == 4 and ref["nnb"].sum() > 0 and (ref["S"][:, 1] != 0).any()
    assert_planes(fq, want, "stale AGE", ref)                              # (idempotent here: the destinations hold what the call stored)
    np.testing.assert_array_equal(st.read(), stats)
    ctx.close()


# ---- two instances of one program; a frozen source ------------------------------------------------------------------------------------------------------
def test_fx_and_source_as_two_instances_of_one_program_and_frozen_instances():
    cap = 4097
    ctx = bh.Context(0)
    prog = ctx.create_program(bh.lower(trails_vec4(cap)))
    fq, fs = prog.create_effect(), prog.create_effect()
    step2(ctx, fq, fs, 0, cap, cap - 100)
    step2(ctx, fq, fs, 1, 0, 0, dt=0.05)
    grid = grid_over([fq, fs], (7, 7, 7))
    want, stats, ref = check(ctx, fq, fs, grid, radius_of(grid), "one program")
    assert list(stats[:4]) == [cap, cap, 0, 0] and list(stats[5:]) == [cap - 100, cap - 100, 0] and ref["nnb"].sum() > cap
    fs.set_simulated(False)
    check(ctx, fq, fs, grid, radius_of(grid), "one program, the source frozen", weight=W_U1)
    fq.set_simulated(False)
    check(ctx, fs, fq, grid, radius_of(grid), "one program, both frozen, roles swapped", weight=W_U2)
    ctx.close()


# ---- two invariants that need no restatement -----------------------------------------------------------------------------------------------------------
def _counts(fx):
    return fx.read_attr(A.F32X4_0.id).view(F32).reshape(-1, 4)[fx.alive_list(), 0].astype(np.int64)


def test_swapped_roles_count_the_same_pairs():
    ctx, fq, fs = burst2(4097, 3000)
    grid = grid_over([fq, fs], (7, 7, 7))
    radius = radius_of(grid)
    sa, sb = Stats(), Stats()
    fq.neighbours_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, COUNT, W_ONE, 4096, 1.0, sa.ptr())
    fs.neighbours_from(fq, grid.dims, grid.origin, grid.inv_cell, radius, COUNT, W_ONE, 4096, 1.0, sb.ptr())       # (POSITION is no destination: the second call sees the same positions)
    ctx.synchronize()
    a, b = sa.read(), sb.read()
    assert a[3] == 0 and b[3] == 0 and a[2] == 0 and b[2] == 0, "nobody is crowded or outside"
    assert (a[0], a[5], a[6]) == (4097, 3000, 3000) and (b[0], b[5], b[6]) == (3000, 4097, 4097)
    assert _counts(fq).sum() == _counts(fs).sum() > 4097                   # the relation is symmetric bit for bit: d2 of (i, j) is d2 of (j, i)
    ctx.close()


@pytest.mark.parametrize("limit", [4096, 400])
def test_a_twin_source_counts_what_hnb_effect_neighbours_counts_plus_the_twin_of_the_query_itself(limit):
    cap = 4097
    ctx, fq, fs = burst2(cap, cap, seed_s=0)                               # the same asset, seeds and frames: the source's state is fx's
    grid = grid_over([fq], (7, 7, 7))
    radius = radius_of(grid)
    sa, sb = Stats(), Stats()
    fq.neighbours(grid.dims, grid.origin, grid.inv_cell, radius, COUNT, W_ONE, limit, 1.0, sa.ptr())
    ctx.synchronize()
    own, a = _counts(fq), sa.read()
    sentinel = np.full((cap, 4), -7.0, F32)
    fq.write_attr(A.F32X4_0.id, sentinel)
    fq.neighbours_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, COUNT, W_ONE, limit, 1.0, sb.ptr())
    ctx.synchronize()
    b = sb.read()
    np.testing.assert_array_equal(a[:5], b[:5])                            # crowding coincides: the candidate counts coincide
    assert (a[3] > 0) == (limit < 4096) and a[1] > 0
    twin = _counts(fq)
    gathered = twin != -7
    assert gathered.sum() == b[1] and (twin[gathered] == own[gathered] + 1).all() and own[gathered].sum() > 0
    ctx.close()


# ---- the state after the call ---------------------------------------------------------------------------------------------------------------------------
def test_the_source_is_untouched_and_fx_is_what_write_attr_of_the_same_values_leaves():
    """Two contexts run the same frames; A makes the call, B does not and receives fx's planes through hnb_effect_write_attr. The source of A equals the
    source of B right after the call and after a stretch of single frames and a hnb_simulate_steps call; so does fx."""
    cap_q, cap_s = 20_000, 12_000
    A_, B_ = [make2(cap_q, cap_s, age_cohort=3) for _ in range(2)]                 # (both trails_vec4: two shells of the same radii)
    for f in range(6):
        for ctx, fq, fs in (A_, B_):
            step2(ctx, fq, fs, f, cap_q if f == 0 else 0, cap_s if f == 0 else 0, dt=1 / 30)
    (ca, qa, sa), (cb, qb, sb) = A_, B_
    grid = grid_over([qa, sa], (12, 12, 12), inner=0.9)
    for ctx, fq, fs in (A_, B_):                                           # lifetimes of 0.3 s + 1 ms per neighbouring source: below the bounds the frames published
        fq.write_attr(A.LIFETIME.id, np.full(cap_q, 0.3, F32))
        step2(ctx, fq, fs, 6, 0, 0, dt=1 / 300)
    ca.synchronize()
    lists = (sa.alive_list().copy(), sa.dead_list().copy(), sa.metadata(), qa.alive_list().copy(), qa.metadata())
    st = Stats()
    qa.neighbours_from(sa, grid.dims, grid.origin, grid.inv_cell, radius_of(grid), [(ONE, 0, 0, 0, A.LIFETIME.id, 0, ADD)], W_ONE, 65536, 0.001, st.ptr())   # no synchronisation around it
    qb.write_attr(A.LIFETIME.id, qa.read_attr(A.LIFETIME.id))              # (the read-back waits for the call)
    stats = st.read()
    assert stats[0] == cap_q and 0 < stats[2] < stats[1] and stats[3] == 0 and 0 < stats[5] < stats[6] == cap_s
    assert sa.compare(sb)["equal"] == 1, "the source right after the call"
    np.testing.assert_array_equal(sa.alive_list(), lists[0]); np.testing.assert_array_equal(sa.dead_list(), lists[1])
    assert sa.metadata() == lists[2] and qa.metadata() == lists[4], "lists, alive bytes and counters are untouched by the call"
    np.testing.assert_array_equal(qa.alive_list(), lists[3])
    life = qa.read_attr(A.LIFETIME.id).view(F32)
    assert (life > F32(0.3)).sum() > cap_q // 4
    alive, f, dt = qa.alive_count(), 7, 1 / 30
    for stretch, k in (("single", 11), ("steps", 8), ("single", 11)):
        for ctx, fq, fs in (A_, B_):
            if stretch == "steps":
                fq.set_frames_ahead([0] * k, [frame_seed(f + j) for j in range(k)])
                fs.set_frames_ahead([0] * k, [frame_seed(f + j + S_SEED) for j in range(k)])
                ctx.simulate_steps([(dt, (f + j) * dt) for j in range(k)])
            else:
                for j in range(k):
                    step2(ctx, fq, fs, f + j, 0, 0, dt=dt)
        f += k
        ca.synchronize(); cb.synchronize()
        assert sa.compare(sb)["equal"] == 1, f"the source at frame {f}"
        assert qa.compare(qb)["equal"] == 1, f"fx at frame {f}"
    assert qa.alive_count() < alive, "particles of fx died on the way, in both"
    for fx in (qa, qb, sa, sb):
        assert fx.check()["ok"] == 1
    ca.close(); cb.close()


# ---- calls in sequence ----------------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_regrow_the_scratch_and_interleave_with_neighbours_and_pairs():
    cap_q = 4097
    caps_s = [300, 4096, 10_000]                                           # sources of growing capacity: the scratch of fx regrows twice
    ctx = bh.Context(0)
    fq = ctx.create_program(bh.lower(trails_vec4(cap_q))).create_effect()
    srcs = [ctx.create_program(bh.lower(trails_vec4(c))).create_effect() for c in caps_s]
    for f, dt in ((0, 1 / 600), (1, 0.05)):
        ctx.frame_begin(dt, f * dt)
        fq.set_frame(cap_q if f == 0 else 0, frame_seed(f))
        for k, fs in enumerate(srcs):
            fs.set_frame(caps_s[k] if f == 0 else 0, frame_seed(f + S_SEED + 10 * k))
        ctx.simulate()
    grid = grid_over([fq] + srcs, (7, 7, 7))
    radius = radius_of(grid)
    # the expectations one after the other on the host, each from the planes the one before left
    start = planes(fq, ATTRS4)
    steps = []
    for fs in srcs + [srcs[0]]:
        want, source, stats, ref = expected(fq, fs, grid, radius, W_U3, CH3, 4096, 0.5)
        steps.append((fs, want, source, stats, ref))
        for a, w in want.items():
            fq.write_attr(a, w)
    for a, w in start.items():                                             # back to the start: the same calls with no synchronisation between them
        fq.write_attr(a, w)
    sts = []
    for fs, *_ in steps:
        sts.append(Stats())
        fq.neighbours_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, CH3, W_U3, 4096, 0.5, sts[-1].ptr())
    ctx.synchronize()
    for st, (fs, want, source, stats, ref) in zip(sts, steps):
        np.testing.assert_array_equal(st.read(), stats)
        assert_planes(fs, source, "a source after every call")
    assert_planes(fq, steps[-1][1], "fx after every call", steps[-1][4])
    assert any(s[4]["nnb"].sum() > 0 for s in steps)
    # interleaved with hnb_effect_neighbours and hnb_effect_pairs on the same two effects: the three scratches are separate
    fs = srcs[1]
    rows = torch.zeros(cap_q, dtype=torch.int32, device="cuda"); offs = torch.zeros(cap_q + 1, dtype=torch.int32, device="cuda")
    rows_s = torch.zeros(fs.capacity, dtype=torch.int32, device="cuda"); offs_s = torch.zeros(fs.capacity + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    want, source, stats, ref = expected(fq, fs, grid, radius, W_U2, COUNT, 4096, 1.0)
    sa, sb, sc, sd = Stats(), Stats(), Stats(), Stats()
    only_y = [(ONE, 0, 0, 0, A.F32X4_0.id, 1, SET)]                        # hnb_effect_neighbours writes another component: the two results sit side by side
    fq.pairs(grid.dims, grid.origin, grid.inv_cell, radius, rows.data_ptr(), offs.data_ptr(), stats_ptr=sa.ptr())
    fq.neighbours(grid.dims, grid.origin, grid.inv_cell, radius, only_y, W_ONE, 4096, 1.0, sb.ptr())
    fq.neighbours_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, COUNT, W_U2, 4096, 1.0, sc.ptr())
    fs.pairs(grid.dims, grid.origin, grid.inv_cell, radius, rows_s.data_ptr(), offs_s.data_ptr(), stats_ptr=sd.ptr())
    ctx.synchronize()
    np.testing.assert_array_equal(sc.read(), stats)
    pairs_total = int(sa.read()[4])
    y = fq.read_attr(A.F32X4_0.id).view(F32).reshape(-1, 4)[:, 1]
    assert pairs_total > 0 and int(y.astype(np.int64).sum()) == pairs_total and sb.read()[1] == cap_q and sd.read()[0] == fs.capacity      # the own-effect count is the own-effect pair list's length
    want[int(A.F32X4_0.id)][:, 1] = y.view(U32)
    assert_planes(fq, want, "interleaved", ref)
    assert_planes(fs, source, "interleaved: the source")
    ctx.close()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_on_live_effects_enqueue_nothing():
    """fx == source, two contexts, a DIFF attribute missing from fx's layout, a misaligned out_stats - and a handful of the description's own
    refusals, which the stand-alone program of tests/test_neighbours_from_abi.py holds in full"""
    cap = 5000
    ctx, fq, fs = burst2(cap, cap, asset_q=effects.firework_trails(cap))   # fx has no F32X4_0; the source has
    other, oq, os_ = burst2(300, 300)
    lib = runtime.load_library()
    grid = grid_over([fq, fs], (6, 6, 6))
    radius = radius_of(grid)
    st = Stats()
    ch = [(ONE, 0, 0, 0, A.VELOCITY.id, 0, SET), (A.POSITION.id, 0, DIFF, 16, A.VELOCITY.id, 1, ADD)]
    good = lambda: runtime.neighbour_desc(grid.dims, grid.origin, grid.inv_cell, radius, ch, W_U3, 4096, 1.0, st.ptr())
    ctx.synchronize(); other.synchronize()
    before = (planes(fq, TRAIL), planes(fs, ATTRS4), planes(oq, ATTRS4))

    def refused(a, b, desc, *texts):
        assert lib.hnb_effect_neighbours_from(a, b, C.byref(desc)) == -1, texts
        err = lib.hnb_last_error()
        assert err and all(t.encode() in err for t in texts), (texts, err)

    for a, b, d in ((None, fs._h, C.byref(good())), (fq._h, None, C.byref(good())), (fq._h, fs._h, None)):
        assert lib.hnb_effect_neighbours_from(a, b, d) == -1 and b"NULL" in lib.hnb_last_error()
    refused(fq._h, fq._h, good(), "fx and source are one effect", "hnb_effect_neighbours'")
    refused(fs._h, fs._h, good(), "hnb_effect_neighbours'")
    refused(fq._h, oq._h, good(), "different contexts")
    refused(oq._h, fs._h, good(), "different contexts")
    x = good(); x.channels[1].src_attr = A.F32X4_0.id; x.channels[1].src_comp = 3
    refused(fq._h, fs._h, x, "channels[1]", "HNB_NEIGHBOUR_DIFF of an attribute that is not an f32 attribute of fx's particle layout")
    x.channels[1].flags = 0                                                # ... which without DIFF is a source like any other
    assert lib.hnb_effect_neighbours_from(fs._h, fq._h, C.byref(x)) == -1 and b"source's particle layout" in lib.hnb_last_error()    # (the other way round the SOURCE lacks it)
    x = good(); x.channels[0].dst_attr = A.F32X4_0.id
    refused(fq._h, fs._h, x, "channels[0]", "fx's particle layout")
    x = good(); x.out_stats = st.ptr() + 4
    refused(fq._h, fs._h, x, "out_stats: NULL or")
    x = good(); x.struct_size = 196
    refused(fq._h, fs._h, x, "struct_size")
    x = good(); x.radius = 1.01 * radius
    refused(fq._h, fs._h, x, "radius * inv_cell is above 1")
    x = good(); x.candidate_limit = 0
    refused(fq._h, fs._h, x, "candidate_limit is not 1..")
    x = good(); x.channels[1].dst_comp = 0
    refused(fq._h, fs._h, x, "an earlier channel's")
    ctx.synchronize(); other.synchronize()
    assert st.untouched()
    for fx, attrs, b in ((fq, TRAIL, before[0]), (fs, ATTRS4, before[1]), (oq, ATTRS4, before[2])):
        after = planes(fx, attrs)
        for a in b:
            np.testing.assert_array_equal(after[a], b[a])
    x = good(); x.channels[1].src_attr = A.F32X4_0.id; x.channels[1].src_comp = 3; x.channels[1].flags = 0     # a source attribute fx lacks is fine without DIFF
    assert lib.hnb_effect_neighbours_from(fq._h, fs._h, C.byref(x)) == 0, lib.hnb_last_error()
    ctx.synchronize()
    check(ctx, fq, fs, grid, radius, "a good call behind the refusals", channels=ch, attrs_q=TRAIL)      # ... and the same effects take a good call
    fq.neighbours_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, ch)                           # out_stats may be NULL
    ctx.synchronize()
    ctx.close(); other.close()
