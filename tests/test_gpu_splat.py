"""hnb_effect_splat / hnb_program_splat on the GPU (include/hanabi_amd_splat.h): the deposit through the sample's trilinear stencil. The expectation is
always the numpy restatement (tests/test_splat_abi.py np_splat) over the host's read-back of the planes and the alive bytes, compared as integers: there
is no tolerance anywhere. Every destination is test_gpu_deposit's Dst - torch tensors pre-filled with a sentinel, with guard words on both sides. Both
kernels run every case: a grid padded with empty layers along +z until its table is past the LDS budget takes k_splat_global (the stencil reaches into
the first added layer, so the padded grid has an expectation of its own, on its own dims). The plan's restatement (splat_plan) states which kernel a
case ran."""
import ctypes as C

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A
from test_bounds_abi import trails_vec4
from test_deposit_abi import LDS_BUDGET, TILE, np_deposit, np_quantise, table_bytes
from test_gpu_deposit import HALF, Dst, add_grids, alive_mask, assert_grid, box, guard_conditions, padded, plant
from test_gpu_deposit import expected as deposit_expected
from test_gpu_deposit import run as run_deposit
from test_gpu_export import step
from test_gpu_export_sorted import make
import test_gpu_program_export_sorted as pes
from test_splat_abi import ONE, np_splat, np_splat_parts, one_source, splat_plan

pytestmark = pytest.mark.gpu

F32 = np.float32
CAPS = (255, 300, 4096, 4097, 3 * 4096 + 5)
# trails_vec4's layout: the weights themselves, a component of a 3-vector, the last of a 4-vector, a scalar
CH4 = [(ONE, 0, 30), (A.VELOCITY.id, 1, 16), (A.F32X4_0.id, 3, 8), (A.LIFETIME.id, 0, 32)]


def run(target, d, accumulate=False):
    target.splat(accumulate=accumulate, **d.args())
    return d


def plan(d, capacity, program=False, n_inst=1):
    return splat_plan(program, n_inst, capacity, d.n_cells, len(d.channels))


def read_state(fx, channels):
    """-> (positions [capacity, 3], alive [capacity], sources: per channel the stored words; 1.0f for HNB_SPLAT_ATTR_ONE) (synchronises)"""
    sources = [one_source(fx.capacity) if a == ONE else fx.read_attr(a).view(np.uint32).reshape(fx.capacity, -1)[:, c] for a, c, _ in channels]
    return fx.read_attr(A.POSITION.id).reshape(-1, 3), alive_mask(fx), sources


def expected(fx, d):
    """the restatement over the host's read-back of the same effect (synchronises; read_attr materialises stale planes for itself)"""
    pos, alive, sources = read_state(fx, d.channels)
    return np_splat(pos, alive, d.dims, d.origin, d.inv_cell, sources, [s for _, _, s in d.channels])


def splat_guard_conditions(fx, d, want):
    """On the restatement alone, for a 4^3 case: a grid of zeros, of counts without sums or of the nearest deposit can never pass"""
    guard_conditions(want, len(d.channels))                                # half of the cells occupied, the outside bin, a rejection, a negative sum
    pos, alive, sources = read_state(fx, d.channels)
    _, inside, _, _, clamped = np_splat_parts(pos[alive], d.dims, d.origin, d.inv_cell)
    assert clamped.sum() * 4 >= inside.sum() and (~clamped).sum() * 4 >= inside.sum(), "a quarter of the inside particles with a clamped corner, a quarter with none"
    nearest = np_deposit(pos, alive, d.dims, d.origin, d.inv_cell, sources, [s for _, _, s in d.channels])
    occupied = want[0][:-1] != 0
    for k in range(len(d.channels)):
        assert (want[1][:-1, k] != nearest[1][:-1, k])[occupied].sum() * 2 > occupied.sum(), f"channel {k}: the splat differs from the nearest deposit in most occupied cells"
    np.testing.assert_array_equal(want[0], nearest[0])                     # the count is the deposit's, and so is the outside row
    np.testing.assert_array_equal(want[1][-1], nearest[1][-1])


def both_paths(fx, channels, dims=(4, 4, 4), **grid):
    """one call into the grid itself (its table fits LDS) and one into the grid padded along +z (it does not)"""
    d = run(fx, Dst(dims, channels, **grid))
    p = run(fx, padded(d))
    assert plan(d, fx.capacity)[0] == "k_splat_lds" and plan(p, fx.capacity)[:2] == ("k_splat_global", -(-fx.capacity // TILE))
    return d, p


# ---- capacities: dead slots interleaved, the tail quad, whole-dead quads; both kernels -------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_capacities_all_alive_and_after_a_die_off(cap):
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    for state in ("all alive", "after a die-off"):
        if state == "after a die-off":
            fx.write_attr(A.VELOCITY.id, np.zeros((cap, 3), F32))          # (the planted NaNs and infinities do not go through the update)
            for f in range(1, 5):                                          # lifetimes are 0.8 .. 1.2 s: a second later part of the burst is gone
                step(ctx, fx, f, 0, dt=0.25)
        plant(fx, cap)
        d, p = both_paths(fx, CH4)                                         # enqueued behind the frames and the writes: nothing synchronises in front
        near = run_deposit(fx, Dst((4, 4, 4), CH4[1:]))                    # hnb_effect_deposit of the same channels but ONE, which it refuses
        ctx.synchronize()
        want = expected(fx, d)
        n = fx.alive_count()
        assert want[2][0] == n and (n == cap if state == "all alive" else 0 < n < cap), (state, n)
        splat_guard_conditions(fx, d, want)
        assert_grid(d, want, f"capacity {cap}, {state}, in LDS")
        assert_grid(p, expected(fx, p), f"capacity {cap}, {state}, in memory")
        # what needs no restatement: the count is hnb_effect_deposit's bit for bit, and so is the outside row of the sums
        got, ref = d.read(), near.read()
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[1][-1, 1:], ref[1][-1])
        assert got[1][-1, 0] == int(got[0][-1]) << 30 and (got[1][:-1, 1:] != ref[1][:-1]).any()
        np.testing.assert_array_equal(p.read()[0][:64], got[0][:64])
        inside = int(n - got[0][-1])                                        # the weights of a particle sum to 1 within their own rounding: the mass is the inside count
        assert abs(int(got[1][:-1, 0].sum()) - (inside << 30)) <= inside << 8
    assert fx.check()["ok"] == 1
    ctx.close()


def test_lds_path_over_several_groups_with_a_span_of_several_tiles_and_a_partial_last_one():
    cap = 24 * TILE + 77
    d = Dst((8, 8, 8), CH4)
    kernel, groups, _, span, lds = plan(d, cap)[:5]
    tiles = -(-cap // TILE)
    assert kernel == "k_splat_lds" and groups >= 2 and span >= 2 and tiles % span != 0 and lds == table_bytes(512, 4), (kernel, groups, span)
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    for f in range(1, 5):
        step(ctx, fx, f, 0, dt=0.25)
    plant(fx, 5)
    run(fx, d)
    ctx.synchronize()
    want = expected(fx, d)
    assert 0 < want[2][0] < cap
    guard_conditions(want, 4)
    assert_grid(d, want, f"{groups} groups of {span} tiles over {tiles}")
    ctx.close()


# ---- grids: an axis of one cell, odd dims, no channel ------------------------------------------------------------------------------------------------
GRIDS = [((1, 1, 1), CH4), ((2, 3, 5), CH4), ((4, 4, 1), CH4), ((4, 4, 4), ()), ((64, 1, 64), CH4)]


@pytest.mark.parametrize("dims,channels", GRIDS, ids=["x".join(str(i) for i in g[0]) + f"-{len(g[1])}ch" for g in GRIDS])
def test_grids_on_both_paths(dims, channels):
    cap = 4097
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    plant(fx, dims[0] * dims[1] * dims[2])
    d = run(fx, Dst(dims, channels))
    lds = table_bytes(d.n_cells, len(channels)) <= LDS_BUDGET
    assert plan(d, cap)[0] == ("k_splat_lds" if lds else "k_splat_global") and lds == (dims != (64, 1, 64))
    p = run(fx, padded(d)) if lds else None                                # (64 x 1 x 64 is past the budget as it is: an axis of one cell in memory)
    ctx.synchronize()
    want = expected(fx, d)
    assert want[2][0] == cap and 0 < want[2][1] < cap and (not channels or (want[2][2] > 0 and (want[1] < 0).any()))
    if 1 in dims and channels:                                             # an axis of one cell: both of its corners are cell 0, every inside particle is clamped
        pos, alive, _ = read_state(fx, channels)
        _, inside, _, _, clamped = np_splat_parts(pos[alive], d.dims, d.origin, d.inv_cell)
        assert inside.any() and clamped.all()
    assert_grid(d, want, f"{dims}, {len(channels)} channels, {plan(d, cap)[0]}")
    if p is not None:
        assert plan(p, cap)[0] == "k_splat_global"
        assert_grid(p, expected(fx, p), f"{dims} padded to {p.dims}, {len(channels)} channels, in memory")
    if dims == (1, 1, 1):
        count, sums, _ = d.read()
        assert int(count[0]) + int(count[1]) == cap and count[0] > 0 and count[1] > 0 and sums[1, 0] == int(count[1]) << 30
    ctx.close()


def test_contention_every_particle_at_one_point_eight_hot_rows():
    cap = 10_000
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    fx.write_attr(A.POSITION.id, np.tile(np.array([1.0, -3.0, 5.0], F32), (cap, 1)))
    fx.write_attr(A.VELOCITY.id, np.tile(np.array([1.5, -2.25, 0.0], F32), (cap, 1)))
    ch = [(ONE, 0, 6), (A.VELOCITY.id, 1, 8)]
    d, p = both_paths(fx, ch)
    ctx.synchronize()
    # t = (p + 8) / 4 = (2.25, 1.25, 3.25): u = (1.75, 0.75, 2.75), cells (1..2, 0..1, 2..3), weights (1/4, 3/4) on every axis, all exact
    want = expected(fx, d)
    rows = [(z * 4 + y) * 4 + x for z in (2, 3) for y in (0, 1) for x in (1, 2)]
    w = [wz * wy * wx for wz in (1, 3) for wy in (1, 3) for wx in (1, 3)]                   # in 64ths
    assert sorted(np.flatnonzero(want[1][:, 0])) == rows and want[1][rows, 0].tolist() == [x * cap for x in w]
    assert want[1][rows, 1].tolist() == [-9 * x * cap for x in w] and want[0][(3 * 4 + 1) * 4 + 2] == cap and list(want[2]) == [cap, 0, 0, 0]
    assert_grid(d, want, "one point, in LDS")
    assert_grid(p, expected(fx, p), "one point, in memory")
    ctx.close()


# ---- edge values ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["k_splat_lds", "k_splat_global"])
def test_edge_values_in_alive_slots(path):
    cap = 300
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    rng = np.random.default_rng(3)
    pos = rng.uniform(-HALF, 0.999 * HALF, (cap, 3)).astype(F32)
    vel = rng.normal(0, 30, (cap, 3)).astype(F32)
    down = lambda x: np.nextafter(F32(x), F32(-100))
    up = lambda x: np.nextafter(F32(x), F32(100))
    pos[0] = (np.nan, 0, 0); pos[1] = (0, np.inf, 0); pos[2] = (0, 0, -np.inf)           # outside
    pos[3] = (-HALF, -0.0, -HALF)                                                         # the lowest corner: inside, clamped on two axes
    pos[4] = (-HALF + 4.0, 0, 0); pos[5] = (down(-HALF + 4.0), 0, 0); pos[6] = (up(-HALF + 4.0), 0, 0)     # on a cell face, one ulp either side
    pos[7] = (down(-HALF), 0, 0)                                                          # one ulp outside
    pos[8] = (0, 0, -0.0)
    pos[9] = (-HALF + 2.0, -HALF + 6.0, -HALF + 14.0)                                     # a cell centre on all three axes: everything in its own cell
    pos[10] = (down(-HALF + 2.0), 2.0, 2.0)                                               # t one ulp below 0.5: u is a tiny negative number, w1 rounds to 1.0
    pos[11] = (-HALF + 2.0, down(-HALF + 2.0), up(-HALF + 14.0))                          # ... and on y; z one ulp past the last centre
    vals = [np.nan, np.inf, -np.inf, -0.0, 1e-45, -1e-40, 1.1754942e-38, 2.0 ** -33, 2.0 ** -100, 0.5, 1.5, 2.5, -0.5, -1.5, -3.5, 2.0 ** 62 * (1 - 2.0 ** -24), 2.0 ** 62, -(2.0 ** 62),
            2.0 ** 61, -(2.0 ** 61), 2.0 ** 29, 2.0 ** 30, 3e38]
    vel[12:12 + len(vals), 0] = np.array(vals, F32)
    vel[3:12, 0] = np.array([2.0 ** 61, -1.5, 2.5, 0.5, 7.0, 1.5, -(2.0 ** 61), 2.0 ** 62 * (1 - 2.0 ** -24), 3.5], F32)      # the edge positions carry edge values too
    wrap = slice(40, 44)                                                   # four values of 2^61 on the last cell's centre: its sum wraps past 2^63
    pos[(pos[:, 0] >= 2.0) & (pos[:, 1] >= 2.0) & (pos[:, 2] >= 2.0)] = (0, 0, 0)          # (t >= 2.5 on every axis: nothing else has a corner in the last cell)
    pos[wrap] = (6.0, 6.0, 6.0)
    vel[wrap, 0] = F32(2.0 ** 61)
    fx.write_attr(A.POSITION.id, pos)
    fx.write_attr(A.VELOCITY.id, vel)
    ch = [(A.VELOCITY.id, 0, 0), (A.VELOCITY.id, 0, 1), (A.VELOCITY.id, 0, 32), (A.POSITION.id, 0, 20)]
    d = Dst((4, 4, 4), ch)
    if path == "k_splat_global":
        d = padded(d)
    assert plan(d, cap)[0] == path
    run(fx, d)
    ctx.synchronize()
    want = expected(fx, d)
    count, sums, stats = want
    assert count[-1] == 4 and stats[1] == 4                                # the NaN, the two infinities, the ulp below the origin
    assert stats[2] >= 3 * 3 + 2 * 2 + 1 + 1                               # NaN and infinities in three channels; 2^62 at every frac_bits; 3e38; the NaN position in its own channel
    # 4 * 2^61 wraps to -2^63; at frac_bits 1 and 32 each of the four is at or above 2^62: rejected. (Padded, the centre has a layer above it: w1 = 0 adds 0 there.)
    assert sums[63].tolist()[:3] == [-2 ** 63, 0, 0] and count[63] == 4
    assert (sums < 0).any() and (sums > 0).any()
    ok, _ = np_quantise(np.array(vals, F32).view(np.uint32), 0)
    assert list(ok) == [False] * 3 + [True] * 13 + [False] * 2 + [True] * 4 + [False]
    assert_grid(d, want, f"edge values, {path}")
    ctx.close()


# ---- accumulate, NULL stats, nothing alive ----------------------------------------------------------------------------------------------------------
def test_accumulate_adds_onto_a_deposit_and_a_call_without_the_flag_overwrites():
    cap = 5000
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    plant(fx, 1)
    ch = CH4[1:]                                                           # (hnb_effect_deposit refuses HNB_SPLAT_ATTR_ONE: the shared grid holds the three others)
    for dims in ((4, 4, 4), (32, 32, 32)):
        d = Dst(dims, ch)
        assert plan(d, cap)[0] == ("k_splat_lds" if dims[0] == 4 else "k_splat_global")
        run_deposit(fx, d)                                                 # hnb_effect_deposit, then hnb_effect_splat with the flag onto the SAME tensors
        run(fx, d, accumulate=True)
        twice = run(fx, Dst(dims, ch))
        run(fx, twice, accumulate=True)
        ctx.synchronize()
        wd, ws = deposit_expected(fx, d), expected(fx, d)
        assert wd[2][0] == cap and ws[2][2] > 0 and (wd[1] != ws[1]).any()
        assert_grid(d, add_grids(wd, ws), f"{dims}: a deposit and a splat in one grid")
        assert_grid(twice, add_grids(ws, ws), f"{dims}: two splats in one grid")
        run(fx, d)                                                         # without the flag: what was there is overwritten
        ctx.synchronize()
        assert_grid(d, ws, f"{dims}: overwritten")
    ctx.close()


def test_out_stats_null_is_accepted():
    cap = 4097
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    plant(fx, 9)
    d = run(fx, Dst((4, 4, 4), CH4, stats=False))
    wide = padded(Dst((4, 4, 4), CH4))
    p = run(fx, Dst(wide.dims, CH4, stats=False, origin=wide.origin, inv_cell=wide.inv_cell))
    ctx.synchronize()
    assert plan(d, cap)[0] == "k_splat_lds" and plan(p, cap)[0] == "k_splat_global"
    assert_grid(d, expected(fx, d), "no out_stats, in LDS")
    assert_grid(p, expected(fx, p), "no out_stats, in memory")
    ctx.close()


@pytest.mark.parametrize("cap", [300, 10_000])
def test_nothing_alive_leaves_zeros_and_clears_planted_garbage(cap):
    ctx, fx = make(cap, trails_vec4(cap))
    grids = lambda: [Dst((4, 4, 4), CH4), padded(Dst((4, 4, 4), CH4)), Dst((2, 3, 5), ())]
    zero = lambda d: (np.zeros(d.n_cells + 1, np.uint32), np.zeros((d.n_cells + 1, len(d.channels)), np.int64), np.zeros(4, np.uint32))
    before = [run(fx, d) for d in grids()]                                 # before the first frame; every destination is the sentinel all over
    step(ctx, fx, 0, cap)
    for f in range(1, 5):
        step(ctx, fx, f, 0, dt=0.5)                                        # every lifetime is over
    after = [run(fx, d) for d in grids()]
    acc = run(fx, Dst((4, 4, 4), CH4), accumulate=True)                    # ... and with the flag nothing is added, so nothing is written
    ctx.synchronize()
    assert fx.alive_count() == 0
    for d in before + after:
        assert_grid(d, zero(d), "nothing alive")
    assert acc.untouched()
    ctx.close()


# ---- program form ---------------------------------------------------------------------------------------------------------------------------------
def check_program(ctx, prog, fxs, dsts, what):
    """the program call in FRONT of the per-effect ones, then: the program's grid == the effect form accumulated over the instances == the sum of the
    restatements, stats included. -> the expected grid of the first destination"""
    cap = fxs[0].capacity
    wants = []
    for make_dst in dsts:
        d, acc = run(prog, make_dst()), make_dst()
        for k, fx in enumerate(fxs):
            run(fx, acc, accumulate=k > 0)
        ctx.synchronize()
        assert plan(d, cap, True, len(fxs))[2] == len(fxs)
        want = None
        for fx in fxs:
            w = expected(fx, d)
            want = w if want is None else add_grids(want, w)
        assert_grid(acc, want, f"{what}: the effect form, accumulated")
        assert_grid(d, want, f"{what}: the program form, {plan(d, cap, True, len(fxs))[0]}")
        wants.append(want)
    return wants[0]


@pytest.mark.parametrize("cap", [300, 4097])
def test_program_of_five_instances_one_empty_one_frozen(cap):
    n = 5
    ctx, prog, fxs = pes.make(cap, n, asset=trails_vec4(cap))
    spawns = [cap, 0, cap // 3, 37, cap - 1]
    pes.step(ctx, fxs, 0, spawns)
    pes.step(ctx, fxs, 1, [0] * n, dt=1 / 60)
    for k, fx in enumerate(fxs):
        plant(fx, 100 + k)
    dsts = (lambda: Dst((4, 4, 4), CH4), lambda: padded(Dst((4, 4, 4), CH4)))
    want = check_program(ctx, prog, fxs, dsts, f"capacity {cap}, burst")
    assert want[2][0] == sum(spawns)
    guard_conditions(want, 4)
    fxs[2].set_simulated(False)
    for f in (2, 3, 4):
        pes.step(ctx, fxs, f, [0] * n, dt=0.3)
    frozen = expected(fxs[2], Dst((4, 4, 4), CH4))
    assert frozen[2][0] == cap // 3                                        # the frozen instance splats the state it was frozen in
    want = check_program(ctx, prog, fxs, dsts, f"capacity {cap}, die-off")
    assert cap // 3 < want[2][0] < sum(spawns)
    ctx.close()


# ---- stale AGE --------------------------------------------------------------------------------------------------------------------------------------
def test_stale_age_is_materialised_first_and_nothing_later_changes():
    """LEAN cohorts: the AGE plane is stale until something materialises it; a channel on AGE does. A twin context that never calls ends bit-identical."""
    cap = 100_000
    pairs = [make(cap, age_cohort=1) for _ in range(2)]
    (ctx, fx), (tctx, twin) = pairs
    assert fx.device_view().stale_attr_mask == 1 << A.AGE.id
    ch = [(A.AGE.id, 0, 32), (ONE, 0, 30)]
    b = box(2.0, 6.0)                                                        # the burst is a shell of radius up to 5: outside along x and y
    keep = []
    for f in range(5):
        for c, e in pairs:
            step(c, e, f, 70_000 if f == 0 else 3000, dt=1 / 60)
        if f >= 3:                                                         # no materialise call in front of them
            keep.append((run(fx, Dst((4, 4, 4), ch, **b)), run(fx, padded(Dst((4, 4, 4), ch, **b)))))
    ctx.synchronize()
    d, p = keep[-1]
    want = expected(fx, d)                                                 # (the read-back materialises for itself - behind the calls above)
    dt = F32(1 / 60)
    ages = fx.read_attr(A.AGE.id).reshape(-1)[alive_mask(fx)]
    assert want[2][0] == 70_000 + 4 * 3000 and ages.min() == dt and ages.max() > F32(4.5) * dt and want[1][:, 0].sum() > 70_000 * 4 * (2 ** 32 // 60) * 0.99
    assert want[2][1] > 0 and (want[0][:-1] > 0).sum() > 16
    assert_grid(d, want, "stale AGE, in LDS")
    assert_grid(p, expected(fx, p), "stale AGE, in memory")
    assert keep[0][0].read()[2][0] == 70_000 + 3 * 3000
    for f in range(5, 12):
        for c, e in pairs:
            step(c, e, f, 0, dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    diff = fx.compare(twin)
    assert diff["equal"] == 1, diff
    assert fx.check()["ok"] == 1
    ctx.close(); tctx.close()


# ---- in the stream, next to the frames, a deposit and a sample -----------------------------------------------------------------------------------------
def test_calls_interleaved_with_frames_a_deposit_and_a_sample_without_a_synchronisation():
    """Six program calls and six effect calls into twelve destinations, a frame between two of them, a deposit and a sample (which changes VELOCITY) in
    between, and no synchronisation of the context until the end. The expected grids of call i come from a replica context that runs the same frames
    and the same sample calls and is read back after each; hnb_effect_compare proves at the end that the replica is the calling context's state."""
    cap, n = 10_000, 2
    (ctx, prog, fxs), (rctx, rprog, rfxs) = pes.make(cap, n), pes.make(cap, n)
    ch = [(A.VELOCITY.id, 0, 12), (ONE, 0, 30), (A.AGE.id, 0, 32)]
    b = box(3.0, 16.0)                                                       # (drag 4 on 60 units a second: nothing travels 16 units)
    field = torch.from_numpy(np.random.default_rng(8).normal(0, 5, 64).astype(F32)).cuda()
    torch.cuda.synchronize()
    sample = dict(dims=(4, 4, 4), origin=b["origin"], inv_cell=b["inv_cell"], field_ptr=field.data_ptr(), channels=[(A.VELOCITY.id, 0, runtime.SAMPLE_ADD)], scale=0.5)
    calls, want, others = [], [], []                                        # (others: their destinations stay allocated until the stream has run them)
    for f in range(6):
        spawns = [cap if f == 0 else 0, 50 * f]
        for c, e in ((ctx, fxs), (rctx, rfxs)):
            pes.step(c, e, f, spawns, dt=1 / 600 if f == 0 else 0.2)               # (lifetimes are 0.8 .. 1.2 s: the last frames lose part of the burst)
            e[0].sample(**sample)
        calls.append((run(prog, Dst((4, 4, 4), ch, **b)), run(fxs[1], padded(Dst((4, 4, 4), ch[:1], **b)))))
        others.append(run_deposit(fxs[0], Dst((4, 4, 4), ch[:1], **b)))
        rctx.synchronize()
        wp = add_grids(expected(rfxs[0], calls[-1][0]), expected(rfxs[1], calls[-1][0]))
        want.append((wp, expected(rfxs[1], calls[-1][1]), deposit_expected(rfxs[0], others[-1])))
    ctx.synchronize()
    for f, ((dp, de), (wp, we, wd)) in enumerate(zip(calls, want)):
        assert_grid(dp, wp, f"program call behind frame {f}")
        assert_grid(de, we, f"effect call behind frame {f}")
        assert_grid(others[f], wd, f"the deposit behind frame {f}")
    assert 0 < want[-1][0][2][0] < cap + 50 * 15 and want[-1][1][2][0] > 0   # the burst is dying off, the trickle is alive
    assert (want[3][0][0][:-1] > 0).sum() > 8 and (want[3][0][1] < 0).any()
    for a, r in zip(fxs, rfxs):
        assert a.compare(r)["equal"] == 1
    ctx.close(); rctx.close()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    """Every refusal of the contract but two: more than 65535 instances, which no test here creates, and a layout without POSITION, which the
    stand-alone program of tests/test_splat_abi.py holds. hnb_effect_deposit keeps refusing HNB_SPLAT_ATTR_ONE."""
    cap = 5000
    ctx, prog, fxs = pes.make(cap, 2)
    pes.step(ctx, fxs, 0, [cap, 100])
    empty_prog = ctx.create_program(bh.lower(effects.firework_trails(300)))
    fx = fxs[0]
    lib = runtime.load_library()
    d = Dst((4, 4, 4), [(A.VELOCITY.id, 1, 16), (ONE, 0, 30)])
    good = lambda: runtime.deposit_desc(**d.args())
    nan, inf = float("nan"), float("inf")

    def refused(call, handle, desc, text):
        assert call(handle, C.byref(desc)) == -1, text
        assert text.encode() in lib.hnb_last_error(), (text, lib.hnb_last_error())

    for call, handle in ((lib.hnb_effect_splat, fx._h), (lib.hnb_program_splat, prog._h)):
        x = good(); x.struct_size = 132
        refused(call, handle, x, "struct_size")
        x = good(); x.flags = 2
        refused(call, handle, x, "flags")
        for dims in ((0, 4, 4), (4096, 4096, 2)):
            x = good(); x.dims = (C.c_uint32 * 3)(*dims)
            refused(call, handle, x, "HNB_BIN_MAX_CELLS")
        x = good(); x.origin[1] = nan
        refused(call, handle, x, "origin is not finite")
        for bad in (0.0, -1.0, inf, nan):
            x = good(); x.inv_cell[2] = bad
            refused(call, handle, x, "inv_cell is not finite and above 0")
        x = good(); x.n_channels = 5
        refused(call, handle, x, "n_channels is above")
        for attr in (A.COLOR.id, A.SIZE3.id, A.ID.id, 9999, ONE - 1):       # packed u32; not in the layout; not stored; no attribute
            x = good(); x.channels[0].attr = attr
            refused(call, handle, x, "channels[0]")
            assert b"not HNB_SPLAT_ATTR_ONE or an f32 attribute" in lib.hnb_last_error()
        x = good(); x.channels[0].comp = 3
        refused(call, handle, x, "comp is at or past")
        for comp in (1, 3):
            x = good(); x.channels[1].comp = comp
            refused(call, handle, x, "HNB_SPLAT_ATTR_ONE and its comp is not 0")
        x = good(); x.channels[1].frac_bits = 33
        refused(call, handle, x, "frac_bits is above 32")
        x = good(); x.channels[1].reserved = 1
        refused(call, handle, x, "reserved is not 0")
        x = good(); x.channels[3].frac_bits = 1
        refused(call, handle, x, "at or past n_channels")
        x = good(); x.channels[2].attr = ONE
        refused(call, handle, x, "at or past n_channels")
        x = good(); x.count = None
        refused(call, handle, x, "count: a 16-byte aligned")
        x = good(); x.count = d.count.data_ptr() + 4
        refused(call, handle, x, "count: a 16-byte aligned")
        x = good(); x.sums = None
        refused(call, handle, x, "sums: a 16-byte aligned")
        x = good(); x.sums = d.sums.data_ptr() + 8
        refused(call, handle, x, "sums: a 16-byte aligned")
        x = good(); x.n_channels = 0; x.channels[0] = runtime.DepositChannel(); x.channels[1] = runtime.DepositChannel()
        refused(call, handle, x, "NULL without")
        x = good(); x.out_stats = d.stats.data_ptr() + 4
        refused(call, handle, x, "out_stats: NULL or")
    refused(lib.hnb_program_splat, empty_prog._h, good(), "0 instances")
    for call, handle in ((lib.hnb_effect_deposit, fx._h), (lib.hnb_program_deposit, prog._h)):      # the deposit has no such channel, and no flag for the stencil
        refused(call, handle, good(), "channels[1]")
        x = good(); x.channels[1] = runtime.DepositChannel(A.VELOCITY.id, 0, 0, 0); x.flags = 2
        refused(call, handle, x, "flags")
    ctx.synchronize()
    assert d.untouched()
    run(prog, d)                                                           # ... and the same destination takes a good call
    ctx.synchronize()
    assert_grid(d, add_grids(expected(fxs[0], d), expected(fxs[1], d)), "a good call behind the refusals")
    ctx.close()
