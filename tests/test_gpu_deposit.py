"""hnb_effect_deposit / hnb_program_deposit on the GPU (include/hanabi_amd_deposit.h): the alive particles summed into a dense uniform grid - a count
per cell and fixed-point sums of up to four f32 components. The expectation is always the numpy restatement (tests/test_deposit_abi.py np_deposit)
over the host's read-back of the planes and the alive bytes, compared as integers: there is no tolerance anywhere. Every destination is a torch
tensor pre-filled with a sentinel with guard words on both sides: a call without HNB_DEPOSIT_ACCUMULATE must clear what it defines and touch nothing
else. The shapes come from the plan's restatement (deposit_plan), so that every case states which of the two kernels it ran."""
import ctypes as C

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A
from test_bounds_abi import trails_vec4
from test_deposit_abi import LDS_BUDGET, TILE, deposit_plan, last_lds_cells, np_deposit, np_quantise, table_bytes
from test_gpu_bounds import run as run_bounds
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, step
from test_gpu_export_binned import Grid as BinGrid, run_binned
from test_gpu_export_sorted import make
import test_gpu_program_export_sorted as pes

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL64 = 0x5EA7BEEF5EA7BEEF
GUARD = 4                                        # words (count, stats) / half as many i64 (sums) on both sides: 16 bytes, the alignment stays
HALF = 8.0                                       # the grids span [-HALF, HALF)^3
CAPS = (255, 300, 4096, 4097, 3 * 4096 + 5, 300_007)
# trails_vec4's layout: a component of a 3-vector, the last of a 4-vector, a scalar, POSITION itself
CH4 = [(A.VELOCITY.id, 1, 16), (A.F32X4_0.id, 3, 8), (A.LIFETIME.id, 0, 32), (A.POSITION.id, 2, 0)]


class Dst:
    """The destination of one call: count, sums and stats between guard words, everything the sentinel"""

    def __init__(self, dims, channels=(), stats=True, origin=(-HALF,) * 3, inv_cell=None):
        self.dims = tuple(int(d) for d in dims)
        self.n_cells = self.dims[0] * self.dims[1] * self.dims[2]
        self.origin = np.asarray(origin, F32)
        self.inv_cell = np.asarray(inv_cell if inv_cell is not None else [d / (2 * HALF) for d in self.dims], F32)
        self.channels = [tuple(int(x) for x in c) for c in channels]
        k, n = len(self.channels), self.n_cells + 1
        self.count = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.sums = torch.full((n * k + GUARD,), SENTINEL64, dtype=torch.int64, device="cuda") if k else None
        self.stats = torch.full((4 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda") if stats else None
        torch.cuda.synchronize()                 # (the fills run on torch's stream, the call on the simulation's)

    def args(self):
        return dict(dims=self.dims, origin=self.origin, inv_cell=self.inv_cell, count_ptr=self.count.data_ptr() + 4 * GUARD, channels=self.channels,
                    sums_ptr=self.sums.data_ptr() + 4 * GUARD if self.sums is not None else None, stats_ptr=self.stats.data_ptr() + 4 * GUARD if self.stats is not None else None)

    def plan(self, capacity, program=False, n_inst=1):
        return deposit_plan(program, n_inst, capacity, self.n_cells, len(self.channels))

    def read(self):
        """-> (count, sums, stats or None), and asserts the guard words on both sides of each"""
        k, n = len(self.channels), self.n_cells + 1
        c = self.count.cpu().numpy().view(np.uint32)
        assert (c[:GUARD] == SENTINEL).all() and (c[GUARD + n:] == SENTINEL).all(), "words next to count were written"
        s = np.zeros((n, 0), np.int64)
        if k:
            raw = self.sums.cpu().numpy()
            assert (raw[: GUARD // 2] == SENTINEL64).all() and (raw[GUARD // 2 + n * k:] == SENTINEL64).all(), "words next to sums were written"
            s = raw[GUARD // 2: GUARD // 2 + n * k].reshape(n, k)
        st = None
        if self.stats is not None:
            raw = self.stats.cpu().numpy().view(np.uint32)
            assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + 4:] == SENTINEL).all(), "words next to out_stats were written"
            st = raw[GUARD: GUARD + 4]
        return c[GUARD: GUARD + n], s, st

    def untouched(self):
        return all(bool((t.cpu().numpy().view(np.uint32) == SENTINEL).all()) for t in (self.count, self.sums, self.stats) if t is not None)


def run(target, d, accumulate=False):
    target.deposit(accumulate=accumulate, **d.args())
    return d


def alive_mask(fx):
    m = np.zeros(fx.capacity, bool)
    m[fx.alive_list()] = True
    return m


def expected(fx, d):
    """the restatement over the host's read-back of the same effect (synchronises; read_attr materialises stale planes for itself)"""
    sources = [fx.read_attr(a).view(np.uint32).reshape(fx.capacity, -1)[:, c] for a, c, _ in d.channels]
    return np_deposit(fx.read_attr(A.POSITION.id).reshape(-1, 3), alive_mask(fx), d.dims, d.origin, d.inv_cell, sources, [s for _, _, s in d.channels])


def add_grids(a, b):
    """two results into one, as HNB_DEPOSIT_ACCUMULATE does: modulo 2^32 and 2^64"""
    return a[0] + b[0], (a[1].view(np.uint64) + b[1].view(np.uint64)).view(np.int64), a[2] + b[2]


def assert_grid(d, want, what):
    count, sums, stats = d.read()
    np.testing.assert_array_equal(count, want[0], err_msg=f"{what}: count")
    np.testing.assert_array_equal(sums, want[1], err_msg=f"{what}: sums")
    if stats is not None:
        np.testing.assert_array_equal(stats, want[2], err_msg=f"{what}: out_stats")


def guard_conditions(want, n_channels):
    """On the restatement alone: a grid of zeros, or of counts without sums, can never pass for the case"""
    count, sums, stats = want
    assert (count[:-1] != 0).sum() * 2 > len(count) - 1, "more than half of the cells are occupied"
    assert count[-1] > 0 and stats[1] == count[-1], "the outside bin is not empty"
    assert stats[0] == count.sum(dtype=np.uint64)
    if n_channels:
        assert stats[2] > 0, "a contribution is rejected"
        assert (sums < 0).any(), "a sum is negative"


def plant(fx, seed, vec4=True):
    """Values over the whole capacity, written with hnb_effect_write_attr: positions a hair wider than the grid along x, y and below it along z (never
    above: a grid padded with cells along +z keeps every cell index), sources of both signs with a NaN, an infinity and a huge value among them"""
    rng = np.random.default_rng(seed)
    cap = fx.capacity
    pos = rng.uniform(-1.05 * HALF, 1.05 * HALF, (cap, 3))
    pos[:, 2] = rng.uniform(-1.05 * HALF, 0.999 * HALF, cap)
    fx.write_attr(A.POSITION.id, pos.astype(F32))
    vel = rng.normal(0, 30, (cap, 3)).astype(F32)
    vel[rng.random(cap) < 0.02, 1] = np.nan
    vel[rng.random(cap) < 0.02, 1] = -np.inf
    vel[rng.random(cap) < 0.02, 1] = 3e38
    fx.write_attr(A.VELOCITY.id, vel)
    if vec4:
        f4 = rng.normal(0, 4, (cap, 4)).astype(F32)
        f4[rng.random(cap) < 0.02, 3] = np.nan
        fx.write_attr(A.F32X4_0.id, f4)


def box(hx, hz):
    """4^3 cells over [-hx, hx)^2 x [-hz, hz): hz is chosen beyond every particle, so that a grid padded along +z stays empty there"""
    return dict(origin=(-hx, -hx, -hz), inv_cell=(2 / hx, 2 / hx, 2 / hz))


def padded(d, channels=None):
    """The same cells - the same origin and edges - with layers of empty cells along +z until the table is past the LDS budget"""
    ch = d.channels if channels is None else channels
    layer = d.dims[0] * d.dims[1]
    nz = -(-(last_lds_cells(len(ch)) + 1) // layer)
    p = Dst((d.dims[0], d.dims[1], nz), ch, origin=d.origin, inv_cell=d.inv_cell)
    assert table_bytes(p.n_cells, len(ch)) > LDS_BUDGET >= table_bytes(p.n_cells - layer, len(ch))
    return p


def assert_padded(p, d, want, what):
    """p = padded(d): the occupied entries are d's, the outside bin moved to the end, everything between is zero"""
    n = d.n_cells
    count, sums, stats = want
    wide = (np.concatenate([count[:n], np.zeros(p.n_cells - n, np.uint32), count[n:]]),
            np.concatenate([sums[:n], np.zeros((p.n_cells - n, sums.shape[1]), np.int64), sums[n:]]), stats)
    assert_grid(p, wide, what)


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
        d = run(fx, Dst((4, 4, 4), CH4))                                   # enqueued behind the frames and the writes: nothing synchronises in front
        p = run(fx, padded(d))
        ctx.synchronize()
        assert d.plan(cap)[0] == "k_deposit_lds" and p.plan(cap)[:2] == ("k_deposit_global", -(-cap // TILE))
        want = expected(fx, d)
        n = fx.alive_count()
        assert want[2][0] == n and (n == cap if state == "all alive" else 0 < n < cap), (state, n)
        guard_conditions(want, 4)
        assert_grid(d, want, f"capacity {cap}, {state}, in LDS")
        assert_padded(p, d, want, f"capacity {cap}, {state}, in memory")
    assert fx.check()["ok"] == 1
    ctx.close()


def test_lds_path_over_several_groups_with_a_span_of_several_tiles_and_a_partial_last_one():
    cap = 24 * TILE + 77
    d = Dst((8, 8, 8), CH4)
    kernel, groups, _, span, lds = d.plan(cap)[:5]
    tiles = -(-cap // TILE)
    assert kernel == "k_deposit_lds" and groups >= 2 and span >= 2 and tiles % span != 0 and lds == table_bytes(512, 4), (kernel, groups, span)
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


# ---- grids: the path the plan names -------------------------------------------------------------------------------------------------------------------
def _dims_of(n_cells):
    """three factors of n_cells, as even as they come"""
    best = None
    for a in range(1, int(round(n_cells ** (1 / 3))) + 2):
        if n_cells % a:
            continue
        for b in range(a, int((n_cells // a) ** 0.5) + 1):
            if (n_cells // a) % b == 0:
                best = (a, b, n_cells // a // b)
    return best


GRIDS = [((1, 1, 1), CH4, "k_deposit_lds", 4096), ((4, 4, 4), CH4, "k_deposit_lds", 4097), ((4, 4, 4), (), "k_deposit_lds", 4097),
         (_dims_of(last_lds_cells(0)), (), "k_deposit_lds", 40_000), (_dims_of(last_lds_cells(0) + 1), (), "k_deposit_global", 40_000),
         (_dims_of(last_lds_cells(4)), CH4, "k_deposit_lds", 40_000), (_dims_of(last_lds_cells(4) + 1), CH4, "k_deposit_global", 40_000),
         ((64, 64, 64), CH4[:1], "k_deposit_global", 300_007)]


@pytest.mark.parametrize("dims,channels,kernel,cap", GRIDS, ids=["x".join(str(i) for i in g[0]) + f"-{len(g[1])}ch" for g in GRIDS])
def test_grids_take_the_path_the_plan_names(dims, channels, kernel, cap):
    d = Dst(dims, channels)
    assert d.plan(cap)[0] == kernel and (table_bytes(d.n_cells, len(channels)) <= LDS_BUDGET) == (kernel == "k_deposit_lds")
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    plant(fx, d.n_cells)
    run(fx, d)
    ctx.synchronize()
    want = expected(fx, d)
    guard_conditions(want, len(channels))
    assert_grid(d, want, f"{dims}, {len(channels)} channels, {kernel}")
    if dims == (1, 1, 1):
        count = d.read()[0]
        assert int(count[0]) + int(count[1]) == fx.alive_count() == cap and count[0] > 0 and count[1] > 0
    ctx.close()


def test_both_paths_agree_for_0_to_4_channels():
    cap = 10_000
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    for f in range(1, 5):
        step(ctx, fx, f, 0, dt=0.25)
    plant(fx, 77)
    pairs = []
    for k in range(5):
        d = run(fx, Dst((4, 4, 4), CH4[:k]))
        pairs.append((d, run(fx, padded(d))))
    ctx.synchronize()
    for k, (d, p) in enumerate(pairs):
        assert d.plan(cap)[0] == "k_deposit_lds" and p.plan(cap)[0] == "k_deposit_global"
        want = expected(fx, d)
        guard_conditions(want, k)
        assert_grid(d, want, f"{k} channels in LDS")
        assert_padded(p, d, want, f"{k} channels in memory")
        got_d, got_p = d.read(), p.read()
        np.testing.assert_array_equal(got_d[0][:64], got_p[0][:64])
        np.testing.assert_array_equal(got_d[1][:64], got_p[1][:64])
    ctx.close()


def test_contention_every_particle_in_one_cell():
    cap = 10_000
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    fx.write_attr(A.POSITION.id, np.tile(np.array([1.0, -3.0, 5.0], F32), (cap, 1)))
    fx.write_attr(A.VELOCITY.id, np.tile(np.array([1.5, -2.25, 0.0], F32), (cap, 1)))
    ch = [(A.VELOCITY.id, 0, 1), (A.VELOCITY.id, 1, 2)]
    d = run(fx, Dst((4, 4, 4), ch))
    p = run(fx, padded(d))
    ctx.synchronize()
    cell = (3 * 4 + 1) * 4 + 2                                             # t = (p + 8) / 4: (2.25, 1.25, 3.25)
    want = expected(fx, d)
    assert want[0][cell] == cap and want[1][cell].tolist() == [3 * cap, -9 * cap] and list(want[2]) == [cap, 0, 0, 0]
    assert_grid(d, want, "one cell, in LDS")
    assert_padded(p, d, want, "one cell, in memory")
    ctx.close()


# ---- edge values ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["k_deposit_lds", "k_deposit_global"])
def test_edge_values_in_alive_slots(path):
    cap = 300
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    rng = np.random.default_rng(3)
    pos = rng.uniform(-HALF, 0.999 * HALF, (cap, 3)).astype(F32)
    vel = rng.normal(0, 30, (cap, 3)).astype(F32)
    pos[0] = (np.nan, 0, 0); pos[1] = (0, np.inf, 0); pos[2] = (0, 0, -np.inf)           # outside
    pos[3] = (-HALF, -0.0, -HALF)                                                         # the lowest corner: inside; t = (-0 + 8) / 4 = 2
    pos[4] = (-HALF + 4.0, 0, 0); pos[5] = (np.nextafter(F32(-HALF + 4.0), F32(-100)), 0, 0)      # on a cell face: the upper cell; one ulp below: the lower
    pos[6] = (np.nextafter(F32(-HALF), F32(-100)), 0, 0)                                  # one ulp outside
    pos[7] = (0, 0, -0.0)
    vals = [np.nan, np.inf, -np.inf, -0.0, 1e-45, -1e-40, 0.5, 1.5, 2.5, -0.5, -1.5, -3.5, 2.0 ** 62 * (1 - 2.0 ** -24), 2.0 ** 62, -(2.0 ** 62), 3e38]
    vel[8:8 + len(vals), 0] = np.array(vals, F32)
    wrap = slice(40, 44)                                                   # four values of 2^61 in a cell of their own: the sum wraps past 2^63
    pos[(pos[:, 0] >= 4.0) & (pos[:, 1] >= 4.0) & (pos[:, 2] >= 4.0)] = (0, 0, 0)
    pos[wrap] = (5.0, 5.0, 5.0)
    vel[wrap, 0] = F32(2.0 ** 61)
    fx.write_attr(A.POSITION.id, pos)
    fx.write_attr(A.VELOCITY.id, vel)
    ch = [(A.VELOCITY.id, 0, 0), (A.VELOCITY.id, 0, 1), (A.VELOCITY.id, 0, 32), (A.POSITION.id, 0, 20)]
    d = Dst((4, 4, 4), ch)
    if path == "k_deposit_global":
        d = padded(d)
    assert d.plan(cap)[0] == path
    run(fx, d)
    ctx.synchronize()
    want = expected(fx, d)
    count, sums, stats = want
    assert count[-1] == 4 and stats[1] == 4                                # the NaN, the two infinities, the ulp below the origin
    assert stats[2] >= 3 * 3 + 2 * 2 + 1 + 1                               # NaN and infinities in three channels; 2^62 at every frac_bits; 3e38; the NaN position in its own channel
    assert sums[63].tolist()[:3] == [-2 ** 63, 0, 0] and count[63] == 4    # 4 * 2^61 wraps to -2^63; at frac_bits 1 and 32 each of the four is at or above 2^62: rejected
    assert (sums < 0).any() and (sums > 0).any()
    ok, q = np_quantise(np.array(vals, F32).view(np.uint32), 0)
    assert list(ok) == [False] * 3 + [True] * 10 + [False] * 3 and list(q[3:13]) == [0, 0, 0, 0, 2, 2, 0, -2, -4, 2 ** 62 - 2 ** 38]
    assert_grid(d, want, f"edge values, {path}")
    ctx.close()


# ---- accumulate, NULL stats, nothing alive ----------------------------------------------------------------------------------------------------------
def test_accumulate_adds_two_effects_of_different_programs_and_a_call_without_the_flag_overwrites():
    ctx = bh.Context(0)
    fa = ctx.create_program(bh.lower(trails_vec4(5000))).create_effect()
    fb = ctx.create_program(bh.lower(effects.firework_trails(3000))).create_effect()
    for f, (na, nb) in enumerate(((5000, 3000), (0, 0))):
        ctx.frame_begin(1 / 600, f / 600)
        fa.set_frame(na, 11 + f)
        fb.set_frame(nb, 23 + f)
        ctx.simulate()
    plant(fa, 1)
    plant(fb, 2, vec4=False)
    ch = [(A.VELOCITY.id, 1, 16), (A.LIFETIME.id, 0, 32)]
    for dims in ((4, 4, 4), (32, 32, 32)):
        d = Dst(dims, ch)
        assert d.plan(5000)[0] == ("k_deposit_lds" if dims[0] == 4 else "k_deposit_global")
        run(fa, d)
        run(fb, d, accumulate=True)
        first = Dst(dims, ch)
        run(fa, first)
        ctx.synchronize()
        wa, wb = expected(fa, d), expected(fb, d)
        assert wa[2][0] == 5000 and wb[2][0] == 3000 and wa[2][2] > 0 and wb[2][2] > 0
        assert_grid(first, wa, "the cleared first call")
        assert_grid(d, add_grids(wa, wb), f"{dims}: two effects into one grid")
        run(fb, d)                                                         # without the flag: what was there is overwritten
        ctx.synchronize()
        assert_grid(d, wb, f"{dims}: overwritten")
    ctx.close()


def test_out_stats_null_is_accepted():
    cap = 4097
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    plant(fx, 9)
    d = run(fx, Dst((4, 4, 4), CH4, stats=False))
    p = run(fx, padded(Dst((4, 4, 4), CH4)))
    p2 = Dst(p.dims, CH4, stats=False, origin=p.origin, inv_cell=p.inv_cell)
    run(fx, p2)
    ctx.synchronize()
    want = expected(fx, d)
    assert_grid(d, want, "no out_stats, in LDS")
    np.testing.assert_array_equal(p2.read()[0], p.read()[0])
    np.testing.assert_array_equal(p2.read()[1], p.read()[1])
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
        assert d.plan(cap, True, len(fxs))[2] == len(fxs)
        want = None
        for fx in fxs:
            w = expected(fx, d)
            want = w if want is None else add_grids(want, w)
        assert_grid(acc, want, f"{what}: the effect form, accumulated")
        assert_grid(d, want, f"{what}: the program form, {d.plan(cap, True, len(fxs))[0]}")
        wants.append(want)
    return wants[0]


@pytest.mark.parametrize("cap", [300, 4097, 10_000])
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
    assert frozen[2][0] == cap // 3                                        # the frozen instance deposits the state it was frozen in
    want = check_program(ctx, prog, fxs, dsts, f"capacity {cap}, die-off")
    assert cap // 3 < want[2][0] < sum(spawns)
    ctx.close()


def test_program_of_300_instances_of_300_slots():
    n, cap = 300, 300
    ctx, prog, fxs = pes.make(cap, n)
    spawns = [(k * 7) % (cap + 1) for k in range(n)]
    pes.step(ctx, fxs, 0, spawns)
    pes.step(ctx, fxs, 1, [0] * n, dt=1 / 30)                                # a shell of radius 1.3 .. 2 round the origin
    ch = [(A.VELOCITY.id, 0, 16), (A.LIFETIME.id, 0, 30)]
    b = box(1.5, 2.5)                                                        # [-1.5, 1.5) along x and y: part of the shell is outside
    want = check_program(ctx, prog, fxs, (lambda: Dst((4, 4, 4), ch, **b), lambda: padded(Dst((4, 4, 4), ch, **b))), "300 x 300")
    assert want[2][0] == sum(spawns) and 0 < want[2][1] < want[2][0] and (want[1] < 0).any()
    ctx.close()


# ---- stale AGE --------------------------------------------------------------------------------------------------------------------------------------
def test_stale_age_is_materialised_first_and_nothing_later_changes():
    """LEAN cohorts: the AGE plane is stale until something materialises it; a channel on AGE does. A twin context that never calls ends bit-identical."""
    cap = 100_000
    pairs = [make(cap, age_cohort=1) for _ in range(2)]
    (ctx, fx), (tctx, twin) = pairs
    assert fx.device_view().stale_attr_mask == 1 << A.AGE.id
    ch = [(A.AGE.id, 0, 32), (A.VELOCITY.id, 1, 8)]
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
    assert want[2][0] == 70_000 + 4 * 3000 and ages.min() == dt and ages.max() > F32(4.5) * dt and want[1][:, 0].sum() > 70_000 * 4 * (2 ** 32 // 60)
    assert want[2][1] > 0 and (want[0][:-1] > 0).sum() > 16
    assert_grid(d, want, "stale AGE, in LDS")
    assert_padded(p, d, want, "stale AGE, in memory")
    assert keep[0][0].read()[2][0] == 70_000 + 3 * 3000
    for f in range(5, 12):
        for c, e in pairs:
            step(c, e, f, 0, dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    diff = fx.compare(twin)
    assert diff["equal"] == 1, diff
    assert fx.check()["ok"] == 1
    ctx.close(); tctx.close()


# ---- in the stream, next to the exports and the bounds ------------------------------------------------------------------------------------------------
def test_ten_calls_interleaved_with_frames_binned_exports_and_bounds_without_a_synchronisation():
    """Ten program calls and ten effect calls into twenty destinations, a frame between two of them, a binned export and a bounds call in between, and
    no synchronisation of the context until the end. The expected grids of call i come from a replica context that runs the same frames and is read
    back after each; hnb_effect_compare proves at the end that the replica is the calling context's state."""
    cap, n = 10_000, 2
    (ctx, prog, fxs), (rctx, rprog, rfxs) = pes.make(cap, n), pes.make(cap, n)
    ch = [(A.VELOCITY.id, 1, 12), (A.AGE.id, 0, 32)]
    b = box(3.0, 16.0)                                                       # (drag 4 on 60 units a second: nothing travels 16 units)
    calls, want, others = [], [], []                                        # (others: their destinations stay allocated until the stream has run them)
    for f in range(10):
        spawns = [cap if f == 0 else 0, 50 * f]
        for c, e in ((ctx, fxs), (rctx, rfxs)):
            pes.step(c, e, f, spawns, dt=1 / 600 if f == 0 else 0.12)
        calls.append((run(prog, Dst((4, 4, 4), ch, **b)), run(fxs[1], padded(Dst((4, 4, 4), ch[:1], **b)))))
        grid = BinGrid((4, 4, 4), b["origin"], b["inv_cell"])
        others.append((run_binned(Export(POS_AGE_LIFE_VEL, 32, cap), fxs[0], grid), grid, run_bounds(fxs[0], A.POSITION.id)))
        rctx.synchronize()
        wp = add_grids(expected(rfxs[0], calls[-1][0]), expected(rfxs[1], calls[-1][0]))
        small = Dst((4, 4, 4), ch[:1], **b)
        want.append((wp, small, expected(rfxs[1], small)))
    ctx.synchronize()
    for f, ((dp, de), (wp, small, we)) in enumerate(zip(calls, want)):
        assert_grid(dp, wp, f"program call behind frame {f}")
        assert_padded(de, small, we, f"effect call behind frame {f}")
    assert 0 < want[-1][0][2][0] < cap + 50 * 45 and want[-1][2][2][0] > 0   # the burst is dying off, the trickle is alive
    assert (want[3][0][0][:-1] > 0).sum() > 8 and (want[3][0][1] < 0).any()
    for a, b in zip(fxs, rfxs):
        assert a.compare(b)["equal"] == 1
    ctx.close(); rctx.close()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    """Every refusal of the contract but two: more than 65535 instances, which no test here creates, and a layout without POSITION, which the
    stand-alone program of tests/test_deposit_abi.py holds."""
    cap = 5000
    ctx, prog, fxs = pes.make(cap, 2)
    pes.step(ctx, fxs, 0, [cap, 100])
    empty_prog = ctx.create_program(bh.lower(effects.firework_trails(300)))
    fx = fxs[0]
    lib = runtime.load_library()
    d = Dst((4, 4, 4), [(A.VELOCITY.id, 1, 16), (A.AGE.id, 0, 32)])
    good = lambda: runtime.deposit_desc(**d.args())
    nan, inf = float("nan"), float("inf")

    def refused(call, handle, desc, text):
        assert call(handle, C.byref(desc)) == -1, text
        assert text.encode() in lib.hnb_last_error(), (text, lib.hnb_last_error())

    for call, handle in ((lib.hnb_effect_deposit, fx._h), (lib.hnb_program_deposit, prog._h)):
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
        for attr in (A.COLOR.id, A.SIZE3.id, A.ID.id, 9999):               # packed u32; not in the layout; not stored; no attribute
            x = good(); x.channels[1].attr = attr
            refused(call, handle, x, "channels[1]")
            assert b"not an f32 attribute" in lib.hnb_last_error()
        x = good(); x.channels[0].comp = 3
        refused(call, handle, x, "comp is at or past")
        x = good(); x.channels[1].frac_bits = 33
        refused(call, handle, x, "frac_bits is above 32")
        x = good(); x.channels[1].reserved = 1
        refused(call, handle, x, "reserved is not 0")
        x = good(); x.channels[3].frac_bits = 1
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
    refused(lib.hnb_program_deposit, empty_prog._h, good(), "0 instances")
    ctx.synchronize()
    assert d.untouched()
    run(prog, d)                                                           # ... and the same destination takes a good call
    ctx.synchronize()
    assert_grid(d, add_grids(expected(fxs[0], d), expected(fxs[1], d)), "a good call behind the refusals")
    ctx.close()
