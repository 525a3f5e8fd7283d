"""hnb_effect_pairs on the GPU (include/hanabi_amd_pairs.h): the fixed-radius neighbour list of one effect as CSR - the slot of every sorted inside row,
the offsets of its run, the neighbours' slots and their squared distances. The expectation is always the brute-force numpy restatement
(tests/test_pairs_abi.py np_pairs / pairs_buffers) over the host's read-back of the positions and the alive list, compared bit for bit over WHOLE
buffers: out_rows and out_start with their tails, out_pairs and out_d2 with the entries the call must leave alone. There is no tolerance anywhere.
Every destination sits between guard words filled with a sentinel. Before comparing, each main case asserts on the restatement alone what makes the
case worth running."""
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
from test_gpu_import import make, planes
from test_gpu_neighbours import ATTRS4, DIMS, radius_of
from test_neighbours_abi import ONE, SET, W_ONE
from test_pairs_abi import NO_ROW, np_pairs, pairs_buffers, truncations

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
GUARD = 4
SENT = U32(SENTINEL & 0xFFFFFFFF)
OFFSETS26 = set(itertools.product((-1, 0, 1), repeat=3)) - {(0, 0, 0)}
NAMES = ("rows", "start", "pairs", "d2", "stats")


class Out:
    """The destinations of one call: each a sentinel-filled device buffer with GUARD words in front and behind"""

    def __init__(self, cap, pc, d2=True, stats=True, pairs=True):
        self.n = dict(rows=cap, start=cap + 1, pairs=pc, d2=pc, stats=8)
        want = dict(rows=True, start=True, pairs=pairs, d2=d2, stats=stats)
        self.buf = {k: torch.full((self.n[k] + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for k in NAMES if want[k]}
        self.pc = pc
        torch.cuda.synchronize()                 # (the fills run on torch's stream, the call on the simulation's)

    def ptr(self, k):
        return self.buf[k].data_ptr() + 4 * GUARD if k in self.buf else None

    def args(self):
        return dict(rows_ptr=self.ptr("rows"), start_ptr=self.ptr("start"), pairs_ptr=self.ptr("pairs"), pair_capacity=self.pc, d2_ptr=self.ptr("d2"), stats_ptr=self.ptr("stats"))

    def read(self, k):
        raw = self.buf[k].cpu().numpy().view(U32)
        assert (raw[:GUARD] == SENT).all() and (raw[GUARD + self.n[k]:] == SENT).all(), f"words next to out_{k} were written"
        return raw[GUARD: GUARD + self.n[k]]

    def untouched(self):
        return all(bool((b.cpu().numpy().view(U32) == SENT).all()) for b in self.buf.values())


def reference(fx, grid, radius, limit=4096, half=False):
    """the restatement over the host's read-back of the effect as it is (synchronises)"""
    pos = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)
    return np_pairs(pos, fx.alive_list(), (grid.dims, grid.origin, grid.inv_cell), radius, limit, half)


def assert_out(out, ref, cap, what):
    """every buffer whole against the restatement"""
    rows, start, written, pairs, d2, stats = pairs_buffers(ref, cap, out.pc)
    np.testing.assert_array_equal(out.read("rows"), rows, err_msg=f"{what}: out_rows")
    np.testing.assert_array_equal(out.read("start"), start, err_msg=f"{what}: out_start")
    if "pairs" in out.buf:
        np.testing.assert_array_equal(out.read("pairs"), np.concatenate([pairs, np.full(out.pc - written, SENT, U32)]), err_msg=f"{what}: out_pairs")
    if "d2" in out.buf:
        np.testing.assert_array_equal(out.read("d2"), np.concatenate([d2, np.full(out.pc - written, SENT, U32)]), err_msg=f"{what}: out_d2")
    if "stats" in out.buf:
        np.testing.assert_array_equal(out.read("stats"), stats, err_msg=f"{what}: out_stats")


def check(ctx, fx, grid, radius, what, limit=4096, half=False, pc=None, d2=True, ref=None, conditions=None):
    """one call against the restatement -> (ref, out); pc None: room for every pair and seven entries more, which must keep their sentinel"""
    ref = reference(fx, grid, radius, limit, half) if ref is None else ref
    if conditions:
        conditions(ref)
    out = Out(fx.capacity, int(ref["T"][-1]) + 7 if pc is None else pc, d2=d2, pairs=pc is None or pc > 0)
    fx.pairs(grid.dims, grid.origin, grid.inv_cell, radius, candidate_limit=limit, half=half, **out.args())
    ctx.synchronize()
    assert_out(out, ref, fx.capacity, what)
    return ref, out


def burst(cap, asset=None, **options):
    ctx, fx = make(cap, trails_vec4(cap) if asset is None else asset, **options)
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    return ctx, fx


def spread(fx, seed, lo=0.0, hi=1.0):
    """uniform positions over [lo, hi)^3 for every slot"""
    pos = np.random.default_rng(seed).uniform(lo, hi, (fx.capacity, 3)).astype(F32)
    fx.write_attr(A.POSITION.id, pos)
    return pos


# ---- 1. capacities: the one-workgroup sort, the first multi-tile capacity, a partial last tile; the burst state --------------------------------------
@pytest.mark.parametrize("cap", [1, 3, 300, 4096, 4097, 10_000])
def test_capacities_on_the_burst_state(cap):
    ctx, fx = burst(cap)
    grid = grid_around(fx, DIMS[cap])
    radius = radius_of(grid)

    def conditions(ref):
        assert not ref["crowded"].any() and ref["n_outside"] == 0 and len(ref["rows"]) == cap, "no particle is crowded or outside"
        if cap >= 300:
            assert OFFSETS26 <= ref["offsets"], ("a pair for every one of the 26 cell offsets", OFFSETS26 - ref["offsets"])

    ref, out = check(ctx, fx, grid, radius, f"capacity {cap}", conditions=conditions)
    rows, start, pairs = out.read("rows").astype(np.int64), out.read("start").astype(np.int64), out.read("pairs")
    total = int(start[-1])
    q = np.repeat(rows, np.diff(start))
    listed = set(zip(q.tolist(), pairs[:total].tolist()))
    assert len(listed) == total and listed == {(j, i) for i, j in listed}, "the full list is symmetric"
    # the run lengths are what hnb_effect_neighbours stores for a count channel on the same state: device against device
    fx.neighbours(grid.dims, grid.origin, grid.inv_cell, radius, [(ONE, 0, 0, 0, A.F32X4_0.id, 0, SET)], W_ONE, 4096, 1.0)
    ctx.synchronize()
    counted = fx.read_attr(A.F32X4_0.id).view(F32).reshape(cap, 4)[:, 0]
    np.testing.assert_array_equal(counted[rows], np.diff(start).astype(F32))
    if cap == 1:
        assert start.tolist() == [0, 0] and out.read("stats").tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    ctx.close()


# ---- 2. 66,000 slots: 258 tiles of 256 rows - the tile scan's second round ---------------------------------------------------------------------------
def test_66000_slots_run_the_tile_scans_second_round():
    cap = 66_000
    ctx, fx = burst(cap)
    spread(fx, 11)
    grid = Grid((56, 56, 56), (0, 0, 0), (56, 56, 56))

    def conditions(ref):
        assert -(-cap // 256) == 258 and len(ref["rows"]) == cap
        assert ref["cand"].max() <= 30, "a grid fine enough that a query has at most 30 candidates"
        assert int(ref["T"][256 * 256]) > 0 and int(ref["T"][-1]) > int(ref["T"][256 * 256]), "pairs in front of and behind the first round of 256 tiles"

    ref, out = check(ctx, fx, grid, radius_of(grid), "66,000 slots", limit=64, conditions=conditions)
    assert out.read("stats")[3] == 0
    ctx.close()


# ---- 3. HALF ------------------------------------------------------------------------------------------------------------------------------------------
def test_half_list_is_the_full_list_filtered_by_the_slot_order():
    cap = 4097
    ctx, fx = burst(cap)
    grid = grid_around(fx, (7, 7, 7))
    radius = radius_of(grid)
    full, out_full = check(ctx, fx, grid, radius, "full")
    half, out_half = check(ctx, fx, grid, radius, "half", half=True)
    assert not full["crowded"].any() and int(full["T"][-1]) == 2 * int(half["T"][-1]) > 0, "nobody crowded: exactly half"
    rows, start = out_full.read("rows").astype(np.int64), out_full.read("start").astype(np.int64)
    total = int(start[-1])
    q = np.repeat(rows, np.diff(start))
    keep = out_full.read("pairs")[:total] > q
    np.testing.assert_array_equal(out_half.read("pairs")[: int(half["T"][-1])], out_full.read("pairs")[:total][keep])
    np.testing.assert_array_equal(out_half.read("d2")[: int(half["T"][-1])], out_full.read("d2")[:total][keep])
    np.testing.assert_array_equal(out_half.read("rows"), out_full.read("rows"))
    # crowded queries: the half list loses the pairs whose lower slot is crowded, and stats[3] says so
    limit = int(np.sort(full["cand"])[len(full["cand"]) // 2])
    ref, out = check(ctx, fx, grid, radius, "half, crowded", half=True, limit=limit)
    assert out.read("stats")[3] > 0 and int(ref["T"][-1]) < int(half["T"][-1])
    ctx.close()


# ---- 4. truncation ------------------------------------------------------------------------------------------------------------------------------------
def test_truncation_writes_a_prefix_and_clamps_the_table():
    cap = 4097
    ctx, fx = burst(cap)
    grid = grid_around(fx, (7, 7, 7))
    radius = radius_of(grid)
    ref = reference(fx, grid, radius)
    total = int(ref["T"][-1])
    assert total >= 1000
    for pc in truncations(ref):
        _, out = check(ctx, fx, grid, radius, f"pair_capacity {pc} of {total}", pc=pc, ref=ref)
        stats, start = out.read("stats"), out.read("start")
        assert (int(stats[4]) | int(stats[5]) << 32, int(stats[6])) == (total, min(total, pc)) and int(start.max()) == min(total, pc) == int(start[-1])
    out = Out(cap, 0, d2=False, pairs=False)                               # count only: out_pairs is NULL
    assert out.ptr("pairs") is None and out.ptr("d2") is None
    fx.pairs(grid.dims, grid.origin, grid.inv_cell, radius, **out.args())
    ctx.synchronize()
    assert_out(out, ref, cap, "count only")
    assert not out.read("start").any() and out.read("stats").tolist()[4:] == [total, 0, 0, 0]
    ctx.close()


# ---- 5. edge states -----------------------------------------------------------------------------------------------------------------------------------
def test_one_cell_that_holds_everything_and_crowded_queries():
    cap = 300
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, 200)                                                  # 200 particles within a hair of the origin: every ordered pair is within the radius
    grid = Grid((1, 1, 1), (-8, -8, -8), (1 / 16, 1 / 16, 1 / 16))
    ref, out = check(ctx, fx, grid, 16.0, "1 x 1 x 1", limit=200)
    assert len(ref["rows"]) == 200 and (ref["counts"] == 199).all() and int(ref["T"][-1]) == 200 * 199
    ref, out = check(ctx, fx, grid, 16.0, "1 x 1 x 1, one below the count", limit=199)     # ... and with the limit one below: everything is crowded
    assert out.read("stats").tolist() == [200, 200, 0, 200, 0, 0, 0, 0] and not out.read("start").any()
    # crowded queries have empty runs yet appear in others' runs
    rng = np.random.default_rng(2)
    pos, alive = np.zeros((cap, 3), F32), fx.alive_list()
    pos[alive[:150]] = (1.5 + rng.uniform(-0.3, 0.3, (150, 3))).astype(F32)                        # 150 in cell (1, 1, 1) of a 5 x 4 x 4 grid of unit cells
    pos[alive[150:170]] = (np.array([2.1, 1.5, 1.5]) + rng.uniform(0, 0.3, (20, 3))).astype(F32)   # 20 next to it, in (2, 1, 1): crowded as well
    pos[alive[170:]] = (np.array([3.05, 1.5, 1.5]) + rng.uniform(0, 0.25, (30, 3))).astype(F32)    # 30 in (3, 1, 1): they see 50 candidates
    fx.write_attr(A.POSITION.id, pos)
    grid = Grid((5, 4, 4), (0, 0, 0), (1, 1, 1))

    def conditions(ref):
        cr = ref["crowded"]
        assert cr.sum() == 170 and not ref["counts"][cr].any() and cr[ref["jrow"]].any(), "crowded queries list nothing and are listed by others"

    ref, out = check(ctx, fx, grid, 1.0, "crowding", limit=128, conditions=conditions)
    assert out.read("stats")[3] == 170
    ctx.close()


def test_a_grid_that_cuts_through_the_cloud_non_finite_positions_and_an_empty_effect():
    cap = 4097
    ctx, fx = burst(cap)
    grid = grid_around(fx, (6, 6, 6), inner=0.6)
    ref, out = check(ctx, fx, grid, radius_of(grid), "inner 0.6")
    assert 0 < ref["n_outside"] < cap and int(ref["T"][-1]) > 0 and (out.read("rows")[len(ref["rows"]):] == NO_ROW).all()
    pos = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3).copy()
    nan, inf = F32(np.nan), F32(np.inf)
    special = [(nan, 0.5, 0.5), (0.5, -nan, 0.5), (inf, 0.5, 0.5), (0.5, 0.5, -inf), (-0.0, -0.0, -0.0), (0.0, 0.0, 0.0)]
    slots = np.arange(7, 7 + 500 * len(special), 500)
    pos[slots] = np.array(special, F32)
    fx.write_attr(A.POSITION.id, pos)
    grid = Grid((4, 4, 4), (0, 0, 0), (1, 1, 1))                           # the origin at 0: -0 is inside; the cloud's negative half is outside

    def conditions(ref):
        assert not np.isin(slots[:4], ref["rows"]).any() and np.isin(slots[4:], ref["rows"]).all(), "non-finite positions are outside, signed zeros inside"
        assert not np.isin(slots[:4], ref["pairs"]).any() and np.isin(slots[4:], ref["pairs"]).all() and (ref["d2"] == 0).any()

    check(ctx, fx, grid, 0.8, "special positions", conditions=conditions)
    ctx.close()
    ctx, fx = make(300, trails_vec4(300))                                  # nothing was ever spawned
    ref, out = check(ctx, fx, Grid((3, 3, 3), (-1, -1, -1), (1.5, 1.5, 1.5)), 0.5, "an empty effect")
    assert not out.read("stats").any() and not out.read("start").any() and (out.read("rows") == NO_ROW).all()
    ctx.close()


# ---- 6. list shapes -----------------------------------------------------------------------------------------------------------------------------------
def test_after_a_die_off_and_on_a_churn_list():
    cap = 10_000
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    for f in range(1, 5):
        step(ctx, fx, f, 0, dt=0.25)
    alive = fx.alive_list()
    assert 0 < len(alive) < cap and not np.array_equal(alive, np.arange(len(alive)))
    grid = grid_around(fx, (5, 5, 5), inner=0.9)
    ref, out = check(ctx, fx, grid, radius_of(grid), "die-off")
    assert ref["n_alive"] == len(alive) and ref["n_outside"] > 0 and int(ref["T"][-1]) > 0
    ctx.close()
    cap = 8000
    ctx, fx = make(cap, effects.firework_trails(cap, spawner=bh.SpawnerSettings.rate(3000.0)))
    rng = np.random.default_rng(5)
    for f in range(40):
        step(ctx, fx, f, int(rng.integers(100, 600)), dt=1 / 20)
    alive = fx.alive_list()
    assert 256 < len(alive) < cap and not np.array_equal(alive, np.sort(alive))
    grid = grid_around(fx, (4, 4, 4), inner=0.8)
    ref, out = check(ctx, fx, grid, radius_of(grid), "churn", limit=8000)
    assert int(ref["T"][-1]) > 0 and not np.array_equal(ref["rows"], np.sort(ref["rows"]))
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
    spread(fx, 3, -1.0, 1.0)                                              # (the ribbon's particles sit on one point: spread them)
    grid = grid_around(fx, (5, 4, 3), inner=0.8)
    ref, out = check(ctx, fx, grid, radius_of(grid), "ring")
    assert ref["n_alive"] == m.alive_count and 0 < ref["n_outside"] < ref["n_alive"] and int(ref["T"][-1]) > 0
    np.testing.assert_array_equal(fx.alive_list(), before)
    m2 = _device_meta(fx)
    assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


# ---- 7. out_d2 given or not ---------------------------------------------------------------------------------------------------------------------------
def test_the_list_is_the_same_with_and_without_d2_and_every_d2_is_the_rules():
    cap = 4097
    ctx, fx = burst(cap)
    grid = grid_around(fx, (7, 7, 7))
    radius = radius_of(grid)
    ref, with_d2 = check(ctx, fx, grid, radius, "with d2")
    fx.set_simulated(False)                                               # a frozen instance takes the call like any other
    _, without = check(ctx, fx, grid, radius, "without d2", d2=False, ref=ref)
    for k in ("rows", "start", "pairs", "stats"):
        np.testing.assert_array_equal(with_d2.read(k), without.read(k))
    total = int(ref["T"][-1])
    assert total > cap and (with_d2.read("d2")[:total].view(F32) < F32(radius) * F32(radius)).all()     # (bit-equal to np_d2: assert_out compared them)
    ctx.close()


# ---- 8. nothing of the effect is written ------------------------------------------------------------------------------------------------------------------
def test_nothing_of_the_effect_is_written_and_later_frames_are_those_of_a_twin_that_never_called():
    cap = 10_000
    (ca, fa), (cb, fb) = [make(cap, trails_vec4(cap)) for _ in range(2)]
    for f in range(6):
        for c, fx in ((ca, fa), (cb, fb)):
            step(c, fx, f, cap if f == 0 else 0, dt=1 / 30)
    ca.synchronize()
    grid = grid_around(fa, (8, 8, 8), inner=0.9)
    before = (planes(fa, ATTRS4), fa.alive_list().copy(), fa.dead_list().copy(), fa.metadata(), fa.check())
    assert before[4]["ok"] == 1
    ref, out = check(ca, fa, grid, radius_of(grid), "between frames")
    assert int(ref["T"][-1]) > 0
    after = (planes(fa, ATTRS4), fa.alive_list(), fa.dead_list(), fa.metadata(), fa.check())
    for a in before[0]:
        np.testing.assert_array_equal(after[0][a], before[0][a])
    np.testing.assert_array_equal(after[1], before[1]); np.testing.assert_array_equal(after[2], before[2])
    assert after[3] == before[3] and after[4] == before[4]
    keep = [Out(cap, 1000) for _ in range(10)]                             # every destination before the loop: the constructor synchronises the device
    for f in range(6, 16):                                                 # ten further frames, a call behind each in one context only, nothing synchronised
        for c, fx in ((ca, fa), (cb, fb)):
            step(c, fx, f, 0, dt=1 / 30)
        fa.pairs(grid.dims, grid.origin, grid.inv_cell, radius_of(grid), half=bool(f & 1), **keep[f - 6].args())
    ca.synchronize(); cb.synchronize()
    assert 0 < fa.alive_count() == fb.alive_count()
    d = fa.compare(fb)
    assert d["equal"] == 1, d
    assert fa.metadata() == fb.metadata() and fa.check()["ok"] == 1
    ca.close(); cb.close()


# ---- 9. scratch reuse ---------------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_share_the_scratch_in_stream_order_between_other_calls_and_a_frame():
    cap = 4097
    calls = [((3, 3, 3), 0.9, False, None), ((9, 8, 7), 0.5, True, 500), ((12, 12, 12), 1.0, False, 0), ((2, 2, 2), 0.7, True, None), ((41, 41, 41), 0.999, False, None)]

    def state():
        ctx, fx = burst(cap)
        return ctx, fx

    # the expectations on the host from one context; nothing the calls do changes the effect, so every call sees this state - but the frame in the
    # middle moves it on: calls behind it are stated from the state behind it
    ctx, fx = state()
    want = []
    for k, (dims, part, half, pc) in enumerate(calls):
        if k == 3:
            step(ctx, fx, 2, 0, dt=0.01)
        grid = grid_around(fx, dims)
        radius = radius_of(grid, part)
        want.append((grid, radius, reference(fx, grid, radius, 4096, half)))
    assert sum(int(w[2]["T"][-1]) > 0 for w in want) >= 4
    ctx.close()
    # every destination of every call before the first one is enqueued - `want` gives the sizes -: the constructors of Out, Grid and Export end in
    # a device-wide synchronisation, and none may stand between two calls
    outs = [Out(cap, int(ref["T"][-1]) + 7 if pc is None else pc, pairs=pc != 0, d2=pc != 0) for (dims, part, half, pc), (grid, radius, ref) in zip(calls, want)]
    tables = [Grid(grid.dims, grid.origin, grid.inv_cell) for grid, radius, ref in want]
    exports = [Export(POS_AGE_LIFE_VEL, 32, cap) for _ in calls]
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    ctx, fx = state()                                                      # a fresh context reaches the same states deterministically
    torch.cuda.synchronize()                                               # once; from here to the end nothing waits for the device
    for k, ((dims, part, half, pc), (grid, radius, ref)) in enumerate(zip(calls, want)):
        if k == 3:
            step(ctx, fx, 2, 0, dt=0.01)
        run_binned(exports[k], fx, tables[k])
        fx.pairs(grid.dims, grid.origin, grid.inv_cell, radius, half=half, **outs[k].args())    # (call 4's 41^3 table grows the scratch while the calls in front are queued)
        fx.neighbours(grid.dims, grid.origin, grid.inv_cell, radius, [(ONE, 0, 0, 0, A.F32X4_0.id, 0, SET)], W_ONE, 4096, 1.0, st.data_ptr())
    ctx.synchronize()
    for k, (out, (grid, radius, ref)) in enumerate(zip(outs, want)):
        assert_out(out, ref, cap, f"call {k}")
    ctx.close()


# ---- 10. argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    """Every refusal class on a live effect but a layout without POSITION and an effect of too many slots, which the stand-alone program of
    tests/test_pairs_abi.py holds"""
    cap, pc = 5000, 3000
    ctx, fx = burst(cap)
    lib = runtime.load_library()
    grid = grid_around(fx, (6, 6, 6))
    radius = radius_of(grid)
    out = Out(cap, pc)
    good = lambda: runtime.pairs_desc(grid.dims, grid.origin, grid.inv_cell, radius, candidate_limit=4096, **out.args())
    nan, inf = float("nan"), float("inf")
    ctx.synchronize()

    def refused(desc, text):
        assert lib.hnb_effect_pairs(fx._h, C.byref(desc)) == -1, text
        err = lib.hnb_last_error()
        assert err and text.encode() in err, (text, err)

    assert lib.hnb_effect_pairs(None, C.byref(good())) == -1 and b"NULL" in lib.hnb_last_error()
    assert lib.hnb_effect_pairs(fx._h, None) == -1 and b"NULL" in lib.hnb_last_error()
    x = good(); x.struct_size = 92
    refused(x, "struct_size")
    for flags in (2, 3, 0x80000000):
        x = good(); x.flags = flags
        refused(x, "flags: 0 or HNB_PAIRS_HALF")
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
    for bad in (0, 65537):
        x = good(); x.candidate_limit = bad
        refused(x, "candidate_limit is not 1..")
    x = good(); x.out_rows = None
    refused(x, "out_rows is NULL")
    x = good(); x.out_start = None
    refused(x, "out_start is NULL")
    x = good(); x.out_pairs = None
    refused(x, "out_pairs is NULL with pair_capacity above 0")
    for name in ("out_rows", "out_start", "out_pairs", "out_d2"):
        x = good(); setattr(x, name, getattr(x, name) + 2)
        refused(x, "not 4-byte aligned")
    x = good(); x.out_stats = out.ptr("stats") + 4
    refused(x, "out_stats: NULL or")
    for a, b, words in (("out_start", "out_rows", cap - 1), ("out_rows", "out_start", cap), ("out_d2", "out_pairs", pc - 1), ("out_d2", "out_pairs", 0), ("out_stats", "out_rows", 4),
                        ("out_stats", "out_d2", pc - 4), ("out_pairs", "out_start", cap), ("out_pairs", "out_stats", 7)):
        x = good(); setattr(x, a, getattr(x, b) + 4 * words)
        refused(x, "two destination ranges overlap")
    ctx.synchronize()
    assert out.untouched()
    check(ctx, fx, grid, radius, "a good call behind the refusals")         # ... and the same effect takes a good call
    o = Out(cap, 0, d2=False, stats=False, pairs=False)
    fx.pairs(grid.dims, grid.origin, grid.inv_cell, radius, **o.args())     # out_stats, out_d2 and - counting only - out_pairs may be NULL
    ctx.synchronize()
    assert_out(o, reference(fx, grid, radius), cap, "NULL stats, d2 and pairs")
    ctx.close()
