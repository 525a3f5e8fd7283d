"""hnb_effect_pairs_from on the GPU (include/hanabi_amd_pairs_from.h): the fixed-radius neighbour list across two effects of one context as CSR - fx's
slot of every sorted inside query row, the offsets of its run, the SOURCE's slots within the radius and their squared distances. The expectation is
always the brute-force numpy restatement (tests/test_pairs_from_abi.py np_pairs_from / pairs_from_buffers) over the host's read-back of the positions
and the alive lists of BOTH effects, compared bit for bit over WHOLE buffers: out_rows and out_start with their tails, out_pairs and out_d2 with the
entries the call must leave alone. There is no tolerance anywhere. Every destination sits between guard words filled with a sentinel. Before comparing,
each main case asserts on the restatement alone what makes the case worth running."""
import ctypes as C

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
from test_gpu_neighbours import ATTRS4, DIMS, Stats, radius_of
from test_gpu_neighbours_from import OFFSETS27, S_SEED, TRAIL, burst2, grid_over, make2, step2
from test_gpu_pairs import SENT, Out
from test_neighbours_abi import ONE, SET, W_ONE
from test_pairs_abi import NO_ROW, truncations
from test_pairs_from_abi import np_d2_from, np_pairs_from, pairs_from_buffers

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
COUNT = [(ONE, 0, 0, 0, A.F32X4_0.id, 0, SET)]


def positions(fx):
    return fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)


def reference(fq, fs, grid, radius, limit=4096):
    """the restatement over the host's read-back of both effects as they are (synchronises)"""
    return np_pairs_from(positions(fq), fq.alive_list(), positions(fs), fs.alive_list(), (grid.dims, grid.origin, grid.inv_cell), radius, limit)


def assert_out(out, ref, cap, what):
    """every buffer whole against the restatement; cap is fx's capacity"""
    rows, start, written, pairs, d2, stats = pairs_from_buffers(ref, cap, out.pc)
    np.testing.assert_array_equal(out.read("rows"), rows, err_msg=f"{what}: out_rows")
    np.testing.assert_array_equal(out.read("start"), start, err_msg=f"{what}: out_start")
    if "pairs" in out.buf:
        np.testing.assert_array_equal(out.read("pairs"), np.concatenate([pairs, np.full(out.pc - written, SENT, U32)]), err_msg=f"{what}: out_pairs")
    if "d2" in out.buf:
        np.testing.assert_array_equal(out.read("d2"), np.concatenate([d2, np.full(out.pc - written, SENT, U32)]), err_msg=f"{what}: out_d2")
    if "stats" in out.buf:
        np.testing.assert_array_equal(out.read("stats"), stats, err_msg=f"{what}: out_stats")


def check(ctx, fq, fs, grid, radius, what, limit=4096, pc=None, d2=True, ref=None, conditions=None):
    """one call against the restatement -> (ref, out); pc None: room for every pair and seven entries more, which must keep their sentinel"""
    ref = reference(fq, fs, grid, radius, limit) if ref is None else ref
    if conditions:
        conditions(ref)
    out = Out(fq.capacity, int(ref["T"][-1]) + 7 if pc is None else pc, d2=d2, pairs=pc is None or pc > 0)
    fq.pairs_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, candidate_limit=limit, **out.args())
    ctx.synchronize()
    assert_out(out, ref, fq.capacity, what)
    return ref, out


def listed(out):
    """(query slot, source slot, d2 words) of every pair of a list that was not truncated, from the device's own buffers"""
    rows, start = out.read("rows").astype(np.int64), out.read("start").astype(np.int64)
    total = int(start[-1])
    return np.repeat(rows, np.diff(start)), out.read("pairs")[:total].astype(np.int64), out.read("d2")[:total]


# ---- 1. capacities: the one-workgroup sort and the multi-pass one on each side independently, a partial last tile ------------------------------------
CAPS = [(1, 1), (3, 300), (300, 3), (4096, 4097), (4097, 4096), (10_000, 300)]


@pytest.mark.parametrize("cap_q,cap_s", CAPS)
def test_capacities_on_the_burst_states(cap_q, cap_s):
    ctx, fq, fs = burst2(cap_q, cap_s)
    grid = grid_over([fq, fs], DIMS[min(cap_q, cap_s)])
    radius = radius_of(grid)

    def conditions(ref):
        assert not ref["crowded"].any() and ref["n_outside"] == 0 and len(ref["rows"]) == cap_q and ref["s_inside"] == cap_s, "nobody is crowded or outside"
        if min(cap_q, cap_s) >= 4096:
            assert OFFSETS27 <= ref["offsets"], ("a pair for each of the 27 cell offsets", OFFSETS27 - ref["offsets"])

    ref, out = check(ctx, fq, fs, grid, radius, f"capacities {cap_q}, {cap_s}", conditions=conditions)
    assert out.read("stats").tolist()[:4] == [cap_q, cap_q, 0, 0] and out.read("stats")[7] == cap_s
    if max(cap_q, cap_s) > 1:
        assert int(ref["T"][-1]) > 0, "somebody has neighbours"
    # the run length of every row is what hnb_effect_neighbours_from stores for a count channel on the same state: device against device
    rows, start = out.read("rows").astype(np.int64), out.read("start").astype(np.int64)
    fq.neighbours_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, COUNT, W_ONE, 4096, 1.0)
    ctx.synchronize()
    counted = fq.read_attr(A.F32X4_0.id).view(F32).reshape(cap_q, 4)[:, 0]
    np.testing.assert_array_equal(counted[rows], np.diff(start).astype(F32))
    assert fq.check()["ok"] == 1 and fs.check()["ok"] == 1
    ctx.close()


# ---- 2. 66,000 queries against 300 sources: 258 tiles of 256 query rows - the tile scan's second round -----------------------------------------------
def test_66000_queries_run_the_tile_scans_second_round():
    cap_q, cap_s = 66_000, 300
    ctx, fq, fs = burst2(cap_q, cap_s)
    fq.write_attr(A.POSITION.id, np.random.default_rng(11).uniform(0, 1, (cap_q, 3)).astype(F32))
    fs.write_attr(A.POSITION.id, np.random.default_rng(12).uniform(0, 1, (cap_s, 3)).astype(F32))
    grid = Grid((6, 6, 6), (0, 0, 0), (6, 6, 6))

    def conditions(ref):
        assert -(-cap_q // 256) == 258 and len(ref["rows"]) == cap_q
        assert int(ref["T"][-1]) > 0 and ref["counts"][256 * 256:].any(), "the total is not 0, and some run lies in a tile past the first round of 256 tiles"
        assert int(ref["T"][256 * 256]) > 0

    ref, out = check(ctx, fq, fs, grid, radius_of(grid), "66,000 queries", conditions=conditions)
    ctx.close()


# ---- 3. truncation ------------------------------------------------------------------------------------------------------------------------------------
def test_truncation_writes_a_prefix_and_clamps_the_table():
    cap_q, cap_s = 4097, 3000
    ctx, fq, fs = burst2(cap_q, cap_s)
    grid = grid_over([fq, fs], (7, 7, 7))
    radius = radius_of(grid)
    ref = reference(fq, fs, grid, radius)
    total = int(ref["T"][-1])
    assert total >= 1000
    for pc in truncations(ref):                                            # 0, 1, inside a run, a run's boundary, total - 1, total, total + 1
        _, out = check(ctx, fq, fs, grid, radius, f"pair_capacity {pc} of {total}", pc=pc, ref=ref)
        stats, start = out.read("stats"), out.read("start")
        assert (int(stats[4]) | int(stats[5]) << 32, int(stats[6])) == (total, min(total, pc)) and int(start.max()) == min(total, pc) == int(start[-1])
    out = Out(cap_q, 0, d2=False, pairs=False)                             # count only: out_pairs is NULL
    assert out.ptr("pairs") is None and out.ptr("d2") is None
    fq.pairs_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, **out.args())
    ctx.synchronize()
    assert_out(out, ref, cap_q, "count only")
    assert not out.read("start").any() and out.read("stats").tolist()[4:] == [total, 0, 0, cap_s]
    ctx.close()


# ---- 4. crowding ----------------------------------------------------------------------------------------------------------------------------------------
def test_one_cell_that_holds_all_the_sources_with_a_limit_below_their_number():
    cap = 300
    ctx, fq, fs = burst2(cap, cap)
    rng = np.random.default_rng(2)
    fs.write_attr(A.POSITION.id, (1.5 + rng.uniform(-0.3, 0.3, (cap, 3))).astype(F32))          # every source in cell (1, 1, 1) of a 5 x 4 x 4 grid of unit cells
    pq = np.empty((cap, 3), F32)
    pq[:150] = rng.uniform(0.5, 2.9, (150, 3)).astype(F32)                                      # 150 queries in the cells around it: in reach
    pq[150:] = (np.array([4.5, 3.5, 3.5]) + rng.uniform(-0.4, 0.4, (150, 3))).astype(F32)       # 150 far away, in (4, 3, 3)
    fq.write_attr(A.POSITION.id, pq)
    grid = Grid((5, 4, 4), (0, 0, 0), (1, 1, 1))

    def below(ref):
        reach = np.isin(ref["rows"], np.arange(150))
        assert (ref["cand"][reach] == cap).all() and ref["crowded"][reach].all() and not ref["crowded"][~reach].any() and (ref["cand"][~reach] == 0).all()
        assert not ref["counts"].any() and len(ref["rows"]) == cap, "every query in reach is crowded and lists nothing; the others have nobody near"

    ref, out = check(ctx, fq, fs, grid, 1.0, "the limit one below the sources", limit=cap - 1, conditions=below)
    assert out.read("stats").tolist() == [cap, cap, 0, 150, 0, 0, 0, cap] and not out.read("start").any()

    def raised(ref):
        assert not ref["crowded"].any() and int(ref["T"][-1]) > 150, "raising the limit lists them"

    ref, out = check(ctx, fq, fs, grid, 1.0, "the limit at the sources", limit=cap, conditions=raised)
    assert out.read("stats")[3] == 0
    ctx.close()


# ---- 5. a grid that cuts through both clouds; non-finite positions; empty sides -----------------------------------------------------------------------
def test_a_grid_that_cuts_through_both_clouds_and_non_finite_positions_on_both_sides():
    cap_q, cap_s = 10_000, 4097
    ctx, fq, fs = burst2(cap_q, cap_s)
    grid = grid_over([fq, fs], (6, 6, 6), inner=0.6)

    def cut(ref):
        assert 0 < ref["n_outside"] < cap_q and 0 < ref["s_inside"] < cap_s and int(ref["T"][-1]) > 0, "there is an outside bin on each side"

    ref, out = check(ctx, fq, fs, grid, radius_of(grid), "inner 0.6", conditions=cut)
    assert (out.read("rows")[len(ref["rows"]):] == NO_ROW).all() and 0 < out.read("stats")[7] < cap_s
    nan, inf = F32(np.nan), F32(np.inf)
    special = [(nan, 0.5, 0.5), (0.5, -nan, 0.5), (inf, 0.5, 0.5), (0.5, 0.5, -inf), (-0.0, -0.0, -0.0), (0.0, 0.0, 0.0)]
    slots = np.arange(7, 7 + 500 * len(special), 500)
    for fx in (fq, fs):
        pos = positions(fx).copy()
        pos[slots] = np.array(special, F32)
        fx.write_attr(A.POSITION.id, pos)
    grid = Grid((4, 4, 4), (0, 0, 0), (1, 1, 1))                           # the origin at 0: -0 is inside; the clouds' negative halves are outside

    def conditions(ref):
        assert not np.isin(slots[:4], ref["rows"]).any() and np.isin(slots[4:], ref["rows"]).all(), "non-finite query positions are outside, signed zeros inside"
        assert not np.isin(slots[:4], ref["srows"]).any() and np.isin(slots[4:], ref["srows"]).all(), "... and the same on the source"
        assert not np.isin(slots[:4], ref["pairs"]).any() and np.isin(slots[4:], ref["pairs"]).all() and (ref["d2"] == 0).any()
        at_origin = np.isin(ref["rows"][ref["qrow"]], slots[4:]) & (ref["d2"] == 0)
        assert set(ref["pairs"][at_origin].tolist()) == set(slots[4:].tolist()), "the queries at the origin list the sources at the origin: coincident, at equal slot numbers too"

    check(ctx, fq, fs, grid, 0.8, "special positions", conditions=conditions)
    ctx.close()


def test_a_source_that_never_spawned_and_an_fx_that_never_spawned():
    cap = 300
    ctx, fq, fs = make2(cap, cap)
    step2(ctx, fq, fs, 0, cap, 0)
    step2(ctx, fq, fs, 1, 0, 0, dt=0.05)
    assert fs.alive_count() == 0 and fq.alive_count() == cap
    grid = grid_over([fq], (4, 4, 4))
    ref, out = check(ctx, fq, fs, grid, radius_of(grid), "no sources")
    assert out.read("stats").tolist() == [cap, cap, 0, 0, 0, 0, 0, 0] and not out.read("start").any() and (out.read("rows") != NO_ROW).all()
    ref, out = check(ctx, fs, fq, grid, radius_of(grid), "no queries")      # the other way round: nobody is visited, no row exists
    assert out.read("stats").tolist() == [0, 0, 0, 0, 0, 0, 0, cap] and not out.read("start").any() and (out.read("rows") == NO_ROW).all()
    ctx.close()


# ---- 6. deaths on both sides; the list forms -------------------------------------------------------------------------------------------------------------
def test_deaths_on_both_sides_suffix_lists_a_churn_list_and_after_a_re_spawn():
    cap_q, cap_s = 10_000, 8000
    ctx, fq, fs = make2(cap_q, cap_s, asset_s=effects.firework_trails(cap_s, spawner=bh.SpawnerSettings.rate(3000.0)))
    rng = np.random.default_rng(5)
    step2(ctx, fq, fs, 0, cap_q, 600)
    for f in range(1, 5):
        step2(ctx, fq, fs, f, 0, int(rng.integers(100, 600)), dt=0.25)
    aq, as_ = fq.alive_list(), fs.alive_list()
    assert 0 < len(aq) < cap_q and not np.array_equal(aq, np.arange(len(aq))), "part of fx has died"
    assert 0 < len(as_) < cap_s
    box = positions(fq)[aq]                                                # (the young sources sit near the origin, inside fx's shell: spread them over fx's box)
    fs.write_attr(A.POSITION.id, rng.uniform(box.min(axis=0), box.max(axis=0), (cap_s, 3)).astype(F32))
    grid = grid_over([fq, fs], (5, 5, 5), inner=0.9)
    ref, out = check(ctx, fq, fs, grid, radius_of(grid), "die-off", limit=8000)
    assert ref["n_alive"] == len(aq) and ref["n_outside"] > 0 and 0 < ref["s_inside"] < len(as_) and int(ref["T"][-1]) > 0
    for f in range(5, 40):                                                 # the source churns on; fx re-spawns into the slots its dead left
        step2(ctx, fq, fs, f, 300 if f % 4 == 0 else 0, int(rng.integers(100, 600)), dt=1 / 20)
    aq, as_ = fq.alive_list(), fs.alive_list()
    assert 256 < len(as_) < cap_s and not np.array_equal(as_, np.sort(as_)), "a churn list on the source"
    assert 256 < len(aq) < cap_q and not np.array_equal(aq, np.sort(aq)), "a list after deaths and re-spawns on fx"
    grid = grid_over([fq, fs], (4, 4, 4), inner=0.8)

    def conditions(ref):
        dead_s = np.setdiff1d(np.arange(cap_s), as_)
        assert len(dead_s) > 0 and int(ref["T"][-1]) > 0 and not np.isin(dead_s, ref["pairs"]).any()
        assert (grid.cells(positions(fs))[dead_s] != grid.n_cells).any(), "dead source slots hold positions inside the grid: they are in no run"
        assert not np.array_equal(ref["rows"], np.sort(ref["rows"]))

    ref, out = check(ctx, fq, fs, grid, radius_of(grid), "churn and re-spawn", limit=8000, conditions=conditions)
    ref, out = check(ctx, fs, fq, grid, radius_of(grid), "churn and re-spawn, roles swapped", limit=10_000)      # the churn list as the queries
    assert int(ref["T"][-1]) > 0
    assert fq.check()["ok"] == 1 and fs.check()["ok"] == 1
    ctx.close()


def test_a_ring_list_on_the_source_and_on_fx_is_read_through_its_head_and_left_alone():
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
    fs.write_attr(A.POSITION.id, np.random.default_rng(3).uniform(-1, 1, (cap_s, 3)).astype(F32))      # (the ribbon's particles sit on one point: spread them)
    fq.write_attr(A.POSITION.id, np.random.default_rng(4).uniform(-1.2, 1.2, (cap_q, 3)).astype(F32))
    grid = grid_over([fs], (5, 4, 3), inner=0.8)
    ref, out = check(ctx, fq, fs, grid, radius_of(grid), "a ring on the source")
    assert 0 < ref["s_inside"] < m.alive_count and 0 < ref["n_outside"] < ref["n_alive"] and int(ref["T"][-1]) > 0
    ref, out = check(ctx, fs, fq, grid, radius_of(grid), "a ring on fx")
    assert ref["n_alive"] == m.alive_count and 0 < ref["n_outside"] < ref["n_alive"] and int(ref["T"][-1]) > 0
    np.testing.assert_array_equal(fs.alive_list(), before)                 # the list, and with it the ribbon's own sort order, is what it was
    m2 = _device_meta(fs)
    assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


# ---- 7. out_d2 given or not ---------------------------------------------------------------------------------------------------------------------------
def test_the_list_is_the_same_with_and_without_d2_and_every_d2_is_the_rules():
    cap_q, cap_s = 4097, 4096
    ctx, fq, fs = burst2(cap_q, cap_s)
    grid = grid_over([fq, fs], (7, 7, 7))
    radius = radius_of(grid)
    ref, with_d2 = check(ctx, fq, fs, grid, radius, "with d2")
    _, without = check(ctx, fq, fs, grid, radius, "without d2", d2=False, ref=ref)
    for k in ("rows", "start", "pairs", "stats"):
        np.testing.assert_array_equal(with_d2.read(k), without.read(k))
    q, j, d2 = listed(with_d2)
    assert len(q) == int(ref["T"][-1]) > cap_q
    rule = np_d2_from(positions(fq)[q], positions(fs)[j])                  # the rule recomputed from the read-back, per listed pair (query, source)
    np.testing.assert_array_equal(d2, rule.view(U32))
    assert (rule < F32(radius) * F32(radius)).all()
    ctx.close()


# ---- 8. cross-checks against merged calls on the same state ---------------------------------------------------------------------------------------------
def test_swapped_roles_list_the_transposed_relation():
    ctx, fq, fs = burst2(4097, 3000)
    grid = grid_over([fq, fs], (7, 7, 7))
    radius = radius_of(grid)
    ref, a = check(ctx, fq, fs, grid, radius, "fx from source")
    back, b = check(ctx, fs, fq, grid, radius, "source from fx")
    assert a.read("stats")[3] == 0 and b.read("stats")[3] == 0 and a.read("stats")[2] == 0 and b.read("stats")[2] == 0, "nobody is crowded or outside"
    qa, ja, da = listed(a)
    qb, jb, db = listed(b)
    assert len(qa) == len(qb) > 4097
    fwd = np.lexsort((ja, qa))
    bwd = np.lexsort((qb, jb))                                             # the other list by (its neighbour, its query): the same order of the same pairs
    np.testing.assert_array_equal(qa[fwd], jb[bwd]); np.testing.assert_array_equal(ja[fwd], qb[bwd])
    np.testing.assert_array_equal(da[fwd], db[bwd])                        # d2 of (i, j) is d2 of (j, i), bit for bit
    ctx.close()


@pytest.mark.parametrize("limit", [4096, 400])
def test_a_twin_source_lists_what_hnb_effect_pairs_lists_plus_the_twin_of_the_query_itself(limit):
    cap = 4097
    ctx, fq, fs = burst2(cap, cap, seed_s=0)                               # the same asset, seeds and frames: the source's state is fx's
    grid = grid_over([fq], (7, 7, 7))
    radius = radius_of(grid)
    ref, twin = check(ctx, fq, fs, grid, radius, "the twin as the source", limit=limit)
    own = Out(cap, int(ref["T"][-1]))
    fq.pairs(grid.dims, grid.origin, grid.inv_cell, radius, candidate_limit=limit, **own.args())
    ctx.synchronize()
    np.testing.assert_array_equal(own.read("rows"), twin.read("rows"))
    np.testing.assert_array_equal(own.read("stats")[:4], twin.read("stats")[:4])      # crowding coincides: the candidate counts coincide
    assert (twin.read("stats")[3] > 0) == (limit < 4096) and int(own.read("stats")[4]) > 0
    rows = twin.read("rows").astype(np.int64)
    n_inside = int(twin.read("stats")[1])
    row_of = np.full(cap, -1, np.int64)
    row_of[rows[:n_inside]] = np.arange(n_inside)                          # the twin's sorted rows are fx's: one state, one sort
    key = lambda out: (lambda q, j, d: row_of[q] * cap + row_of[j])(*listed(out))
    k_twin, k_own = key(twin), key(own)
    assert (np.diff(k_twin) > 0).all() and (np.diff(k_own) > 0).all(), "CSR order: by row, then by ascending neighbour row"
    listing = np.flatnonzero(np.diff(twin.read("start").astype(np.int64))[:n_inside] > 0)       # the rows that are not crowded: each lists at least its own twin
    assert n_inside - len(listing) == twin.read("stats")[3]
    np.testing.assert_array_equal(k_twin, np.sort(np.concatenate([k_own, listing * cap + listing])))
    ctx.close()


# ---- 9. nothing of either effect is written ---------------------------------------------------------------------------------------------------------------
def _pair(one_program, cap_q, cap_s):
    if not one_program:
        return make2(cap_q, cap_s)
    ctx = bh.Context(0)
    prog = ctx.create_program(bh.lower(trails_vec4(cap_q)))
    return ctx, prog.create_effect(), prog.create_effect()


def _state(fx):
    return planes(fx, ATTRS4), fx.alive_list().copy(), fx.dead_list().copy(), fx.metadata(), fx.check()


def _assert_same(after, before, what):
    for a in before[0]:
        np.testing.assert_array_equal(after[0][a], before[0][a], err_msg=f"{what}: attribute {a}")
    np.testing.assert_array_equal(after[1], before[1]); np.testing.assert_array_equal(after[2], before[2])
    assert after[3] == before[3] and after[4] == before[4], what


@pytest.mark.parametrize("one_program,frozen", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["two programs", "two programs, both frozen", "two instances of one program", "two frozen instances of one program"])
def test_nothing_of_either_effect_is_written_and_later_frames_are_those_of_a_twin_context_that_never_called(one_program, frozen):
    cap = 10_000
    A_, B_ = [_pair(one_program, cap, cap) for _ in range(2)]
    for f in range(6):
        for ctx, fq, fs in (A_, B_):
            step2(ctx, fq, fs, f, cap if f == 0 else 0, cap - 100 if f == 0 else 0, dt=1 / 30)
    (ca, qa, sa), (cb, qb, sb) = A_, B_
    if frozen:
        for fx in (qa, sa, qb, sb):
            fx.set_simulated(False)
    ca.synchronize()
    grid = grid_over([qa, sa], (8, 8, 8), inner=0.9)
    radius = radius_of(grid)
    before = (_state(qa), _state(sa))
    assert before[0][4]["ok"] == 1 and before[1][4]["ok"] == 1
    ref, out = check(ca, qa, sa, grid, radius, "between frames")
    assert int(ref["T"][-1]) > 0 and ref["n_outside"] > 0
    _assert_same(_state(qa), before[0], "fx"); _assert_same(_state(sa), before[1], "the source")
    ref, out = check(ca, sa, qa, grid, radius, "between frames, roles swapped")
    _assert_same(_state(qa), before[0], "fx as the source"); _assert_same(_state(sa), before[1], "the source as fx")
    if frozen:
        for fx in (qa, sa, qb, sb):
            fx.set_simulated(True)
    keep = [Out(cap, 1000) for _ in range(10)]                             # every destination before the loop: the constructor synchronises the device
    for f in range(6, 16):                                                 # ten further frames, a call behind each in one context only, nothing synchronised
        for ctx, fq, fs in (A_, B_):
            step2(ctx, fq, fs, f, 0, 0, dt=1 / 30)
        (qa if f & 1 else sa).pairs_from(sa if f & 1 else qa, grid.dims, grid.origin, grid.inv_cell, radius, **keep[f - 6].args())
    ca.synchronize(); cb.synchronize()
    assert 0 < qa.alive_count() == qb.alive_count() and 0 < sa.alive_count() == sb.alive_count()
    assert qa.compare(qb)["equal"] == 1 and sa.compare(sb)["equal"] == 1
    assert qa.metadata() == qb.metadata() and sa.metadata() == sb.metadata()
    for fx in (qa, sa, qb, sb):
        assert fx.check()["ok"] == 1
    assert all(int(o.read("stats")[0]) > 0 for o in keep)
    ca.close(); cb.close()


# ---- 10. calls in sequence ----------------------------------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_regrow_the_scratch_and_interleave_with_the_other_calls_and_a_frame():
    cap_q, caps_s = 4097, [300, 10_000]
    # (source, dims, part of the largest radius, pair_capacity or None for room): a small capacity, then one that regrows the scratch - a larger
    # source and a 41^3 table - while the call in front is queued; then behind the three merged calls; then behind a frame
    calls = [(0, (3, 3, 3), 0.9, None), (1, (41, 41, 41), 0.999, None), (1, (9, 8, 7), 0.5, 500), (0, (7, 7, 7), 0.8, 0), (1, (12, 12, 12), 0.7, None)]

    def state():
        ctx = bh.Context(0)
        fq = ctx.create_program(bh.lower(trails_vec4(cap_q))).create_effect()
        srcs = [ctx.create_program(bh.lower(trails_vec4(c))).create_effect() for c in caps_s]
        frame(ctx, fq, srcs, 0, 1 / 600, True)
        frame(ctx, fq, srcs, 1, 0.05, False)
        return ctx, fq, srcs

    def frame(ctx, fq, srcs, f, dt, spawn):
        ctx.frame_begin(dt, f * dt)
        fq.set_frame(cap_q if spawn else 0, frame_seed(f))
        for k, fs in enumerate(srcs):
            fs.set_frame(caps_s[k] if spawn else 0, frame_seed(f + S_SEED + 10 * k))
        ctx.simulate()

    def sequence(ctx, fq, srcs, on_call, bufs):
        """the calls in their order; on_call makes call k. The merged calls and the frame run the same in both passes: they write F32X4_0 of fq"""
        rows, offs, rows_s, offs_s, st = bufs
        for k in range(len(calls)):
            if k == 2:
                g, r = on_call.merged
                fq.pairs(g.dims, g.origin, g.inv_cell, r, rows.data_ptr(), offs.data_ptr(), stats_ptr=st[0].ptr())
                fq.neighbours(g.dims, g.origin, g.inv_cell, r, [(ONE, 0, 0, 0, A.F32X4_0.id, 1, SET)], W_ONE, 4096, 1.0, st[1].ptr())
                fq.neighbours_from(srcs[1], g.dims, g.origin, g.inv_cell, r, COUNT, W_ONE, 4096, 1.0, st[2].ptr())
                srcs[1].pairs(g.dims, g.origin, g.inv_cell, r, rows_s.data_ptr(), offs_s.data_ptr(), stats_ptr=st[3].ptr())
            if k == 4:
                frame(ctx, fq, srcs, 2, 0.01, False)
            on_call(k, fq, srcs[calls[k][0]])

    def buffers():
        b = (torch.zeros(cap_q, dtype=torch.int32, device="cuda"), torch.zeros(cap_q + 1, dtype=torch.int32, device="cuda"),
             torch.zeros(caps_s[1], dtype=torch.int32, device="cuda"), torch.zeros(caps_s[1] + 1, dtype=torch.int32, device="cuda"), [Stats() for _ in range(4)])
        torch.cuda.synchronize()
        return b

    # pass 1: the expectations on the host, call by call, each from the read-back of the state it sees (nothing a call does changes a position)
    ctx, fq, srcs = state()
    want = []

    def expect(k, fq, fs):
        grid = grid_over([fq] + srcs, calls[k][1])
        radius = radius_of(grid, calls[k][2])
        want.append((grid, radius, reference(fq, fs, grid, radius)))
        if k == 1:
            expect.merged = (grid_over([fq] + srcs, (7, 7, 7)), radius_of(grid_over([fq] + srcs, (7, 7, 7))))

    sequence(ctx, fq, srcs, expect, buffers())
    ctx.synchronize()
    merged_total = None
    assert sum(int(w[2]["T"][-1]) > 0 for w in want) >= 4
    ctx.close()
    # every destination of every call before the first one is enqueued - `want` gives the sizes -: the constructors end in a device-wide
    # synchronisation, and none may stand between two calls
    outs = [Out(cap_q, int(ref["T"][-1]) + 7 if pc is None else pc, pairs=pc != 0, d2=pc != 0) for (_, _, _, pc), (grid, radius, ref) in zip(calls, want)]
    bufs = buffers()
    ctx, fq, srcs = state()                                                # a fresh context reaches the same states deterministically
    torch.cuda.synchronize()                                               # once; from here to the end nothing waits for the device

    def enqueue(k, fq, fs):
        grid, radius, ref = want[k]
        fq.pairs_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, **outs[k].args())

    enqueue.merged = expect.merged
    sequence(ctx, fq, srcs, enqueue, bufs)
    ctx.synchronize()
    for k, (out, (grid, radius, ref)) in enumerate(zip(outs, want)):
        assert_out(out, ref, cap_q, f"call {k}")
    st = bufs[4]
    merged_total = int(st[0].read()[4])
    y = fq.read_attr(A.F32X4_0.id).view(F32).reshape(-1, 4)
    assert merged_total > 0 and int(y[:, 1].astype(np.int64).sum()) == merged_total and st[1].read()[1] == cap_q and st[3].read()[0] == caps_s[1]      # the merged calls gave what they give alone
    assert int(y[:, 0].astype(np.int64).sum()) > 0 and st[2].read()[0] == cap_q
    ctx.close()


# ---- 11. argument errors --------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_on_live_effects_enqueue_nothing():
    """Every refusal class on live effects but a layout without POSITION and an effect of too many slots, which the stand-alone program of
    tests/test_pairs_from_abi.py holds"""
    cap_q, cap_s, pc = 5000, 3000, 3000
    ctx, fq, fs = burst2(cap_q, cap_s)
    other, oq, os_ = burst2(300, 300)
    lib = runtime.load_library()
    grid = grid_over([fq, fs], (6, 6, 6))
    radius = radius_of(grid)
    out = Out(cap_q, pc)
    good = lambda: runtime.pairs_desc(grid.dims, grid.origin, grid.inv_cell, radius, candidate_limit=4096, **out.args())
    nan, inf = float("nan"), float("inf")
    ctx.synchronize(); other.synchronize()
    before = (planes(fq, ATTRS4), planes(fs, ATTRS4))

    def refused(desc, *texts, a=None, b=None):
        assert lib.hnb_effect_pairs_from(fq._h if a is None else a, fs._h if b is None else b, C.byref(desc)) == -1, texts
        err = lib.hnb_last_error()
        assert err and all(t.encode() in err for t in texts), (texts, err)

    for a, b, d in ((None, fs._h, C.byref(good())), (fq._h, None, C.byref(good())), (fq._h, fs._h, None)):
        assert lib.hnb_effect_pairs_from(a, b, d) == -1 and b"NULL" in lib.hnb_last_error()
    refused(good(), "fx and source are one effect", "hnb_effect_pairs'", b=fq._h)
    refused(good(), "hnb_effect_pairs'", a=fs._h)
    refused(good(), "different contexts", b=oq._h)
    refused(good(), "different contexts", a=oq._h)
    x = good(); x.struct_size = 92; x.flags = 1
    refused(x, "fx and source are one effect", b=fq._h)                    # the two effects come before the description
    x = good(); x.struct_size = 92
    refused(x, "struct_size")
    for flags in (1, 3):
        x = good(); x.flags = flags
        refused(x, "HNB_PAIRS_HALF", "a slot order across two effects means nothing")
    for flags in (2, 0x80000000):
        x = good(); x.flags = flags
        refused(x, "flags must be 0")
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
    # the destinations are sized from FX's capacity (5000), not the source's (3000)
    for a, b, words in (("out_start", "out_rows", cap_q - 1), ("out_rows", "out_start", cap_q), ("out_d2", "out_pairs", pc - 1), ("out_d2", "out_pairs", 0), ("out_stats", "out_rows", 4),
                        ("out_stats", "out_d2", pc - 4), ("out_pairs", "out_start", cap_q), ("out_pairs", "out_stats", 7)):
        x = good(); setattr(x, a, getattr(x, b) + 4 * words)
        refused(x, "two destination ranges overlap")
    ctx.synchronize(); other.synchronize()
    assert out.untouched()
    for fx, b in ((fq, before[0]), (fs, before[1])):
        after = planes(fx, ATTRS4)
        for a in b:
            np.testing.assert_array_equal(after[a], b[a])
    check(ctx, fq, fs, grid, radius, "a good call behind the refusals")     # ... and the same effects take a good call
    o = Out(cap_q, 0, d2=False, stats=False, pairs=False)
    fq.pairs_from(fs, grid.dims, grid.origin, grid.inv_cell, radius, **o.args())      # out_stats, out_d2 and - counting only - out_pairs may be NULL
    ctx.synchronize()
    assert_out(o, reference(fq, fs, grid, radius), cap_q, "NULL stats, d2 and pairs")
    ctx.close(); other.close()
