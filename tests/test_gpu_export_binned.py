"""hnb_effect_export_binned on the GPU (include/hanabi_amd_binned.h): record r of the caller's buffer = the particle with
the r-th smallest grid cell, ties in list order, and cell_start[c] = the records in cells below c. Expected records are built on the host as
tests/test_gpu_export.py builds them (read_attr + alive_list()), the cells restated in numpy binary32 from the header's formulas
(tests/test_export_binned_abi.py), the order from a stable argsort, the table from searchsorted. Everything is compared bit for bit: every result is
uniquely determined, there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A, frame_seed
from test_export_binned_abi import np_cells, np_table
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, _device_meta, assert_export, expected_records, step
from test_gpu_export_sorted import CAPS, TILE, burst_then_die_off, make, varying_bytes

pytestmark = pytest.mark.gpu

F32 = np.float32
POS_ID = [(A.POSITION.id, 0), (A.ID.id, 12)]        # stride 16: the slot in every record says which particle it is


class Grid:
    """A uniform grid as the call takes it: binary32 origin and 1 / cell edge, and the sentinel-filled device table (8 words more than it needs)"""

    def __init__(self, dims, origin, inv_cell):
        self.dims = tuple(int(d) for d in dims)
        self.origin, self.inv_cell = np.asarray(origin, F32), np.asarray(inv_cell, F32)
        self.n_cells = self.dims[0] * self.dims[1] * self.dims[2]
        self.table = torch.full((self.n_cells + 2 + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def fresh(self):
        return Grid(self.dims, self.origin, self.inv_cell)

    def words(self):
        return self.table.cpu().numpy().view(np.uint32)

    def cells(self, p):
        return np_cells(p, self.dims, self.origin, self.inv_cell)


def positions(fx, alive=None):
    p = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3)
    return p if alive is None else p[alive]


def grid_around(fx, dims, inner=None):
    """A grid of `dims` cells over the box of the alive particles' finite positions, a hair larger so that nothing is outside; inner: over the middle
    `inner` of that box along every axis, so that some particles are."""
    p = positions(fx, fx.alive_list()).astype(np.float64)
    p = p[np.isfinite(p).all(axis=1)]
    lo, hi = (p.min(axis=0), p.max(axis=0)) if len(p) else (np.full(3, -1.0), np.full(3, 1.0))
    size = np.maximum(hi - lo, 1e-3)
    if inner is None:
        lo, size = lo - 0.01 * size, 1.02 * size
    else:
        lo, size = lo + 0.5 * (1 - inner) * size, inner * size
    return Grid(dims, lo, np.asarray(dims, np.float64) / size)


def expected_binned(fx, fields, stride, grid):
    """-> (the records in cell order, the cells in list order, the stable order, the table)"""
    alive = fx.alive_list()
    cells = grid.cells(positions(fx, alive))
    order = np.argsort(cells, kind="stable")
    return expected_records(fx, fields, stride)[order], cells, order, np_table(cells[order], grid.n_cells)


def run_binned(ex, fx, grid):
    fx.export_binned(ex.fields, ex.dst.data_ptr(), ex.stride, ex.capacity, ex.cnt.data_ptr(), dims=grid.dims, origin=grid.origin, inv_cell=grid.inv_cell,
                     cell_start_ptr=grid.table.data_ptr())
    return ex


def assert_binned(ex, grid, expected, what):
    """records, out_count and the sentinels behind them; the whole table and the sentinels behind it"""
    rec, cells, order, table = expected
    assert_export(ex, rec, what, alive_rows=len(rec))
    got = grid.words()
    np.testing.assert_array_equal(got[: grid.n_cells + 2], table, err_msg=what)
    assert (got[grid.n_cells + 2:] == SENTINEL).all(), f"{what}: words behind cell_start[n_cells + 1] were written"
    assert table[0] == 0 and table[-1] == len(rec) and table[-2] == (cells < grid.n_cells).sum()


def check_binned(ctx, fx, what, grid, fields=POS_AGE_LIFE_VEL, stride=32, capacity=None):
    """export, synchronise, compare; -> (cells in list order, the stable order, the table)"""
    ex = run_binned(Export(fields, stride, fx.capacity if capacity is None else capacity), fx, grid)
    ctx.synchronize()
    expected = expected_binned(fx, fields, stride, grid)
    assert_binned(ex, grid, expected, f"{what}, {grid.dims}")
    return expected[1:]


@pytest.mark.parametrize("cap", CAPS)
def test_every_capacity_on_the_burst_state_with_an_8x8x8_grid_around_the_cloud(cap):
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    cells, order, table = check_binned(ctx, fx, f"capacity {cap}", grid_around(fx, (8, 8, 8)))
    assert len(cells) == cap and cells.max() < 512 and len(np.unique(cells)) > 50 and not np.array_equal(order, np.arange(cap))
    cells, order, table = check_binned(ctx, fx, f"capacity {cap}, the middle of the cloud", grid_around(fx, (8, 8, 8), inner=0.6))
    assert 0 < table[512] < cap                                         # some inside, some in the outside bin
    ctx.close()


DIGIT_EDGES = [(17, 5, 3), (8, 8, 4), (257, 51, 5), (64, 32, 32), (64, 64, 32)]      # 255 | 256 | 65,535 | 65,536 | 131,072 cells


@pytest.mark.parametrize("cap", [TILE, 10_000])
def test_digit_edges_of_the_outside_key(cap):
    """n_cells = 255, 256, 65,535: the outside key is 0xFF | 0x100 | 0xFFFF and lies on the other side of a digit boundary from the largest inside
    key; 65,536: it alone has bit 16; 64 x 64 x 32: inside keys of three digits. With the outside key present and without it."""
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    passes = {}
    for dims in DIGIT_EDGES:
        for inner in (0.6, None):
            cells, order, table = check_binned(ctx, fx, f"capacity {cap}, inner {inner}", grid_around(fx, dims, inner))
            n_cells = dims[0] * dims[1] * dims[2]
            assert ((cells == n_cells).any()) == (inner is not None)
            passes[dims, inner] = varying_bytes(cells)
    assert passes[(17, 5, 3), None] == [0] and passes[(8, 8, 4), None] == [0] and passes[(8, 8, 4), 0.6] == [0, 1]         # 0x100 brings the second digit in
    assert passes[(257, 51, 5), None] == [0, 1] and passes[(64, 32, 32), None] == [0, 1] and passes[(64, 32, 32), 0.6] == [0, 1, 2]
    assert passes[(64, 64, 32), None] == [0, 1, 2] and passes[(64, 64, 32), 0.6] == [0, 1, 2]
    ctx.close()


@pytest.mark.parametrize("cap", [300, 4097])
def test_degenerate_grids_and_states(cap):
    ctx, fx = make(cap)
    grid = Grid((3, 2, 2), (-1, -1, -1), (1.5, 1, 1))
    ex = run_binned(Export(POS_AGE_LIFE_VEL, 32, cap), fx, grid)         # nothing alive: the table is all zeros
    ctx.synchronize()
    assert ex.counts() == [0, 0] and (ex.words() == SENTINEL).all()
    assert (grid.words()[:14] == 0).all() and (grid.words()[14:] == SENTINEL).all()
    step(ctx, fx, 0, cap - 7)
    step(ctx, fx, 1, 0, dt=0.05)
    big = Grid((4, 4, 4), (-1.5e6, -1.5e6, -1.5e6), (1e-6, 1e-6, 1e-6))  # every particle in one cell of 64 (t = 1.5 on every axis: cell 21): no pass runs
    cells, order, table = check_binned(ctx, fx, "one cell", big)
    assert len(np.unique(cells)) == 1 and 0 < cells[0] < 64 and np.array_equal(order, np.arange(cap - 7)) and varying_bytes(cells) == []
    far = Grid((4, 4, 4), (1e6, 1e6, 1e6), (1, 1, 1))                    # every particle outside
    cells, order, table = check_binned(ctx, fx, "all outside", far)
    assert (cells == 64).all() and (table[:65] == 0).all() and table[65] == cap - 7
    one = Grid((1, 1, 1), (-1e6, -1e6, -1e6), (4e-7, 4e-7, 4e-7))        # 1 x 1 x 1 around everything: hnb_effect_export, byte for byte
    binned = run_binned(Export(POS_AGE_LIFE_VEL, 32, cap), fx, one)
    plain = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    ctx.synchronize()
    np.testing.assert_array_equal(binned.words(), plain.words())
    assert binned.counts() == plain.counts() == [cap - 7, cap - 7] and list(one.words()[:3]) == [0, cap - 7, cap - 7]
    ctx.close()


def test_non_finite_and_signed_zero_positions_land_in_the_restatements_cell():
    cap = 10_000
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    ctx.synchronize()
    alive = fx.alive_list()
    pos = fx.read_attr(A.POSITION.id).view(F32).reshape(-1, 3).copy()
    nan, inf = F32(np.nan), F32(np.inf)
    special = [(nan, 0.5, 0.5), (0.5, nan, 0.5), (0.5, 0.5, -nan), (inf, 0.5, 0.5), (0.5, -inf, 0.5), (0.5, 0.5, inf), (-0.0, -0.0, -0.0), (0.0, 0.0, 0.0), (-0.0, 0.5, 1.0),
               (1.0, 1.0, 1.0), (np.nextafter(F32(1.0), F32(0)), 0.25, 0.25), (4.0, 0.0, 0.0), (np.nextafter(F32(4.0), F32(0)), 0.0, 0.0), (-1e-45, 0.0, 0.0)]
    rows = alive[7::701][: len(special)]                                 # scattered over the list, so over several tiles
    assert len(rows) == len(special)
    pos[rows] = np.array(special, F32)
    fx.write_attr(A.POSITION.id, pos.view(np.uint32))
    grid = Grid((4, 4, 4), (0, 0, 0), (1, 1, 1))                         # the origin at 0: -0 is inside, in cell 0 of its axis; the cloud's negative half is outside
    cells, order, table = check_binned(ctx, fx, "special positions", grid, fields=POS_ID, stride=16)
    at = {int(s): int(c) for s, c in zip(alive, cells)}
    got = [at[int(r)] for r in rows]
    assert got == [64] * 6 + [0, 0, 16, 1 + 4 + 16, 0, 64, 3, 64], got
    ctx.close()


@pytest.mark.parametrize("cap", [10_000, 135_245])
def test_order_inside_every_cell_is_list_order_after_a_die_off(cap):
    ctx, fx = burst_then_die_off(cap)
    alive = fx.alive_list()
    assert 0 < len(alive) < cap and not np.array_equal(alive, np.arange(len(alive)))
    for dims, inner in (((2, 2, 2), None), ((3, 1, 2), 0.5)):            # thousands of particles per cell
        ex = run_binned(Export(POS_ID, 16, cap), fx, grid := grid_around(fx, dims, inner))
        ctx.synchronize()
        expected = expected_binned(fx, POS_ID, 16, grid)
        assert_binned(ex, grid, expected, f"die-off at {cap}")
        slots = ex.words()[: len(alive) * 4].reshape(-1, 4)[:, 3]        # the ID field: slot_base 0
        table = expected[3]
        where = {int(s): i for i, s in enumerate(alive)}
        for c in range(grid.n_cells + 1):                                # the outside bin included
            rows = np.array([where[int(s)] for s in slots[table[c]: table[c + 1]]])
            assert (np.diff(rows) > 0).all(), (c, "not in list order")
        assert np.bincount(expected[1]).max() > len(alive) // 16
    ctx.close()


def test_order_inside_every_cell_is_list_order_on_the_list_of_a_rate_spawner_churn():
    cap = 135_245
    ctx, fx = make(cap, effects.firework_trails(cap, spawner=bh.SpawnerSettings.rate(3000.0)))
    rng = np.random.default_rng(5)
    for f in range(60):
        step(ctx, fx, f, int(rng.integers(1000, 6000)), dt=1 / 20)
    alive = fx.alive_list()
    assert 4 * TILE < len(alive) < cap and not np.array_equal(alive, np.sort(alive))
    cells, order, table = check_binned(ctx, fx, "churn", grid_around(fx, (4, 4, 4), inner=0.7), fields=POS_ID, stride=16)
    assert (np.diff(order[cells[order] == cells[order][0]]) > 0).all() and 0 < table[64] < len(alive)
    ctx.close()


def test_ring_list_is_read_through_its_head_and_left_alone():
    cap = 10_000
    fields = [(A.AGE.id, 0), (A.POSITION.id, 4), (A.RIBBON_ID.id, 16), (A.SIZE.id, 20)]
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
    cells, order, table = check_binned(ctx, fx, "ring", grid_around(fx, (5, 4, 3), inner=0.8), fields=fields, stride=24)
    assert len(np.unique(cells)) > 3 and not np.array_equal(order, np.arange(len(order)))
    np.testing.assert_array_equal(fx.alive_list(), before)              # the list, and with it the ribbon's own sort order, is what it was
    m2 = _device_meta(fx)
    assert (m2.list_column, m2.alive_count) == (m.list_column, m.alive_count)
    ctx.close()


def test_top_k_clamp_leaves_the_table_unclamped():
    cap = 10_000
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    base = grid_around(fx, (6, 5, 4), inner=0.7)
    for K in (1, 255, 4096, cap - 1):
        grid = base.fresh()
        ex = run_binned(Export(POS_AGE_LIFE_VEL, 32, K, slack=64), fx, grid)
        ctx.synchronize()
        expected = expected_binned(fx, POS_AGE_LIFE_VEL, 32, grid)
        assert len(expected[0]) == cap and ex.counts() == [K, cap]
        assert_binned(ex, grid, expected, f"first {K}")                  # the first K of the order, sentinels behind record K; the table of all cap rows
        assert expected[3][-1] == cap > K
    grid = base.fresh()
    ex0 = run_binned(Export(POS_AGE_LIFE_VEL, 32, 0, slack=16), fx, grid)
    ctx.synchronize()
    assert ex0.counts() == [0, cap] and (ex0.words() == SENTINEL).all()
    np.testing.assert_array_equal(grid.words()[: grid.n_cells + 2], expected_binned(fx, POS_AGE_LIFE_VEL, 32, grid)[3])
    ctx.close()


def test_stale_age_is_current_as_a_field_and_nothing_later_changes():
    """LEAN cohorts: the AGE plane is stale until something materialises it. The binned export does, for the field; a twin context that never
    exports ends the run in the same state."""
    cap = 100_000
    fields = [(A.AGE.id, 0), (A.LIFETIME.id, 4), (A.POSITION.id, 8)]
    pairs = [make(cap, age_cohort=1) for _ in range(2)]
    (ctx, fx), (tctx, twin) = pairs
    assert fx.device_view().stale_attr_mask == 1 << A.AGE.id
    grid = Grid((8, 8, 8), (-2, -2, -2), (2, 2, 2))
    keep = []
    for f in range(5):
        for c, e in pairs:
            step(c, e, f, 70_000 if f == 0 else 3000, dt=1 / 60)
        if f >= 3:                                                       # no materialise call in front of it
            keep.append(run_binned(Export(fields, 20, cap), fx, g := grid.fresh()))
    ctx.synchronize()
    expected = expected_binned(fx, fields, 20, g)                        # the last frame's, against the read-back (which materialises for itself)
    assert len(expected[0]) == 70_000 + 4 * 3000 and len(np.unique(expected[0][:, 0])) == 5
    assert_binned(keep[-1], g, expected, "stale AGE")
    assert keep[0].counts() == [70_000 + 3 * 3000] * 2
    for f in range(5, 12):
        for c, e in pairs:
            step(c, e, f, 0, dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    d = fx.compare(twin)
    assert d["equal"] == 1, d
    assert fx.check()["ok"] == 1
    ctx.close(); tctx.close()


def test_binned_export_disturbs_nothing():
    cap = 10_000
    (ctx, fx), (tctx, twin) = burst_then_die_off(cap), burst_then_die_off(cap)
    ctx.synchronize()
    alive, dead = fx.alive_list().copy(), fx.dead_list().copy()
    grid = grid_around(fx, (8, 8, 8), inner=0.8)
    first = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    mid = run_binned(Export(POS_AGE_LIFE_VEL, 32, cap), fx, grid)
    second = Export(POS_AGE_LIFE_VEL, 32, cap).run(fx)
    ctx.synchronize()
    rec = expected_records(fx, POS_AGE_LIFE_VEL, 32)
    assert_export(first, rec, "plain export in front")
    assert_export(second, rec, "plain export behind: list order again")
    assert_binned(mid, grid, expected_binned(fx, POS_AGE_LIFE_VEL, 32, grid), "between them")
    np.testing.assert_array_equal(fx.alive_list(), alive)
    np.testing.assert_array_equal(fx.dead_list(), dead)
    for f in range(5, 25):
        for c, e in ((ctx, fx), (tctx, twin)):
            step(c, e, f, 300 if f % 4 == 0 else 0, dt=1 / 20)
    ctx.synchronize(); tctx.synchronize()
    d = fx.compare(twin)
    assert d["equal"] == 1, d
    ctx.close(); tctx.close()


def test_back_to_back_exports_with_different_grids_share_the_scratch_in_stream_order():
    """Different grids into different destinations and tables with no synchronisation between the calls; effects on both paths in one context."""
    ctx = bh.Context(0)
    fxs = []
    for cap in (TILE, 10_000):
        prog = ctx.create_program(bh.lower(effects.firework_trails(cap)))
        fxs += [prog.create_effect(), prog.create_effect()]
    for f, dt in ((0, 1 / 600), (1, 0.05)):
        ctx.frame_begin(dt, f * dt)
        for i, fx in enumerate(fxs):
            fx.set_frame((fx.capacity - 100 * i) if f == 0 else 0, frame_seed(i))
        ctx.simulate()
    ctx.synchronize()
    grids = [grid_around(fxs[0], (8, 8, 8)), grid_around(fxs[0], (1, 1, 1)), grid_around(fxs[0], (64, 64, 32), inner=0.5), grid_around(fxs[0], (17, 5, 3), inner=0.9)]
    runs = []
    for fx in fxs:                                                      # four exports per effect, sixteen in all, nothing waits in between
        for grid in grids:
            g = grid.fresh()
            runs.append((fx, g, run_binned(Export(POS_AGE_LIFE_VEL, 32, fx.capacity), fx, g)))
    ctx.synchronize()
    for fx, g, ex in runs:
        assert_binned(ex, g, expected_binned(fx, POS_AGE_LIFE_VEL, 32, g), f"capacity {fx.capacity}, effect {fx.index()}, {g.dims}")
    ctx.close()


@pytest.mark.parametrize("cap", [300, 4097])
def test_interleaved_with_the_sorted_and_the_filtered_export_on_one_effect(cap):
    from test_gpu_export_sorted import expected_sorted, run_sorted
    ctx, fx = make(cap)
    step(ctx, fx, 0, cap)
    step(ctx, fx, 1, 0, dt=0.05)
    grid = grid_around(fx, (8, 8, 8), inner=0.7)
    sort = dict(key="depth", v=(0.3, -0.5, 0.8))
    ctx.synchronize()
    p = positions(fx, fx.alive_list())
    sphere = (0.0, 0.0, 0.0, float(np.median((p.astype(np.float64) ** 2).sum(axis=1))))      # about half of the cloud
    runs = []
    for _ in range(2):                                                  # binned, sorted, filtered, binned, sorted, filtered: no synchronisation in between
        runs.append(("binned", g := grid.fresh(), run_binned(Export(POS_AGE_LIFE_VEL, 32, cap), fx, g)))
        runs.append(("sorted", None, run_sorted(Export(POS_AGE_LIFE_VEL, 32, cap), fx, **sort)))
        ex = Export(POS_AGE_LIFE_VEL, 32, cap)
        fx.export_filtered(ex.fields, ex.dst.data_ptr(), ex.stride, ex.capacity, ex.cnt.data_ptr(), kind="sphere", sphere=sphere)
        runs.append(("filtered", None, ex))
    ctx.synchronize()
    rec = expected_records(fx, POS_AGE_LIFE_VEL, 32)
    p = positions(fx, fx.alive_list())
    e = p - np.asarray(sphere[:3], F32)
    kept = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) <= F32(sphere[3])
    assert 0 < kept.sum() < cap
    for kind, g, ex in runs:
        if kind == "binned":
            assert_binned(ex, g, expected_binned(fx, POS_AGE_LIFE_VEL, 32, g), f"binned at {cap}")
        elif kind == "sorted":
            assert_export(ex, expected_sorted(fx, POS_AGE_LIFE_VEL, 32, **sort)[0], f"sorted at {cap}")
        else:
            assert_export(ex, rec[kept], f"filtered at {cap}")
    ctx.close()


def test_argument_errors_enqueue_nothing():
    """Every refusal of the contract but two: a layout without POSITION cannot be reached from here, because the lowering refuses an asset whose
    layout lacks POSITION - no program of that kind can be created to export from; and an effect of more than 0xFFFFFF00 slots does not fit a
    test (the launch plan's host test covers the layout that refuses it)."""
    cap = 1000
    ctx = bh.Context(0)
    fx = ctx.create_program(bh.lower(effects.firework_trails(cap))).create_effect()
    step(ctx, fx, 0, cap)
    ex = Export(POS_AGE_LIFE_VEL, 32, cap)
    grid = Grid((4, 4, 4), (-1, -1, -1), (2, 2, 2))
    ok = dict(dims=grid.dims, origin=grid.origin, inv_cell=grid.inv_cell, cell_start_ptr=grid.table.data_ptr())
    bad_desc = {       # every case hnb_effect_export_sorted rejects in desc
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
    for what, kw in bad_desc.items():
        with pytest.raises(bh.HanabiError) as ei:
            fx.export_binned(kw.get("fields", POS_AGE_LIFE_VEL), kw.get("dst", ex.dst.data_ptr()), kw.get("stride", 32), cap, ex.cnt.data_ptr(), **ok)
        assert ei.value.code == -1 and len(str(ei.value)) > 8, what
    inf, nan = float("inf"), float("nan")
    bad_bins = {
        "a dimension of 0": dict(dims=(4, 0, 4)),
        "another dimension of 0": dict(dims=(0, 4, 4)),
        "more than 2^24 cells": dict(dims=(1 << 24, 2, 1)),
        "a product that is 0 modulo 2^32": dict(dims=(65536, 65536, 65536)),
        "a product that wraps to a small number": dict(dims=(0x80000001, 2, 1)),
        "an infinite origin": dict(origin=(0, inf, 0)),
        "a NaN origin": dict(origin=(nan, 0, 0)),
        "an infinite inv_cell": dict(inv_cell=(1, 1, inf)),
        "a NaN inv_cell": dict(inv_cell=(1, nan, 1)),
        "an inv_cell of 0": dict(inv_cell=(0.0, 1, 1)),
        "an inv_cell of -0": dict(inv_cell=(1, -0.0, 1)),
        "a negative inv_cell": dict(inv_cell=(1, 1, -2.0)),
        "cell_start NULL": dict(cell_start_ptr=0),
        "cell_start not 16-byte aligned": dict(cell_start_ptr=grid.table.data_ptr() + 4),
    }
    for what, kw in bad_bins.items():
        with pytest.raises(bh.HanabiError) as ei:
            fx.export_binned(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, cap, ex.cnt.data_ptr(), **{**ok, **kw})
        assert ei.value.code == -1 and "HnbExportBins" in str(ei.value), what
    lib = runtime.load_library()
    d = runtime.export_desc(POS_AGE_LIFE_VEL, ex.dst.data_ptr(), 32, cap, ex.cnt.data_ptr())
    g = runtime.export_bins(grid.dims, grid.origin, grid.inv_cell, grid.table.data_ptr())
    assert lib.hnb_effect_export_binned(fx._h, C.byref(d), None) == -1 and lib.hnb_effect_export_binned(fx._h, None, C.byref(g)) == -1
    assert lib.hnb_effect_export_binned(None, C.byref(d), C.byref(g)) == -1
    for field, value in (("struct_size", 52), ("struct_size", 64), ("flags", 1), ("reserved", 1)):
        keep = getattr(g, field)
        setattr(g, field, value)
        assert lib.hnb_effect_export_binned(fx._h, C.byref(d), C.byref(g)) == -1 and len(lib.hnb_last_error()) > 8, field
        setattr(g, field, keep)
    for field, value in (("struct_size", 64), ("flags", 1)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert lib.hnb_effect_export_binned(fx._h, C.byref(d), C.byref(g)) == -1, field
        setattr(d, field, keep)
    ctx.synchronize()
    assert ex.untouched() and (grid.words() == SENTINEL).all()
    assert lib.hnb_effect_export_binned(fx._h, C.byref(d), C.byref(g)) == 0       # ... and the same arguments, unbroken, are accepted
    ctx.synchronize()
    assert ex.counts() == [cap, cap]
    assert_binned(ex, grid, expected_binned(fx, POS_AGE_LIFE_VEL, 32, grid), "after the refusals")
    ctx.close()
