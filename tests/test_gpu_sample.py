"""hnb_effect_sample on the GPU (include/hanabi_amd_sample.h): up to four channels of an f32 grid field on the device - the particle's cell or the
trilinear blend of the eight cell centres around it - scaled and stored or added into components of f32 attributes. The expectation is always the
numpy restatement (tests/test_sample_abi.py np_sample / np_store) over the host's read-back of the planes and the alive list, compared bit for bit
over WHOLE planes (dead slots, outside particles and unnamed components included); where the restatement gives a NaN the result must be a NaN. There
is no tolerance anywhere. The field and the stats sit between guard words filled with a sentinel. Before comparing, each main case asserts on the
restatement alone that a no-op or a nearest-for-trilinear kernel cannot pass (guard_conditions)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, runtime
from helpers import A
from test_bounds_abi import trails_vec4
from test_gpu_bounds import run as run_bounds
from test_gpu_export import POS_AGE_LIFE_VEL, SENTINEL, Export, step
from test_gpu_export_binned import Grid as BinGrid, run_binned
from test_gpu_import import alive_mask, make, planes, run_stretch
from test_sample_abi import ADD, NEAREST, SET, TILE, TRILINEAR, np_sample, np_store, same_bits_or_both_nan, sample_plan

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
GUARD = 4                                        # words on both sides of the field and of the stats: 16 bytes, the alignment stays
HALF = 8.0                                       # the grids span [-HALF, HALF)^3
CAPS = (255, 300, 4096, 4097, 3 * 4096 + 5, 300_007)
MODES = (NEAREST, TRILINEAR)
ATTRS4 = [A.POSITION.id, A.VELOCITY.id, A.AGE.id, A.LIFETIME.id, A.F32X4_0.id]          # trails_vec4's layout, every plane of it
# a component of a 3-vector, the last of a 4-vector, a scalar, POSITION itself; SET and ADD mixed
CH4 = [(A.VELOCITY.id, 1, ADD), (A.F32X4_0.id, 3, SET), (A.LIFETIME.id, 0, ADD), (A.POSITION.id, 2, SET)]


class Field:
    """The field of one call - values [n_cells (+ tail_rows), k] - and the stats, each between guard words; everything else the sentinel"""

    def __init__(self, dims, values, stats=True, origin=(-HALF,) * 3, inv_cell=None, tail_rows=0):
        self.dims = tuple(int(d) for d in dims)
        self.n_cells = self.dims[0] * self.dims[1] * self.dims[2]
        self.origin = np.asarray(origin, F32)
        self.inv_cell = np.asarray(inv_cell if inv_cell is not None else [d / (2 * HALF) for d in self.dims], F32)
        self.values = np.ascontiguousarray(values, F32).reshape(self.n_cells + tail_rows, -1)
        self.k = self.values.shape[1]
        words = np.full(self.values.size + 2 * GUARD, SENTINEL, np.int64).astype(U32)
        words[GUARD: GUARD + self.values.size] = self.values.reshape(-1).view(U32)
        self.words = words
        self.buf = torch.from_numpy(words.view(np.int32)).cuda()
        self.stats = torch.full((4 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda") if stats else None
        torch.cuda.synchronize()                 # (the copies run on torch's stream, the call on the simulation's)

    def args(self):
        return dict(dims=self.dims, origin=self.origin, inv_cell=self.inv_cell, field_ptr=self.buf.data_ptr() + 4 * GUARD,
                    stats_ptr=self.stats.data_ptr() + 4 * GUARD if self.stats is not None else None)

    def cells(self):
        return self.values[: self.n_cells]

    def read_stats(self):
        """-> the four stats, and asserts the guard words on both sides of them and the whole field buffer: the call only reads it"""
        np.testing.assert_array_equal(self.buf.cpu().numpy().view(U32), self.words, err_msg="the field or the words next to it were written")
        if self.stats is None:
            return None
        raw = self.stats.cpu().numpy().view(U32)
        assert (raw[:GUARD] == U32(SENTINEL & 0xFFFFFFFF)).all() and (raw[GUARD + 4:] == U32(SENTINEL & 0xFFFFFFFF)).all(), "words next to out_stats were written"
        return raw[GUARD: GUARD + 4]

    def untouched(self):
        ok = bool((self.buf.cpu().numpy().view(U32) == self.words).all())
        return ok and (self.stats is None or bool((self.stats.cpu().numpy().view(U32) == U32(SENTINEL & 0xFFFFFFFF)).all()))


def random_field(dims, k, seed, special=False, tail_rows=0):
    rng = np.random.default_rng(seed)
    n = dims[0] * dims[1] * dims[2]
    v = rng.normal(0, 3, (n + tail_rows, k)).astype(F32)
    if special:                                  # an infinity, a NaN and denormals among the cells
        idx = rng.permutation(n)
        bad = np.array([np.inf, np.nan, 1e-40, -1e-45, -np.inf, -0.0], F32)
        for i, b in zip(idx, bad):
            v[i, rng.integers(k)] = b
    if tail_rows:
        v[n:] = np.nan                           # the deposit's outside row: never read
    return v


def plant(fx, seed, dims, vec4=True):
    """Values over the whole capacity, written with hnb_effect_write_attr: positions uniform in 1.05 of the grid's half-width - a part of them
    outside - and two fifths of them moved into the outer half cell along one axis, where a corner of the trilinear stencil clamps"""
    rng = np.random.default_rng(seed)
    cap = fx.capacity
    pos = rng.uniform(-1.05 * HALF, 1.05 * HALF, (cap, 3))
    edge = np.flatnonzero(rng.random(cap) < 0.4)
    axis = rng.integers(3, size=len(edge))
    half_cell = HALF / np.asarray(dims, np.float64)[axis]
    pos[edge, axis] = rng.choice([-1.0, 1.0], len(edge)) * (HALF - rng.uniform(0.02, 0.98, len(edge)) * half_cell)
    fx.write_attr(A.POSITION.id, pos.astype(F32))
    fx.write_attr(A.VELOCITY.id, rng.normal(0, 30, (cap, 3)).astype(F32))
    if vec4:
        fx.write_attr(A.F32X4_0.id, rng.normal(0, 4, (cap, 4)).astype(F32))


def expected(fx, fld, channels, mode, scale, attrs):
    """The restatement over the host's read-back of the effect as it is (synchronises). -> (before, want: attribute -> [capacity, ncomp] words;
    stats [4]; info: the masks the guard conditions are stated on)"""
    before = planes(fx, attrs)
    alive = alive_mask(fx)
    pos = before[int(A.POSITION.id)].view(F32)
    inside, s, clamped = np_sample(pos, fld.cells(), fld.dims, fld.origin, fld.inv_cell, mode)
    wr = alive & inside
    want = {a: p.copy() for a, p in before.items()}
    nan = {a: np.zeros(p.shape, bool) for a, p in before.items()}
    for k, (attr, comp, op) in enumerate(channels):
        out = np_store(op, before[int(attr)][:, comp].view(F32), s[:, k], scale)
        want[int(attr)][wr, comp] = out.view(U32)[wr]
        nan[int(attr)][wr, comp] = np.isnan(out[wr])
    changed = np.zeros(fx.capacity, bool)
    for a in before:
        changed |= (before[a] != want[a]).any(axis=1)
    stats = np.array([alive.sum(), wr.sum(), (alive & ~inside).sum(), 0], np.uint64).astype(U32)
    return before, want, stats, dict(alive=alive, wr=wr, clamped=alive & clamped, changed=changed, nan=nan)


def guard_conditions(info):
    """On the restatement alone: a no-op, or a nearest kernel in place of the trilinear one, can never pass for the case"""
    alive, wr = int(info["alive"].sum()), int(info["wr"].sum())
    assert alive > 0 and 4 * int(info["clamped"].sum()) >= alive, "at least a quarter of the alive particles are sampled with a clamped corner"
    assert alive - wr > 0, "the outside bin is not empty"
    assert 2 * int((info["changed"] & info["wr"]).sum()) > wr, "more than half of the sampled particles change a destination's bits"
    assert not (info["changed"] & ~info["wr"]).any()


def assert_planes(fx, want, info, what):
    """every plane, whole: the expected bits everywhere; where a NaN is expected, a NaN"""
    got = planes(fx, list(want))
    for a, w in want.items():
        ok = (got[a] == w) | (info["nan"][a] & np.isnan(got[a].view(F32)))
        bad = np.argwhere(~ok)
        assert not len(bad), (what, f"attribute {a}", len(bad), [(int(s), int(c), hex(int(got[a][s, c])), hex(int(w[s, c])), bool(info["alive"][s]), bool(info["wr"][s])) for s, c in bad[:6]])


def check_sample(ctx, fx, fld, channels, mode, scale, what, attrs=ATTRS4, guards=True):
    """one call against the restatement: planes, stats, guard words -> (want, stats, info)"""
    before, want, stats, info = expected(fx, fld, channels, mode, scale, attrs)
    if guards:
        guard_conditions(info)
    fx.sample(channels=channels, mode=mode, scale=scale, **fld.args())
    ctx.synchronize()
    assert_planes(fx, want, info, what)
    got = fld.read_stats()
    if got is not None:
        np.testing.assert_array_equal(got, stats, err_msg=f"{what}: out_stats")
    return want, stats, info


# ---- capacities: dead slots interleaved, the tail quad, whole-dead quads, a partial last tile, several tiles; both kernels ------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_capacities_all_alive_and_after_a_die_off(cap):
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    dims = (5, 4, 3)
    for state in ("all alive", "after a die-off"):
        if state == "after a die-off":
            fx.write_attr(A.VELOCITY.id, np.zeros((cap, 3), F32))
            fx.write_attr(A.LIFETIME.id, np.random.default_rng(cap).uniform(0.8, 1.2, cap).astype(F32))       # (the calls above added to it)
            for f in range(1, 5):                                          # lifetimes are 0.8 .. 1.2 s: a second later part of the burst is gone
                step(ctx, fx, f, 0, dt=0.25)
        for mode in MODES:
            plant(fx, cap + mode, dims)
            fld = Field(dims, random_field(dims, 4, cap + 7 * mode))
            assert sample_plan(mode, cap)[1] == -(-cap // TILE)
            _, stats, info = check_sample(ctx, fx, fld, CH4, mode, -0.25, f"capacity {cap}, {state}, mode {mode}")
            n = fx.alive_count()
            assert stats[0] == n and (n == cap if state == "all alive" else 0 < n < cap), (state, n)
    fx.write_attr(A.LIFETIME.id, np.full(cap, 5.0, F32))                   # (the calls added to the lifetimes: age < lifetime is the verifier's, not the call's)
    assert fx.check()["ok"] == 1                                           # lists, alive bytes and counters are as the frames left them
    ctx.close()


# ---- grids ----------------------------------------------------------------------------------------------------------------------------------------
GRIDS = [((1, 1, 1), 4097), ((2, 1, 7), 4097), ((5, 4, 3), 4097), ((64, 64, 64), 40_000)]


@pytest.mark.parametrize("dims,cap", GRIDS, ids=["x".join(str(i) for i in g[0]) for g in GRIDS])
def test_grids(dims, cap):
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    for mode in MODES:
        plant(fx, 31 * dims[0] + mode, dims)
        fld = Field(dims, random_field(dims, 4, dims[2]))
        want, _, info = check_sample(ctx, fx, fld, CH4, mode, 2.0, f"{dims}, mode {mode}")
        if dims == (1, 1, 1):                                              # every corner clamps: the sample is field[0], exactly, in both modes
            wr = info["wr"]
            assert info["clamped"].sum() == wr.sum() > 0
            assert (want[int(A.F32X4_0.id)][wr, 3] == (fld.cells()[0, 1] * F32(2.0)).view(U32)).all()
            assert (want[int(A.POSITION.id)][wr, 2] == (fld.cells()[0, 3] * F32(2.0)).view(U32)).all()
    ctx.close()


def test_one_to_four_channels_on_one_state_and_a_frozen_instance():
    cap, dims = 10_000, (5, 4, 3)
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    for f in range(1, 5):
        step(ctx, fx, f, 0, dt=0.25)
    fx.set_simulated(False)                                                # frozen instances accept the call
    step(ctx, fx, 5, 0, dt=0.25)
    dests = [(A.VELOCITY.id, 0, ADD), (A.VELOCITY.id, 2, SET), (A.F32X4_0.id, 0, ADD), (A.LIFETIME.id, 0, SET)]
    for k in range(1, 5):
        for mode in MODES:
            plant(fx, 10 * k + mode, dims)
            # a deposit-shaped tensor: the outside row is still on it, holds NaNs, and is never read
            fld = Field(dims, random_field(dims, k, k, tail_rows=1), tail_rows=1)
            _, stats, _ = check_sample(ctx, fx, fld, dests[:k], mode, 1.0, f"{k} channels, mode {mode}")
            assert 0 < stats[0] < cap
    ctx.close()


def test_position_itself_is_read_before_it_is_stored_all_three_components():
    cap, dims = 4097, (5, 4, 3)
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    ch = [(A.POSITION.id, 0, SET), (A.POSITION.id, 1, ADD), (A.POSITION.id, 2, SET), (A.VELOCITY.id, 1, SET)]
    for mode in MODES:
        plant(fx, 5 + mode, dims)
        check_sample(ctx, fx, Field(dims, random_field(dims, 4, 99)), ch, mode, 0.5, f"POSITION as a destination, mode {mode}")
    ctx.close()


# ---- edge values ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES, ids=["nearest", "trilinear"])
def test_edge_positions_and_edge_field_values(mode):
    cap, dims = 300, (4, 4, 4)                                             # cells of edge 4 over [-8, 8)^3
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    rng = np.random.default_rng(3)
    pos = rng.uniform(-HALF, 0.999 * HALF, (cap, 3)).astype(F32)
    pos[0] = (np.nan, 0, 0); pos[1] = (0, np.inf, 0); pos[2] = (0, 0, -np.inf)           # outside
    pos[3] = (-HALF, -0.0, -HALF)                                                         # the lowest corner: inside; two axes clamp
    pos[4] = (-HALF + 4.0, 0, 0); pos[5] = (np.nextafter(F32(-HALF + 4.0), F32(-100)), 0, 0)      # on a cell face; one ulp below
    pos[6] = (np.nextafter(F32(-HALF), F32(-100)), 0, 0)                                  # one ulp outside
    pos[7] = (0, 0, -0.0)
    pos[8] = (-HALF + 2.0, -HALF + 6.0, -HALF + 10.0)                                     # cell centres: w = 0 on every axis
    pos[9] = (np.nextafter(F32(-HALF + 2.0), F32(-100)), np.nextafter(F32(-HALF + 2.0), F32(100)), HALF - 2.0)      # either side of t = 0.5; t = dims - 0.5
    pos[10] = (F32(HALF - 2.0 ** -20), np.nextafter(F32(HALF - 2.0), F32(100)), np.nextafter(F32(HALF - 2.0), F32(-100)))      # x + 8 = 16 - 2^-20, exactly: the last t inside
    pos[11] = (HALF, 0, 0)                                                                # the upper end: outside
    pos[12] = (-2.0, -2.0, -2.0)                                                          # the centre of cell 21, whose first channel is a NaN
    pos[13] = (np.nextafter(F32(HALF), F32(-100)), 0, 0)                                  # 8 - 2^-21 is below the end, but x + 8 rounds to 16: t = 4, outside
    fx.write_attr(A.POSITION.id, pos)
    vel = rng.normal(0, 30, (cap, 3)).astype(F32)
    vel[12:40:3, 1] = F32(1e-41); vel[13:40:3, 1] = F32(-0.0); vel[14:40:3, 1] = F32(np.inf)
    fx.write_attr(A.VELOCITY.id, vel)
    values = random_field(dims, 2, 11)
    values[0, 0] = np.inf; values[21, 0] = np.nan; values[42, 0] = -np.inf; values[63, 1] = np.nan
    values[5, 1] = 1e-40; values[6, 1] = -1e-45; values[22, 0] = 1e-39; values[41, 1] = -0.0
    ch = [(A.VELOCITY.id, 1, ADD), (A.LIFETIME.id, 0, SET)]
    for scale in (1.0, 2.0 ** -140):                                       # the second: every finite s * scale is a denormal or a zero
        fld = Field(dims, values)
        want, stats, info = check_sample(ctx, fx, fld, ch, mode, scale, f"edge values, mode {mode}, scale {scale}", guards=False)
        assert stats[2] == 6 and list(info["wr"][:14]) == [False, False, False, True, True, True, False, True, True, True, True, False, True, False]
        n_nan = sum(int(v.sum()) for v in info["nan"].values())
        life = want[int(A.LIFETIME.id)][info["wr"], 0].view(F32)
        assert n_nan > 0 and (scale == 1.0 or ((np.abs(life) < F32(1.1754944e-38)) & (life != 0)).any()), "NaN results and denormal results are among the expectations"
        fx.write_attr(A.VELOCITY.id, vel)
    ctx.close()


# ---- stats, nothing alive -------------------------------------------------------------------------------------------------------------------------------
def test_out_stats_null_is_accepted():
    cap, dims = 4097, (5, 4, 3)
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    for mode in MODES:
        plant(fx, 9 + mode, dims)
        check_sample(ctx, fx, Field(dims, random_field(dims, 4, 4), stats=False), CH4, mode, 1.0, f"no out_stats, mode {mode}")
    ctx.close()


@pytest.mark.parametrize("cap", [300, 10_000])
def test_nothing_alive_writes_nothing_and_leaves_zero_stats(cap):
    dims = (5, 4, 3)
    ctx, fx = make(cap, trails_vec4(cap))
    fields = [Field(dims, random_field(dims, 4, m)) for m in range(4)]
    for mode in MODES:                                                     # before the first frame
        fx.sample(channels=CH4, mode=mode, **fields[mode].args())
    step(ctx, fx, 0, cap)
    plant(fx, 1, dims)
    for f in range(1, 5):
        step(ctx, fx, f, 0, dt=0.5)                                        # every lifetime is over
    ctx.synchronize()
    before = planes(fx, ATTRS4)
    for mode in MODES:
        fx.sample(channels=CH4, mode=mode, **fields[2 + mode].args())
    ctx.synchronize()
    assert fx.alive_count() == 0
    after = planes(fx, ATTRS4)
    for a in before:
        np.testing.assert_array_equal(after[a], before[a])
    for fld in fields:
        assert list(fld.read_stats()) == [0, 0, 0, 0]
    ctx.close()


# ---- the state after the call -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dest", ["LIFETIME", "VELOCITY"])
def test_later_frames_compute_what_they_would_after_write_attr(dest):
    """70,000 slots, past the 65,536 threshold of HNB_AGE_COHORT_AUTO. Frames publish the chunks' lifetime bounds and death horizons; the sample then
    stores lifetimes shorter than those bounds, so particles die from the next frames on (or adds to the velocities). The twin gets the same planes
    through hnb_effect_write_attr. Both run 30 frames, 8 of them through hnb_simulate_steps; every plane, list and counter must agree - which they
    do not when the call leaves the cached bounds standing."""
    cap, dims = 70_000, (5, 4, 3)
    asset = effects.firework_trails(cap)
    (ca, fa), (cb, fb) = [make(cap, age_cohort=3) for _ in range(2)]
    for f in range(6):
        for c, fx in ((ca, fa), (cb, fb)):
            step(c, fx, f, cap if f == 0 else 0, dt=1 / 30)
    rng = np.random.default_rng(4)
    n = dims[0] * dims[1] * dims[2]
    if dest == "LIFETIME":
        values = rng.uniform(0.31, 0.9, (n, 1)).astype(F32)              # from 0.31 s: below the bound of 0.8 s every chunk published
        values[::7] = F32(0.05)                                            # ... and some cells kill at once: age >= lifetime in the next update
        ch, attr = [(A.LIFETIME.id, 0, SET)], A.LIFETIME.id
    else:
        values = rng.normal(0, 20, (n, 3)).astype(F32)
        ch, attr = [(A.VELOCITY.id, 0, ADD), (A.VELOCITY.id, 1, ADD), (A.VELOCITY.id, 2, ADD)], A.VELOCITY.id
    ca.synchronize()
    pos = fa.read_attr(A.POSITION.id).reshape(-1, 3)
    lo, hi = pos.min(axis=0), pos.max(axis=0)                              # the burst's box, a little narrower: some particles are outside
    origin = lo + 0.02 * (hi - lo)
    fld = Field(dims, values, origin=origin, inv_cell=np.asarray(dims) / (0.96 * (hi - lo)))
    fa.sample(channels=ch, mode=TRILINEAR, **fld.args())                   # no synchronisation in front or behind
    fb.write_attr(int(attr), fa.read_attr(int(attr)))                      # (the read-back waits for the call)
    stats = fld.read_stats()
    assert stats[0] == cap and 0 < stats[2] < stats[1]
    for c, fx in ((ca, fa), (cb, fb)):
        step(c, fx, 6, 0, dt=1 / 30)
    alive = fa.alive_count()                                               # the cells of 0.05 s killed their particles in this frame, the others live on
    assert alive == fb.alive_count() and ((0 < alive < cap) if dest == "LIFETIME" else alive == cap), alive
    run_stretch([(ca, fa), (cb, fb)], 7, asset, f"sampled {dest}")
    assert fa.alive_count() < alive and fa.check()["ok"] == 1              # particles died on the way, in both
    ca.close(); cb.close()


# ---- the loop the call closes: deposit -> a torch op on the grid -> sample ------------------------------------------------------------------------------
def test_ten_rounds_of_deposit_torch_and_sample_between_frames_a_binned_export_and_a_bounds_call():
    cap, dims = 10_000, (8, 8, 8)
    n_cells = 512
    ctx, fx = make(cap, trails_vec4(cap))
    b = dict(origin=np.full(3, -3.0, F32), inv_cell=np.full(3, 8 / 6.0, F32))       # [-3, 3)^3: part of the burst leaves it
    count = torch.zeros(n_cells + 1, dtype=torch.int32, device="cuda")
    sums = torch.zeros((n_cells + 1, 2), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ch = [(A.VELOCITY.id, 0, ADD), (A.F32X4_0.id, 2, SET)]
    others = []                                                            # (their destinations stay allocated until the stream has run them)
    sampled = 0
    for r in range(10):
        step(ctx, fx, r, cap if r == 0 else 0, dt=1 / 600 if r == 0 else 0.02)
        fx.deposit(dims, b["origin"], b["inv_cell"], count.data_ptr(), [(A.VELOCITY.id, 0, 12), (A.VELOCITY.id, 1, 12)], sums.data_ptr())
        grid = BinGrid(dims, b["origin"], b["inv_cell"])
        others.append((run_binned(Export(POS_AGE_LIFE_VEL, 32, cap), fx, grid), grid, run_bounds(fx, A.POSITION.id)))
        ctx.synchronize()                                                  # the torch op runs on torch's stream
        grid_f = sums.to(torch.float32) * (2.0 ** -12 * -0.01)             # scale it: a drag towards the cell's mean velocity ...
        grid_f = torch.roll(grid_f, shifts=1, dims=0).contiguous()         # ... roll it: the outside row comes first, the last cell's row goes last
        torch.cuda.synchronize()
        mode = MODES[r % 2]
        fld = Field(dims, grid_f.cpu().numpy(), tail_rows=1, **b)
        before, want, stats, info = expected(fx, fld, ch, mode, 0.5, ATTRS4)
        fx.sample(dims, b["origin"], b["inv_cell"], grid_f.data_ptr(), ch, mode, 0.5, fld.stats.data_ptr() + 4 * GUARD)      # the torch tensor itself
        ctx.synchronize()
        assert_planes(fx, want, info, f"round {r}, mode {mode}")
        np.testing.assert_array_equal(fld.read_stats(), stats)
        sampled += int((info["changed"] & info["wr"]).sum())
    assert sampled > cap and 0 < stats[2] and fx.check()["ok"] == 1
    ctx.close()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing():
    """Every refusal of the contract but a layout without POSITION, which the stand-alone program of tests/test_sample_abi.py holds"""
    cap, dims = 5000, (4, 4, 4)
    ctx, fx = make(cap, trails_vec4(cap))
    step(ctx, fx, 0, cap)
    plant(fx, 1, dims)
    lib = runtime.load_library()
    fld = Field(dims, random_field(dims, 2, 1))
    ch = [(A.VELOCITY.id, 1, ADD), (A.LIFETIME.id, 0, SET)]
    good = lambda: runtime.sample_desc(channels=ch, mode=TRILINEAR, scale=1.0, **fld.args())
    nan, inf = float("nan"), float("inf")
    ctx.synchronize()
    before = planes(fx, ATTRS4)

    def refused(desc, text):
        assert lib.hnb_effect_sample(fx._h, C.byref(desc)) == -1, text
        assert text.encode() in lib.hnb_last_error(), (text, lib.hnb_last_error())

    assert lib.hnb_effect_sample(None, C.byref(good())) == -1 and b"NULL" in lib.hnb_last_error()
    assert lib.hnb_effect_sample(fx._h, None) == -1 and b"NULL" in lib.hnb_last_error()
    x = good(); x.struct_size = 132
    refused(x, "struct_size")
    x = good(); x.flags = 1
    refused(x, "flags: 0")
    x = good(); x.mode = 2
    refused(x, "mode: HNB_SAMPLE_NEAREST or")
    for d in ((0, 4, 4), (4096, 4096, 2)):
        x = good(); x.dims = (C.c_uint32 * 3)(*d)
        refused(x, "HNB_BIN_MAX_CELLS")
    x = good(); x.origin[1] = nan
    refused(x, "origin is not finite")
    for bad in (0.0, -1.0, inf, nan):
        x = good(); x.inv_cell[2] = bad
        refused(x, "inv_cell is not finite and above 0")
    for n in (0, 5):
        x = good(); x.n_channels = n
        refused(x, "n_channels is not 1..")
    for attr in (A.AGE.id, A.COLOR.id, A.SIZE3.id, A.ID.id, 9999):         # AGE; not in this layout (COLOR, SIZE3); not stored; no attribute
        x = good(); x.channels[1].attr = attr
        refused(x, "channels[1]")
        assert b"not an f32 attribute" in lib.hnb_last_error()
    x = good(); x.channels[0].comp = 3
    refused(x, "comp is at or past")
    x = good(); x.channels[1].op = 2
    refused(x, "op: HNB_SAMPLE_SET or")
    x = good(); x.channels[1].reserved = 1
    refused(x, "reserved is not 0")
    x = good(); x.channels[1] = runtime.SampleChannel(int(A.VELOCITY.id), 1, SET, 0)
    refused(x, "an earlier channel's")
    x = good(); x.channels[3].op = 1
    refused(x, "at or past n_channels")
    for bad in (nan, inf, -inf):
        x = good(); x.scale = bad
        refused(x, "scale is not finite")
    x = good(); x.field = None
    refused(x, "field: a 16-byte aligned")
    x = good(); x.field = fld.buf.data_ptr() + 4 * GUARD + 8
    refused(x, "field: a 16-byte aligned")
    x = good(); x.out_stats = fld.stats.data_ptr() + 4
    refused(x, "out_stats: NULL or")
    ctx.synchronize()
    assert fld.untouched()
    after = planes(fx, ATTRS4)
    for a in before:
        np.testing.assert_array_equal(after[a], before[a])
    check_sample(ctx, fx, fld, ch, TRILINEAR, 1.0, "a good call behind the refusals")        # ... and the same destination takes a good call
    ctx.close()
