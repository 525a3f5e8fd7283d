"""The ribbon sort (hnb_sort.hip.h) driven directly: chosen keys, every launch path of enqueue_ribbon_sort.

The other ribbon tests feed the sort keys that fall out of a simulation (a few thousand particles, a handful of ribbon ids, small
non-negative ages). Here the host writes the RIBBON_ID and AGE planes (tests/ribbon_keys.py: the patterns and the numpy model,
tied to the oracle without a GPU by tests/test_ribbon_sort_model.py), one frame runs, and the alive list is compared bit for bit with

  * the oracle's list (a stable merge sort on (RIBBON_ID, AGE bits)), and
  * numpy's stable argsort on the 64-bit keys of the planes READ BACK from the GPU after the frame,

at the smallest capacities at which each mechanism exists (ROWS below), with three instances per program sorted by the same launches:
one empty (or sparse), one partly filled, one full. Every case asserts from Program.kernel_info() ("ribbon sorts by path") that the
frame took the path its row names: a later change to the dispatch condition fails here instead of quietly turning the rows into
copies of one another.

Exceptions to "bit for bit against the oracle", the only ones: the pattern `nan_ages` writes quiet NaNs (0x7FC00000 | payload, both
signs) into a tenth of the ages, and is checked against the numpy model on the GPU's own planes, not against the oracle: the payload
of a NaN that went through an addition differs between x86 and gfx950 (helpers._both_nan). Those particles die in the frame (NaN <
lifetime is false), so what the pattern adds is a sort behind a compaction that removed every tenth row.

Cost: one program per capacity (module fixture, created once: its run-time specialisation is the fixture's one-time cost); a case at
266,240 slots steps three oracle instances of up to that size, which is most of its second or two.
"""
import re

import numpy as np
import pytest

import bevy_hanabi_amd as bh
import ribbon_keys as rk
from helpers import A, OracleRunner

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
PATHS = ("one-tile", "one-workgroup", "multi-launch")

# row -> (capacity, alive counts of the three instances, the path enqueue_ribbon_sort takes for a list it cannot prove anything about)
ROWS = {
    "tile1": (4096, (0, 257, 4096), "one-tile"),                        # k_sort_tile1: capacity <= kSortTile
    "tile1_tiny": (4096, (1, 64, 65), "one-tile"),                      # one row; one wave exactly; one wave and a row
    "one_workgroup": (16384, (0, 4097, 16384), "one-workgroup"),        # k_sort_fill + k_sort_small + k_sort_merge: capacity <= kSortSmallMax / 4
    "multi_one_group": (20480, (0, 16385, 20480), "multi-launch"),      # 5 tiles: k_sort_hist / k_sort_scatter, one group of tiles
    "multi_three_groups": (266240, (131072, 131073, 266240), "multi-launch"),   # 65 tiles: exactly one group, one group and a row, three groups
}


class Rig:
    """One context and one program of the sort asset per capacity; the instances come and go with the cases."""

    def __init__(self, cap):
        self.cap = cap
        self.asset = rk.sort_asset(cap)
        self.ctx = bh.Context(0)
        self.prog = self.ctx.create_program(bh.lower(self.asset))
        self.seed = 0x51DE

    def instances(self, n=3):
        return [(self.prog.create_effect(), OracleRunner(self.asset)) for _ in range(n)]

    def step(self, insts, dt, spawns, props=None):
        """One frame of every instance, on the GPU (one hnb_simulate: the instances share every launch) and in the oracles."""
        self.seed += 16
        self.ctx.frame_begin(dt, 0.0)
        for i, ((fx, orc), spawn) in enumerate(zip(insts, spawns)):
            for k, v in (props or {}).items():
                fx.set_property(k, v)
                orc.fx.set_property(k, v)
            fx.set_frame(spawn, self.seed + i)
            orc.fx.step(dt, spawn, self.seed + i)
        self.ctx.simulate()

    def paths(self):
        line = [l for l in self.prog.kernel_info().split("\n") if l.startswith("ribbon sorts by path:")]
        assert len(line) == 1, self.prog.kernel_info()
        m = re.fullmatch(r"ribbon sorts by path: one-tile (\d+), one-workgroup (\d+), multi-launch (\d+) frames", line[0])
        assert m, line[0]
        return dict(zip(PATHS, (int(x) for x in m.groups())))

    def ran(self, before):
        """The paths of the sorts since `before`, as {path: frames} without the zeros."""
        now = self.paths()
        return {p: now[p] - before[p] for p in PATHS if now[p] != before[p]}

    @staticmethod
    def release(insts):
        for fx, orc in insts:
            fx.destroy()
            orc.fx.close()


_rigs = {}


@pytest.fixture(scope="module")
def rig():
    def get(cap):
        if cap not in _rigs:
            _rigs[cap] = Rig(cap)
        return _rigs[cap]
    yield get
    for r in _rigs.values():
        r.ctx.close()
    _rigs.clear()


def _burst(r, insts, ns, a0=0.5):
    """Spawn ns[i] particles with one key for all (k = 1, one age): the list is in spawn order and the first sort has nothing to move."""
    r.step(insts, 0.0, ns, props={"a0": np.float32(a0), "k": np.array([1], np.uint32)})
    lists = []
    for (fx, orc), n in zip(insts, ns):
        before = fx.alive_list()
        assert len(before) == n
        np.testing.assert_array_equal(before, orc.fx.alive_list())
        lists.append(before)
    return lists


def _write_keys(r, fx, orc, before, rid, age_bits):
    rp, ap, lp = rk.planes(r.cap, before, rid, age_bits)
    for t in (fx, orc.fx):
        t.write_attr(A.RIBBON_ID.id, rp)
        t.write_attr(A.AGE.id, ap.view(np.float32))
        t.write_attr(A.LIFETIME.id, lp.view(np.float32))
    return rp, ap, lp


def _check_sorted(fx, orc, rows, what, against_oracle=True):
    """The GPU list against the numpy model on the GPU's own planes (`rows`: the alive rows in the order the sort received them, None = take the
    model's answer from the oracle only) and against the oracle, planes included. Returns the GPU's (list, rid plane, age bits plane)."""
    assert fx.metadata()["fault"] == 0, what
    got = fx.alive_list()
    rid_after = fx.read_attr(A.RIBBON_ID.id)
    age_after = fx.read_attr(A.AGE.id).view(np.uint32)
    if rows is not None:
        want = rk.expected_list(rows, rid_after, age_after)
        if not np.array_equal(got, want):
            first = int(np.argmax(got != want)) if len(got) == len(want) else -1
            raise AssertionError(f"{what}: list differs from the stable argsort of the read-back keys: lengths {len(got)} / {len(want)}, first differing row {first} "
                                 f"(tile {first // 4096}, group {first // (4096 * 32)}), {int((got != want).sum()) if first >= 0 else '?'} rows differ")
    if against_oracle:
        ref = orc.fx.alive_list()
        if not np.array_equal(got, ref):
            first = int(np.argmax(got != ref)) if len(got) == len(ref) else -1
            raise AssertionError(f"{what}: list differs from the oracle's: lengths {len(got)} / {len(ref)}, first differing row {first} (tile {first // 4096}, group {first // (4096 * 32)})")
        np.testing.assert_array_equal(rid_after, orc.fx.read_attr(A.RIBBON_ID.id), err_msg=f"{what}: RIBBON_ID plane")
        np.testing.assert_array_equal(age_after, orc.fx.read_attr(A.AGE.id).view(np.uint32), err_msg=f"{what}: AGE plane")
        assert fx.metadata()["alive_count"] == orc.fx.alive_count()
    return got, rid_after, age_after


# ---- every key pattern on every path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", list(ROWS))
@pytest.mark.parametrize("name", list(rk.PATTERNS))
def test_sort_of_written_keys(rig, row, name):
    cap, ns, path = ROWS[row]
    gen, dt = rk.PATTERNS[name]
    r = rig(cap)
    insts = r.instances()
    try:
        lists = _burst(r, insts, ns)
        written = []
        for i, ((fx, orc), before) in enumerate(zip(insts, lists)):
            rid, age = gen(len(before), 1000 + 17 * i)
            written.append(_write_keys(r, fx, orc, before, rid, age))
            if len(before) >= 2:   # a sort that did nothing must not pass
                assert rk.in_key_order(before, written[-1][0], written[-1][1]) == (name == "all_equal"), (row, name, i)
        p0 = r.paths()
        r.step(insts, dt, [0, 0, 0])
        assert r.ran(p0) == {path: 1}, (row, name, r.prog.kernel_info())
        for i, ((fx, orc), before) in enumerate(zip(insts, lists)):
            rp, ap, lp = written[i]
            what = f"{row} / {name} / instance {i} ({len(before)} of {cap})"
            age_now = fx.read_attr(A.AGE.id).view(np.uint32)
            rows = rk.survivors(before, age_now, lp)
            nan = name == "nan_ages"       # quiet-NaN ages: the one pattern not compared against the oracle (see the module docstring)
            got, rid_after, age_after = _check_sorted(fx, orc, rows, what, against_oracle=not nan)
            np.testing.assert_array_equal(rid_after, rp, err_msg=what)
            assert len(got) == (len(before) - len(range(4, len(before), 10)) if nan else len(before)), what
            if name == "all_equal":
                np.testing.assert_array_equal(got, before, err_msg=what)       # varying == 0: the list stands
            if dt == 0.0:
                # a tick of +0 passes every bit pattern through (denormals too); -0 becomes +0; a NaN stays a NaN (payload not compared)
                isnan = (ap & 0x7F800000 == 0x7F800000) & (ap & 0x007FFFFF != 0)
                np.testing.assert_array_equal(np.where(isnan, 0, age_after), np.where(isnan, 0, np.where(ap == 0x80000000, 0, ap)), err_msg=what)
                assert ((age_after[isnan] & 0x7F800000 == 0x7F800000) & (age_after[isnan] & 0x007FFFFF != 0)).all(), what
    finally:
        r.release(insts)


# ---- the head-order check of sort_fill_tile at its seams ----------------------------------------------------------------------------------
def _ascending_with_one_swap(n, i):
    j = np.arange(n, dtype=np.uint64)
    if i is not None:
        j[i], j[i + 1] = j[i + 1], j[i]
    return (j >> np.uint64(12)).astype(np.uint32), (np.uint64(0x3F000000) + (j & np.uint64(4095)) * np.uint64(16)).astype(np.uint32)


@pytest.mark.parametrize("cap,n,i", [(20480, 20000, i) for i in (0, 62, 63, 255, 4094, 4095, 8191, 19998)] + [(4096, 4000, i) for i in (63, 255, 3998)])
def test_one_inversion_in_the_head_is_found_at_every_seam(rig, cap, n, i):
    """No spawn, tick 0, keys strictly ascending along the list but for ONE swapped adjacent pair at rows (i, i + 1): lanes 62|63 (shuffle), 63|64 and rows
    255|256 (through LDS), rows 4095|4096 (the next tile's first row, from global memory), the list's first and last pair. With no spawn the range is empty
    unless the check finds the inversion: a missed one leaves the list unsorted. Capacity 4096 takes the one-tile variant, which keeps the verdict in LDS.
    Next to it an instance without inversion (its list must stand) and an empty one."""
    r = rig(cap)
    insts = r.instances()
    try:
        lists = _burst(r, insts, [0, n, n])
        keys = [None, _ascending_with_one_swap(n, i), _ascending_with_one_swap(n, None)]
        for (fx, orc), before, k in zip(insts[1:], lists[1:], keys[1:]):
            rp, ap, _ = _write_keys(r, fx, orc, before, *k)
        assert not rk.in_key_order(lists[1], *rk.planes(cap, lists[1], *keys[1])[:2])
        p0 = r.paths()
        r.step(insts, 0.0, [0, 0, 0])
        assert r.ran(p0) == {"one-tile" if cap <= 4096 else "multi-launch": 1}, r.prog.kernel_info()
        for idx, ((fx, orc), before) in enumerate(zip(insts, lists)):
            got, rid_after, age_after = _check_sorted(fx, orc, before, f"capacity {cap}, swap at {i}, instance {idx}")
            assert rk.in_key_order(got, rid_after, age_after)
        np.testing.assert_array_equal(insts[2][0].alive_list(), lists[2])
    finally:
        r.release(insts)


# ---- merge of a sorted head with a sorted tail: a range that starts inside a tile ---------------------------------------------------------------
def _sorted_head(h, tie_bits):
    """h keys in key order: ribbon ids 0, 1, 2, 5 in four runs, ages rising within each: a third below `tie_bits`, a third exactly it, a third above."""
    rid, age = np.zeros(h, np.uint32), np.zeros(h, np.uint32)
    bounds = [h * q // 4 for q in range(5)]
    for q, rv in enumerate((0, 1, 2, 5)):
        g = bounds[q + 1] - bounds[q]
        j = np.arange(g, dtype=np.int64)
        lo, hi = g // 3, g - g // 3
        a = np.where(j < lo, tie_bits - (lo - j), np.where(j < hi, tie_bits, tie_bits + 1 + (j - hi)))
        rid[bounds[q]:bounds[q + 1]] = rv
        age[bounds[q]:bounds[q + 1]] = a.astype(np.uint32)
    return rid, age


@pytest.mark.parametrize("h,t", [(5000, 7), (5000, 140000), (131071, 4097), (100000, 65536), (100000, 65537)])
def test_merge_of_head_and_spawns_with_an_unaligned_range(rig, h, t):
    """A head of h rows in key order (written; then one frame without spawns makes it 'the previous frame's sorted list'), then a frame that spawns t
    particles with ribbon ids 0, 1, 2 whose age ties with the middle third of every head run after the common tick: the device finds the head in order,
    the radix range is the tail [h, h + t) - not tile-aligned, in two groups of tiles for t = 140000 -, and k_sort_merge places head rows first on equal
    keys. Head keys below every tail key and above every tail key (ribbon id 5) take sorted_rank's two early-outs, the others and every tail key its
    binary search. Bit-exact against the oracle after both frames.
    The AGE write makes the list unprovable for good (RibbonHistory::values_broken), so every case here sorts by the eight radix passes whatever t is;
    test_spawn_range_at_the_one_workgroup_limit covers the proven side of kSortSmallMax."""
    cap = 266240
    r = rig(cap)
    insts = r.instances()
    hs, ts = [0, h // 2 + 1, h], [0, t // 2 + 1, t]
    tie = np.float32(0.5)
    after_first = tie + np.float32(DT)         # f32 sum, as the update computes it: the age of the tie rows when the spawns arrive
    try:
        lists = _burst(r, insts, hs)
        for (fx, orc), before in zip(insts, lists):
            _write_keys(r, fx, orc, before, *_sorted_head(len(before), int(tie.view(np.uint32))))
        p0 = r.paths()
        r.step(insts, DT, [0, 0, 0])
        assert r.ran(p0) == {"multi-launch": 1}
        for i, ((fx, orc), before) in enumerate(zip(insts, lists)):
            got, _, _ = _check_sorted(fx, orc, before, f"head {h}, instance {i}, frame without spawns")
            np.testing.assert_array_equal(got, before)            # it was in order: the list stands
        p0 = r.paths()
        r.step(insts, DT, ts, props={"a0": after_first, "k": np.array([3], np.uint32)})
        assert r.ran(p0) == {"multi-launch": 1}, r.prog.kernel_info()
        for i, ((fx, orc), before) in enumerate(zip(insts, lists)):
            got, rid_after, age_after = _check_sorted(fx, orc, None, f"head {hs[i]} + {ts[i]} spawns, instance {i}")
            assert len(got) == hs[i] + ts[i]
            key = rk.key64(rid_after[:, 0], age_after[:, 0])[got]
            assert (key[1:] >= key[:-1]).all()
            if ts[i] and hs[i]:
                spawned = np.setdiff1d(got, before)
                ties = np.isin(key, key[np.isin(got, spawned)])    # rows whose key some spawn has
                assert ties.sum() > ts[i] + hs[i] // 5              # ... include a good part of the head (a third of three of its four runs): the ties exist
                # head rows first on equal keys: within every run of equal keys, no spawn in front of a head row
                is_spawn = np.isin(got, spawned).astype(np.int8)
                same = key[1:] == key[:-1]
                assert not (same & (is_spawn[:-1] == 1) & (is_spawn[1:] == 0)).any()
    finally:
        r.release(insts)


@pytest.mark.parametrize("t,path", [(65536, "one-workgroup"), (65537, "multi-launch")])
def test_spawn_range_at_the_one_workgroup_limit(t, path):
    """Nothing written to AGE: the program stays provable (uniform non-negative initial ages and ticks), the host bounds the radix range by the largest
    spawn request, and kSortSmallMax = 65536 decides between one workgroup sorting the range and the eight radix passes. A head of 100000 (ribbon ids
    0, 1, 2, 5 written - a RIBBON_ID write makes the next sort a full one, nothing more) and t spawns whose age ties with every head row of their ribbon."""
    cap, h = 266240, 100000
    r = Rig(cap)                                   # its own program: the shared one has had its AGE plane written
    insts = r.instances()
    hs, ts = [0, 70001, h], [0, 9, t]
    try:
        lists = _burst(r, insts, hs)               # tick 0: every age is 0.5
        for (fx, orc), before in zip(insts, lists):
            rid = _sorted_head(len(before), 0)[0]
            rp = np.zeros((cap, 1), np.uint32)
            rp[before, 0] = rid
            fx.write_attr(A.RIBBON_ID.id, rp)
            orc.fx.write_attr(A.RIBBON_ID.id, rp)
        p0 = r.paths()
        r.step(insts, DT, [0, 0, 0])
        assert r.ran(p0) == {"multi-launch": 1}    # after a host write the whole list is the range
        now = np.float32(0.5) + np.float32(DT)
        p0 = r.paths()
        r.step(insts, DT, ts, props={"a0": now, "k": np.array([3], np.uint32)})
        assert r.ran(p0) == {path: 1}, r.prog.kernel_info()
        for i, ((fx, orc), before) in enumerate(zip(insts, lists)):
            got, rid_after, age_after = _check_sorted(fx, orc, None, f"proven head {hs[i]} + {ts[i]} spawns, instance {i}")
            assert len(got) == hs[i] + ts[i] and len(np.unique(age_after[got, 0])) <= 1      # every age ties: ribbon id and stability decide the order
            is_spawn = ~np.isin(got, before)
            key = rk.key64(rid_after[:, 0], age_after[:, 0])[got]
            same = key[1:] == key[:-1]
            assert (key[1:] >= key[:-1]).all() and not (same & is_spawn[:-1] & ~is_spawn[1:]).any()    # in key order, head rows first on equal keys
            np.testing.assert_array_equal(got[~is_spawn], before)                                      # ... and the head rows among themselves as they were
    finally:
        r.release(insts)
        r.ctx.close()


# ---- the sort skipped in list-free frames relies on every path being stable -----------------------------------------------------------------------
def _skipped(prog):
    line = [l for l in prog.kernel_info().split("\n") if l.startswith("ribbon sorts skipped in list-free frames")]
    return int(line[0].split(":")[1].split()[0]) if line else 0


def test_sort_skip_on_and_off_agree_while_ages_collide_under_rounding():
    """Two contexts - the default, which skips the sort of a frame whose list kernels it skipped, and one with skip_lists off, which sorts in every frame -
    and the oracle, over 40 frames. Three ribbon ids, spawns over the first 6 frames, then a host write of AGE: distinct adjacent floats just below 2048.0,
    scattered over the list. The ulp doubles at 2048: under a tick of 1/60 pairs of distinct ages round to the same float within a few frames. A sort that
    runs then sees new ties; not sorting is only the same thing because every sort path is stable. Lists and AGE planes identical across all three after
    every frame; the number of distinct keys falls, or the inputs do not do what they claim."""
    cap = 3000
    asset = rk.sort_asset(cap)
    ctxs = [bh.Context(0), bh.Context(0)]
    ctxs[1].set_option("skip_lists", 0)
    progs = [c.create_program(bh.lower(asset)) for c in ctxs]
    fxs = [p.create_effect() for p in progs]
    orc = OracleRunner(asset)
    distinct = []
    try:
        for f in range(40):
            spawn, seed = (150 if f < 6 else 0), 0xABC0 + f
            for c, fx in zip(ctxs, fxs):
                if f == 0:
                    fx.set_property("k", np.array([3], np.uint32))
                c.frame_begin(DT, f * DT)
                fx.set_frame(spawn, seed)
                c.simulate()
            if f == 0:
                orc.fx.set_property("k", np.array([3], np.uint32))
            orc.fx.step(DT, spawn, seed, time=f * DT)
            if f == 5:
                alive = orc.fx.alive_list()
                assert len(alive) == 900
                top = int(np.float32(2048.0).view(np.uint32))
                ages = np.zeros((cap, 1), np.uint32)
                ages[alive, 0] = top - 1 - np.random.default_rng(5).permutation(len(alive)).astype(np.uint32)     # 900 distinct floats, the nearest below 2048
                for t in fxs + [orc.fx]:
                    t.write_attr(A.AGE.id, ages.view(np.float32))
            ref_list, ref_age = orc.fx.alive_list(), orc.fx.read_attr(A.AGE.id).view(np.uint32)
            for which, fx in zip(("skip on", "skip off"), fxs):
                assert fx.metadata()["fault"] == 0
                np.testing.assert_array_equal(fx.alive_list(), ref_list, err_msg=f"frame {f}, {which}: alive list")
                np.testing.assert_array_equal(fx.read_attr(A.AGE.id).view(np.uint32), ref_age, err_msg=f"frame {f}, {which}: AGE plane")
            if f >= 6:
                distinct.append(len(np.unique(rk.key64(orc.fx.read_attr(A.RIBBON_ID.id)[ref_list, 0], ref_age[ref_list, 0]))))
        assert _skipped(progs[0]) > 0, progs[0].kernel_info()
        assert _skipped(progs[1]) == 0, progs[1].kernel_info()
        # The ages did collide: the 900 written ages are consecutive floats of [1024, 2048); within 900 * 2^-13 s = 7 frames all have crossed 2048, where the
        # grid is twice as coarse: an interval of 900 old ulps holds at most 451 floats there, and a common tick never separates equal ages again.
        assert len(np.unique(ref_age[ref_list, 0])) <= 451 and (ref_age[ref_list, 0].view(np.float32) >= 2048.0).all()
        assert distinct[0] > distinct[-1], distinct       # ... and with them keys (two ages that met share a key where they share the ribbon id: about a third of the pairs)
    finally:
        for c in ctxs:
            c.close()
