"""Builders for the adversarial spawn-event tests (tests/test_event_scripts.py: oracle only; tests/test_gpu_event_edges.py: the kernels).

k_emit_count / k_emit_events order a frame's spawn events: a cross-chunk prefix over the 4096-row chunks of the parent, a workgroup scan over a
chunk's rows, rows below kEmitHeavy = 32 events written by their own thread, heavier rows queued in LDS and dealt over gridDim.y splits by
`row % n_split`, every writer cut at the buffer's capacity. No ABI call reads an event buffer, so the tests make it observable: a parent whose
per-row event counts are DICTATED (the update emits attr(U32_0) events on channel 0 and, on death, attr(U32_1) on channel 1; the test writes both
planes), and fresh, empty children of at least the buffer's capacity that store the emitting particle's U32_2 (= its ID) in U32_3. One frame after
the emitting frame a child's alive list is 0 .. n-1 and its U32_3 plane IS the stored prefix of the buffer, row for row.

Everything here is a function of (rows, pattern): the capacities come from the pattern's running sum, never from a table."""
import numpy as np

import bevy_hanabi_amd as bh
from helpers import A, Frame, assert_same_linked_state, frame_seed

CHUNK = 4096          # rows per workgroup of k_emit_* (kChunk)
HEAVY = 32            # kEmitHeavy: events of one row from which the whole workgroup writes them
PARENT_CAPS = (CHUNK, CHUNK + 1, 3 * CHUNK + 5)
CHILD_CLASSES = (8192, 32768, 140000, 524288)   # capacities of the child programs: a probe takes the smallest that holds its event buffer
MAX_EVENT_CAPACITY = CHILD_CLASSES[-1]  # (a buffer for the 1 << 30 pattern's total would be 4 GiB: capacities above this are not probed)
DT = 1 / 60


# ---- plan::size_event_grid (hnb_plan.h) restated ---------------------------------------------------------------------------------------------
def size_event_grid(max_event_capacity, total_chunks):
    per_chunk = max_event_capacity // max(total_chunks, 1)
    return min(max((per_chunk + 16383) // 16384, 1), 64)


def chunks_of(capacity):
    return (capacity + CHUNK - 1) // CHUNK


# ---- assets --------------------------------------------------------------------------------------------------------------------------------
def dictated_parent(capacity):
    """Emits attr(U32_0) events per alive row on channel 0 and attr(U32_1) per dying row on channel 1. The init leaves both 0 (a new particle
    emits nothing until the test writes the planes), U32_2 = ID, POSITION a function of the ID, AGE 0, LIFETIME 1000 (the test writes LIFETIME
    to schedule deaths)."""
    w = bh.ExprWriter()
    F = bh.ValueType(bh.ScalarType.Float)
    pos = w.attr(A.ID).cast(F).vec3(w.lit(1.0), w.lit(2.0))
    init = [bh.SetAttributeModifier(A.POSITION, pos.expr()), bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr()),
            bh.SetAttributeModifier(A.LIFETIME, w.lit(1000.0).expr()), bh.SetAttributeModifier(A.U32_2, w.attr(A.ID).expr())]
    upd = [bh.EmitSpawnEventModifier(bh.EventEmitCondition.Always, w.attr(A.U32_0).expr(), 0),
           bh.EmitSpawnEventModifier(bh.EventEmitCondition.OnDie, w.attr(A.U32_1).expr(), 1)]
    a = bh.EffectAsset(capacity, bh.SpawnerSettings.once(float(capacity)), w.finish())
    for m in init:
        a.init(m)
    for m in upd:
        a.update(m)
    return a


def recording_child(capacity, lifetime=None):
    """POSITION inherited, U32_3 = the emitting particle's U32_2. lifetime None: no AGE / LIFETIME at all, the particles stay (a fresh child
    per probe); a lifetime below the tick: every particle dies in the update of the frame it was spawned in, the planes keep what it read."""
    w = bh.ExprWriter()
    init = [bh.InheritAttributeModifier(A.POSITION), bh.SetAttributeModifier(A.U32_3, w.parent_attr(A.U32_2).expr())]
    if lifetime is not None:
        init += [bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr()), bh.SetAttributeModifier(A.LIFETIME, w.lit(lifetime).expr())]
    a = bh.EffectAsset(capacity, bh.SpawnerSettings(), w.finish())
    for m in init:
        a.init(m)
    return a


def reuse_parent(capacity=CHUNK, lifetime=0.04):
    """Part 6: random POSITION and F32_0 (so that a slot's next occupant differs from the last), a uniform lifetime of three ticks, 2 events
    per dying particle."""
    w = bh.ExprWriter()
    init = [bh.SetPositionSphereModifier(w.lit((0.0, 0.0, 0.0)).expr(), w.lit(2.0).expr(), bh.ShapeDimension.Volume),
            bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr()), bh.SetAttributeModifier(A.LIFETIME, w.lit(lifetime).expr()),
            bh.SetAttributeModifier(A.F32_0, w.rand(bh.ValueType(bh.ScalarType.Float)).expr())]
    emit = bh.EmitSpawnEventModifier(bh.EventEmitCondition.OnDie, w.lit(bh.Value.u32(2)).expr(), 0)
    a = bh.EffectAsset(capacity, bh.SpawnerSettings.once(float(capacity)), w.finish())
    for m in init:
        a.init(m)
    return a.update(emit)


def reuse_child(capacity=8 * CHUNK):
    w = bh.ExprWriter()
    init = [bh.InheritAttributeModifier(A.POSITION), bh.SetAttributeModifier(A.F32_1, w.parent_attr(A.F32_0).expr()),
            bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr()), bh.SetAttributeModifier(A.LIFETIME, w.lit(100.0).expr())]
    a = bh.EffectAsset(capacity, bh.SpawnerSettings(), w.finish())
    for m in init:
        a.init(m)
    return a


_ASSETS = {}


def asset(kind, *args):
    """one asset object per (kind, arguments): a cache key for the programs of a context"""
    key = (kind,) + args
    if key not in _ASSETS:
        _ASSETS[key] = {"parent": dictated_parent, "child": recording_child, "reuse_parent": reuse_parent, "reuse_child": reuse_child}[kind](*args)
    return key, _ASSETS[key]


SPLIT64_CAPACITY = 1 << 20
TABLE_CHILD_CAPACITY = 70_000
TABLE_CHILD_LIFETIME = 0.01      # below the tick


def warm_assets():
    """the fixed programs of the GPU tests (tools/warm_jit_cache.py compiles their kernels ahead of the tests)"""
    out = [asset("parent", c)[1] for c in PARENT_CAPS] + [asset("child", c, None)[1] for c in CHILD_CLASSES + (SPLIT64_CAPACITY,)]
    return out + [asset("child", TABLE_CHILD_CAPACITY, TABLE_CHILD_LIFETIME)[1], asset("reuse_parent")[1], asset("reuse_child")[1]]


# ---- count patterns ------------------------------------------------------------------------------------------------------------------------
class Pattern:
    """c0 / c1: the U32_0 / U32_1 value of every list row; die: the rows that die in the emitting frame (None: none). What is EMITTED: channel 0
    by the rows that stay alive, channel 1 by the rows that die."""

    def __init__(self, c0, c1=None, die=None):
        n = len(c0)
        self.c0 = np.asarray(c0, dtype=np.uint32)
        self.c1 = np.zeros(n, dtype=np.uint32) if c1 is None else np.asarray(c1, dtype=np.uint32)
        self.die = np.zeros(n, dtype=bool) if die is None else np.asarray(die, dtype=bool)

    def emitted(self, channel):
        return np.where(self.die, 0, self.c0).astype(np.uint32) if channel == 0 else np.where(self.die, self.c1, 0).astype(np.uint32)


def _rows(n):
    return np.arange(n, dtype=np.uint32)


def _one_heavy(n, row, rest, count=1000):
    c = np.full(n, rest, dtype=np.uint32)
    c[row] = count
    return c


def count_patterns(n):
    """{name: Pattern} for a parent of n rows (issue part 2)."""
    r = _rows(n)
    p = {"all31": Pattern(np.full(n, 31)), "all32": Pattern(np.full(n, 32)),    # (all32: every row heavy, the LDS queue holds 4096 entries per chunk)
         "alt31_32": Pattern(31 + (r & 1)), "every17th_33": Pattern(np.where(r % 17 == 0, 33, 1))}
    last = n - 1
    for row in sorted({0, CHUNK - 1, CHUNK, last}):
        if row < n:
            for rest in (0, 1):
                p[f"heavy1000_row{row}_rest{rest}"] = Pattern(_one_heavy(n, row, rest))
    p["one_2pow30"] = Pattern(_one_heavy(n, n // 2 + 3, 0, 1 << 30) + (r % 3) * (r != n // 2 + 3))
    only_last = np.zeros(n, dtype=np.uint32)
    only_last[last] = 3
    p["only_last_row"] = Pattern(only_last)
    p["zero"] = Pattern(np.zeros(n))
    # OnDie: every 7th row (from 3) dies and emits its U32_1 - 40 on every 5th row, else 2 - on channel 1; the survivors feed channel 0
    p["ondie"] = Pattern(1 + (r & 1), np.where(r % 5 == 0, 40, 2), r % 7 == 3)
    return p


def split_patterns(n):
    """issue part 3: with 3 (5) splits `row % n_split` does not line up with a thread's 16 consecutive rows; rows = 1 (mod 3): one split owns
    every heavy row, another owns none"""
    r = _rows(n)
    return {"every3rd_heavy": Pattern(np.where(r % 3 == 0, 32, 1)), "every5th_heavy": Pattern(np.where(r % 5 == 0, 32, 1)),
            "mod3_eq1_heavy": Pattern(np.where(r % 3 == 1, 32, 1))}


# (parent capacity, capacity of channel 0's buffer, splits expected, pattern)
SPLIT_CASES = [(CHUNK, 16384, 1, "every3rd_heavy"), (CHUNK + 1, 65536, 2, "every3rd_heavy"),
               (CHUNK, 49152, 3, "every3rd_heavy"), (CHUNK, 49152, 3, "mod3_eq1_heavy"), (CHUNK, 49152, 3, "every5th_heavy"),
               (CHUNK, 81920, 5, "every5th_heavy"), (CHUNK, 81920, 5, "mod3_eq1_heavy"), (CHUNK, 81920, 5, "every3rd_heavy")]


def split64_pattern(n=CHUNK):
    """4096 rows of 257 events: 1,052,672 requested, 1,048,576 stored, every row heavy, dealt over 64 splits"""
    return Pattern(np.full(n, 257))


# ---- capacities from a pattern's running sum -------------------------------------------------------------------------------------------------
def prefix(counts):
    return np.concatenate([[0], np.cumsum(counts.astype(np.int64))])


def named_capacities(counts):
    """{name: capacity} for the counts a channel emits per list row (issue part 2). Names whose state the pattern cannot reach (no heavy row, a
    total of 0, a capacity above MAX_EVENT_CAPACITY) are left out; test_event_scripts.py asserts every state that is named."""
    P = prefix(counts)
    total, n = int(P[-1]), len(counts)
    first_chunk = int(P[min(CHUNK, n)])
    out = {"one": 1}
    pos = np.nonzero(counts > 0)[0]
    if len(pos):
        out["row_first_event"] = int(P[pos[len(pos) // 2]]) + 1            # the last stored event is the first of a row in the middle
    light = np.nonzero((counts >= 2) & (counts < HEAVY))[0]
    if len(light):
        out["into_light_row"] = int(P[light[len(light) // 2]]) + 1
    heavy = np.nonzero(counts >= HEAVY)[0]
    if len(heavy):
        out["into_heavy_row"] = int(P[heavy[len(heavy) // 2]]) + 1
    if first_chunk:
        out.update({"first_chunk_total": first_chunk, "first_chunk_minus1": first_chunk - 1, "first_chunk_plus1": first_chunk + 1})
        if n > CHUNK:
            out["below_first_chunk"] = (first_chunk + 1) // 2     # every later chunk starts at or above the capacity
    if total:
        out.update({"total": total, "total_plus1": total + 1})
    return {k: v for k, v in out.items() if 0 < v <= MAX_EVENT_CAPACITY}


def stored_rows(counts, capacity):
    """the list row behind every stored event: event e belongs to the row whose running sum passes e (no 2^30-element array)"""
    P = prefix(counts)
    n = int(min(P[-1], capacity))
    return np.searchsorted(P[1:], np.arange(n, dtype=np.int64), side="right").astype(np.int64)


def describe_cut(counts, capacity):
    """where the capacity cuts the pattern: facts test_event_scripts.py asserts per named capacity"""
    P = prefix(counts)
    total, n = int(P[-1]), len(counts)
    d = {"total": total, "stored": min(total, capacity), "dropped": max(total - capacity, 0)}
    if d["stored"]:
        row = int(np.searchsorted(P[1:], d["stored"] - 1, side="right"))
        d.update({"last_row": row, "last_offset": d["stored"] - 1 - int(P[row]), "last_count": int(counts[row])})
    # chunks whose exclusive prefix already lies at or above the capacity and that still have events (the `excl >= capacity` exit)
    d["chunks_past_capacity"] = sum(1 for j in range(1, chunks_of(n)) if int(P[j * CHUNK]) >= capacity and int(P[min((j + 1) * CHUNK, n)]) > int(P[j * CHUNK]))
    return d


def probe_plan(pattern):
    """[(name, capacity of channel 0, capacity of channel 1 or None)]: the named capacities of the channel the pattern is about - channel 1 for a
    pattern with dying rows (channel 0 then listens with half of what the survivors emit), else channel 0 with nobody on channel 1"""
    if pattern.die.any():
        half = max(int(prefix(pattern.emitted(0))[-1]) // 2, 1)
        return [(name, half, cap) for name, cap in named_capacities(pattern.emitted(1)).items()]
    return [(name, cap, None) for name, cap in named_capacities(pattern.emitted(0)).items()]


def child_class(capacity):
    return next(c for c in CHILD_CLASSES if c >= capacity)


# ---- the probe script ----------------------------------------------------------------------------------------------------------------------
def probe_frames(names, f, spawn):
    return {n: Frame(DT, spawn.get(n, 0), frame_seed(1000 * i + f), time=f * DT) for i, n in enumerate(names)}


class Probes:
    """One dictated parent 'P' on every system of `systems` (the oracle first), its list made a non-identity permutation; probe() then runs an
    emitting frame and the frame in which fresh children record the buffers, comparing every system with the oracle after both."""

    def __init__(self, systems, parent_cap):
        self.systems, self.oracle, self.cap, self.f, self.n_probe = systems, systems[0], parent_cap, 0, 0
        key, a = asset("parent", parent_cap)
        for s in systems:
            s.add("P", a) if s is self.oracle else s.add("P", a, key)
        self.frame({"P": parent_cap})
        # partly kill and refill: the survivors move up, the new particles follow them - events go by list row, not by slot
        slots = np.arange(parent_cap, dtype=np.uint32)
        life = np.where((slots * np.uint32(2654435761) >> np.uint32(28)) % 3 == 0, np.float32(0.001), np.float32(1000.0)).astype(np.float32)
        self.write("P", A.LIFETIME, life.reshape(-1, 1))
        self.frame({})
        self.frame({"P": parent_cap})
        self.check("setup")

    def names(self):
        return list(self.oracle.fx)

    def write(self, name, attr, array):
        for s in self.systems:
            s.write_attr(name, attr, array)

    def frame(self, spawn, frozen=()):
        frames = probe_frames(self.names(), self.f, spawn)
        for s in self.systems:
            s.step(frames, frozen)
        self.f += 1

    def check(self, what):
        ref = self.oracle.state()
        for s in self.systems[1:]:
            assert_same_linked_state(ref, s.state(), f"{what} (frame {self.f - 1}, {s.name})")
        return ref

    def by_slot(self, per_row, dtype=np.uint32, fill=0):
        alive = self.oracle.fx["P"].alive_list()
        assert len(alive) == len(per_row) == self.cap, (len(alive), len(per_row))   # the parent is full before every probe
        plane = np.full((self.cap, 1), fill, dtype=dtype)
        plane[alive, 0] = per_row
        return plane, alive

    def probe(self, pattern, cap0, cap1=None, child_caps=None, on_emitted=None, what=""):
        """cap0 / cap1: event capacity of the child on channel 0 / 1 (None: nobody listens). on_emitted(oracle parent, alive list): called after
        the emitting frame (the oracle-only assertions). Returns the oracle's state after the recording frame."""
        k = self.n_probe
        self.n_probe += 1
        p0, alive = self.by_slot(pattern.c0)
        p1, _ = self.by_slot(pattern.c1)
        self.write("P", A.U32_0, p0)
        self.write("P", A.U32_1, p1)
        if pattern.die.any():
            # a dying row: alive before the tick (AGE < LIFETIME), not after it (OnDie fires on exactly that edge)
            age = self.oracle.fx["P"].read_attr(A.AGE.id)[alive, 0]
            life, _ = self.by_slot(np.where(pattern.die, age + np.float32(0.005), np.float32(1000.0)).astype(np.float32), np.float32)
            self.write("P", A.LIFETIME, life)
        children = []
        for ch, cap in ((0, cap0), (1, cap1)):
            if cap is None:
                continue
            name = f"c{ch}_{k}"
            size = (child_caps or {}).get(ch) or child_class(cap)
            assert size >= cap
            key, a = asset("child", size, None)
            for s in self.systems:
                s.add(name, a) if s is self.oracle else s.add(name, a, key)
                s.link(name, "P", ch, cap)
            children.append(name)
        self.frame({})                     # the emitting frame: the children's buffers are empty, they spawn nothing
        self.check(f"{what}: emitting frame")
        if on_emitted:
            on_emitted(self.oracle.fx["P"], alive)
        self.frame({"P": self.cap})        # the children record the buffers; the parent refills what died
        ref = self.check(f"{what}: recording frame")
        for name in children:
            for s in self.systems:
                s.remove(name)
        return {n[:2]: ref[n] for n in children}, ref["P"], alive

    def close(self):
        for s in self.systems:
            for n in list(s.fx):
                if n != "P":
                    s.remove(n)
            s.remove("P")


def expected_recording(pattern, channel, capacity, alive, slot_base=0):
    """what the child on `channel` must hold one frame after the pattern was emitted: (n, U32_3[0 .. n))"""
    rows = stored_rows(pattern.emitted(channel), capacity)
    return len(rows), (alive[rows] + slot_base).astype(np.uint32)


# ---- instance tables (issue part 4) --------------------------------------------------------------------------------------------------------
TABLE_PARENT_CAP = CHUNK + 1
# child: (parent, channel, event capacity); P2 has no listener on channel 1
TABLE_LINKS = {"C0": ("P0", 0, 16), "C1": ("P0", 1, 300), "C2": ("P1", 0, 5000), "C3": ("P2", 0, 70_000), "C4": ("P1", 1, 300)}


def table_counts(inst, cap=TABLE_PARENT_CAP):
    """(U32_0, U32_1) by slot, different for every parent instance: light only and overflowing 16 events; one heavy row in 64 and a cut inside
    5000; heavy and light alternating with more than 70,000 events; instance 3 (created late): a few heavy rows"""
    s = np.arange(cap, dtype=np.uint32)
    c0 = [s % 4, 1 + (s % 64 == 0) * 40, np.where(s & 1, 33, 3), np.where(s % 100 == 7, 50, 0)][inst % 4]
    c1 = [np.where(s % 11 == 0, 35, 1), np.where(s % 5 == 0, 3, 0), np.full(cap, 2), np.full(cap, 1)][inst % 4]
    return c0.astype(np.uint32).reshape(-1, 1), c1.astype(np.uint32).reshape(-1, 1)


def table_lifetimes(age, inst, tag):
    """a third of the slots dies within the next six frames, spread over them"""
    s = np.arange(len(age), dtype=np.uint32)
    soon = (s + inst + tag) % 3 == 0
    return np.where(soon, age + ((1 + (s // 3 + inst) % 6) / 60.0 - 0.004), 1000.0).astype(np.float32).reshape(-1, 1)


def run_instance_tables(systems, steps_per_call=1):
    """The script of issue part 4 on every system (the oracle first), compared after every frame - with steps_per_call 2 after every call: frames
    between which the host does nothing go through one step_many() of up to two frames.
    Returns the number of frames compared and facts the oracle-only test asserts."""
    orc = systems[0]
    pk, pa = asset("parent", TABLE_PARENT_CAP)
    ck, ca = asset("child", TABLE_CHILD_CAPACITY, TABLE_CHILD_LIFETIME)
    facts = {"frames": 0, "calls_of_two": 0, "counter": {}, "events": {}}

    def add(name, key, a):
        for s in systems:
            s.add(name, a) if s is orc else s.add(name, a, key)

    def link(child, parent, ch, cap):
        for s in systems:
            s.link(child, parent, ch, cap)

    def remove(name):
        for s in systems:
            s.remove(name)

    def write_parent(name, inst, tag):
        c0, c1 = table_counts(inst)
        life = table_lifetimes(orc.fx[name].read_attr(A.AGE.id)[:, 0], inst, tag)
        for s in systems:
            s.write_attr(name, A.U32_0, c0)
            s.write_attr(name, A.U32_1, c1)
            s.write_attr(name, A.LIFETIME, life)

    for i in range(3):
        add(f"P{i}", pk, pa)
    for c in TABLE_LINKS:
        add(c, ck, ca)
    for c, (p, ch, cap) in TABLE_LINKS.items():
        link(c, p, ch, cap)
    inst_of = {"P0": 0, "P1": 1, "P2": 2, "P3": 3}

    # the timeline: (host work before the frame, frozen effects of the frame)
    W = lambda tag: ("write", tag)
    plan = {1: [W(1)], 3: [W(3)], 6: [W(6)], 10: [W(10)], 15: [W(15)], 17: ["reparent_and_destroy", W(17)], 20: [W(20)], 23: ["create_fourth"], 24: [W(24)], 27: [W(27)]}
    frozen_at = {3: ("P1",), 4: ("P1",), 5: ("P1",), 7: ("C3",), 8: ("C3",), 9: ("C3",), 12: ("P0", "P1", "P2"), 13: ("P0", "P1", "P2"), 14: ("P0", "P1", "P2")}
    n_frames = 30

    seed_of = {n: 977 * (i + 1) for i, n in enumerate(list(inst_of) + ["C0", "C1", "C2", "C3", "C4", "C5"])}

    def frames_of(f):   # every parent asks for a full refill every frame: what died is replaced by particles that emit nothing until the next write
        return {n: Frame(DT, TABLE_PARENT_CAP if n in inst_of else 0, frame_seed(seed_of[n] + f), time=f * DT) for n in orc.fx}

    def check(f):
        ref = orc.state()
        for s in systems[1:]:
            assert_same_linked_state(ref, s.state(), f"instance tables frame {f}, {s.name}")
        facts["frames"] += 1
        facts["counter"][f] = {n: st["counters"]["particle_counter"] for n, st in ref.items()}
        facts["events"][f] = {n: [orc.fx[n].events(ch)[0] for ch in (0, 1)] for n in orc.fx if n in inst_of}
        return ref

    f = 0
    while f < n_frames:
        for op in plan.get(f, []):
            if op == "reparent_and_destroy":     # P0 goes: one of its children moves to P2 (channel 1, free until now), the other goes too
                link("C1", "P2", 1, 300)
                remove("C0")
                remove("P0")                     # (the last instance of the program, P2, takes index 0)
            elif op == "create_fourth":
                add("P3", pk, pa)                # reuses the freed slab
                add("C5", ck, ca)
                link("C5", "P3", 0, 300)
            else:
                for name in [n for n in orc.fx if n in inst_of]:
                    write_parent(name, inst_of[name], op[1])
        frozen = frozen_at.get(f, ())
        group = [f]
        while len(group) < steps_per_call and group[-1] + 1 < n_frames and group[-1] + 1 not in plan and frozen_at.get(group[-1] + 1, ()) == frozen:
            group.append(group[-1] + 1)
        if len(group) == 1:
            for s in systems:
                s.step(frames_of(f), frozen)
        else:
            fl = [frames_of(g) for g in group]
            for s in systems:
                s.step_many(fl, frozen)
            facts["calls_of_two"] += 1
        f = group[-1] + 1
        check(f - 1)
    return facts


TABLE_ALL_PARENTS_FROZEN = (12, 13, 14)


# ---- slot reuse before the child reads (issue part 6) ----------------------------------------------------------------------------------------
def run_slot_reuse(systems):
    """A full parent of 4096 slots whose particles all die in their third update and emit 2 events each; the host re-bursts the free slots in the
    very next frame. Init passes run parents first, so the child reads the NEW occupant of every slot. Returns (parent F32_0 before the deaths,
    oracle state after the frame in which the child spawned)."""
    orc = systems[0]
    pk, pa = asset("reuse_parent")
    ck, ca = asset("reuse_child")
    for s in systems:
        s.add("P", pa) if s is orc else s.add("P", pa, pk)
        s.add("C", ca) if s is orc else s.add("C", ca, ck)
        s.link("C", "P", 0, 2 * CHUNK)
    old, ref = None, None
    for f in range(5):
        frames = {"P": Frame(DT, CHUNK if f in (0, 3) else 0, frame_seed(f), time=f * DT), "C": Frame(DT, 0, frame_seed(500 + f), time=f * DT)}
        if f == 2:
            old = orc.fx["P"].read_attr(A.F32_0.id).copy()
        for s in systems:
            s.step(frames)
        ref = orc.state()
        for s in systems[1:]:
            assert_same_linked_state(ref, s.state(), f"slot reuse frame {f}")
        if f == 3:
            at_spawn = ref
    return old, at_spawn


# ---- a sibling of test_fuzz._random_system: counts around kEmitHeavy (issue part 7) ----------------------------------------------------------
FUZZ_COUNTS = (0, 1, 31, 32, 33, 200)
FUZZ_SEEDS = tuple(range(700, 710))


def fuzz_system(seed):
    """A parent with 1-2 event channels whose counts come from FUZZ_COUNTS - a literal, or a U32 plane the script rewrites - and a child per
    channel with a short lifetime. Returns (parent asset, planes [attribute or None per channel], [(child asset, event capacity)])."""
    rng = np.random.default_rng(seed)
    cap = int(rng.choice([37, 300, CHUNK, 4200, 9000]))
    n_ch = int(rng.integers(1, 3))
    w = bh.ExprWriter()
    init = [bh.SetPositionSphereModifier(w.lit((0.0, 0.0, 0.0)).expr(), w.lit(1.0).expr(), bh.ShapeDimension.Volume),
            bh.SetAttributeModifier(A.AGE, w.lit(0.0).expr()), bh.SetAttributeModifier(A.LIFETIME, w.lit(0.05).uniform(w.lit(float(rng.uniform(0.1, 0.4)))).expr()),
            bh.SetAttributeModifier(A.U32_2, w.attr(A.ID).expr())]
    planes, upd = [], []
    for ch in range(n_ch):
        cond = bh.EventEmitCondition.OnDie if rng.random() < 0.5 else bh.EventEmitCondition.Always
        if rng.random() < 0.3:
            planes.append(None)
            count = w.lit(bh.Value.u32(int(rng.choice(FUZZ_COUNTS[:5]))))
        else:
            planes.append((A.U32_0, A.U32_1)[ch])
            count = w.attr(planes[-1])
        upd.append(bh.EmitSpawnEventModifier(cond, count.expr(), ch))
    parent = bh.EffectAsset(cap, bh.SpawnerSettings.once(float(cap)), w.finish())
    for m in init:
        parent.init(m)
    for m in upd:
        parent.update(m)
    children = []
    for ch in range(n_ch):
        ev_cap = int(rng.choice([16, 256, 5000, 1 << 16]))
        children.append((recording_child(int(rng.choice([300, 5000, 1 << 16])), float(rng.choice([0.01, 0.03, 0.2]))), ev_cap))
    return parent, planes, children


def run_fuzz(seed, systems, n_frames=24):
    parent, planes, children = fuzz_system(seed)
    orc = systems[0]
    for s in systems:
        s.add("P", parent)
        for ch, (a, ev_cap) in enumerate(children):
            s.add(f"C{ch}", a)
            s.link(f"C{ch}", "P", ch, ev_cap)
    rng = np.random.default_rng(seed + 5)     # (its own generator: the script, not the assets)
    cap = parent.capacity
    heavy_seen = 0
    for f in range(n_frames):
        if f % 4 == 1:
            for attr in planes:
                if attr is not None:
                    # mostly light, a few heavy rows; every 8th frame a heavy frame
                    pr = [0.3, 0.3, 0.1, 0.1, 0.1, 0.1] if f % 8 == 1 else [0.5, 0.38, 0.03, 0.03, 0.03, 0.03]
                    plane = rng.choice(FUZZ_COUNTS, size=(cap, 1), p=pr).astype(np.uint32)
                    heavy_seen += int((plane >= HEAVY).sum())
                    for s in systems:
                        s.write_attr("P", attr, plane)
        dt = DT if rng.random() < 0.8 else 2 * DT
        spawn = cap if f == 0 else (int(rng.integers(0, cap // 2 + 2)) if rng.random() < 0.5 else 0)
        frames = {n: Frame(dt, spawn if n == "P" else 0, frame_seed(seed * 101 + f * 7 + i), time=f * DT) for i, n in enumerate(orc.fx)}
        for s in systems:
            s.step(frames)
        if f % 4 == 3 or f == n_frames - 1:
            ref = orc.state()
            for s in systems[1:]:
                assert_same_linked_state(ref, s.state(), f"fuzz seed {seed} frame {f}")
    return heavy_seen, orc.state()
