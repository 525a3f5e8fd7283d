"""hnb_effect_check and hnb_effect_compare (k_check_rows, k_compare_words) against planted faults of every class they exist to report: the judge
of bench.py's gate and of the export, import, steps and ribbon tests is itself held against tests/verify_model.py (the header's rules in numpy)
and against literal expectations. Every comparison is exact.

Twin contexts - default options against PLAIN - step the same frames; single wrong words are then written into the raw state of one of them
(verify_model.planted) and taken back. The rules every test here keeps:

  * A corrupted effect is never simulated, exported, imported or sorted. Between planting and restoring only check, compare and read-backs
    through hipMemcpy run on it.
  * After every restore check()["ok"] == 1 and compare with the untouched twin gives equal == 1 (assert_healthy): that also proves the restore.
  * A list head is never planted: bits 1..31 of HnbDeviceMeta::list_column are left alone.
  * An alive_count above the capacity is never planted: every planted state is one on which the kernels stay in bounds by reading them.
    Out-of-range SLOT values are fine - k_check_rows returns before it indexes with one, k_compare_words indexes with none.
  * AGE words are planted only into effects that keep their ages in the plane (HNB_OPT_AGE_COHORT 0, or the default AUTO below 65,536 slots for an
    asset whose renderer reads AGE): under a cohort the materialise in front of both calls rewrites the plane.
  * The alive bytes are not in the device view: they are derived from the lists of the healthy state, which check() has just found consistent.

Left out: a layout with AGE but without LIFETIME - neither effects.py nor reference_examples.py has one."""
import numpy as np
import pytest

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects
from helpers import A, frame_seed
from test_gpu_export import step
from test_gpu_import import trails_mixed
from test_verification import PLAIN
import verify_model as vm

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
AGE, LIFETIME, POSITION, VELOCITY = A.AGE.id, A.LIFETIME.id, A.POSITION.id, A.VELOCITY.id
QNAN = 0x7FC00000
CHECK_COUNTS = ("bad_slots", "duplicate_slots", "alive_byte_mismatches", "alive_past_lifetime")
CLEAN = dict(bad_slots=0, duplicate_slots=0, alive_byte_mismatches=0, alive_past_lifetime=0, ok=1)


def make(asset, options):
    ctx = bh.Context(0)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx, ctx.create_program(bh.lower(asset)).create_effect()


def twins(asset_of, cap, frames):
    """(ctx, fx) under default options and under PLAIN, stepped through the same frames [(spawn, dt)]"""
    pair = [make(asset_of(cap), {}), make(asset_of(cap), PLAIN)]
    for f, (spawn, dt) in enumerate(frames):
        for ctx, fx in pair:
            step(ctx, fx, f, spawn, dt)
    return pair


def churned(cap):
    """a burst, a second in which part of it dies (lifetimes are 0.8 .. 1.2 s), spawns into freed slots: the lists are permuted and partial"""
    return [(cap, 1 / 600)] + [(0, 0.25)] * 4 + [(cap // 8, 1 / 600)]


def assert_healthy(fx, twin):
    c = fx.check()
    assert c["ok"] == 1, c
    d = fx.compare(twin)
    assert d["equal"] == 1 and d["first_section"] == -1, d


def assert_permuted_and_partial(state):
    n, cap = state["alive_count"], state["capacity"]
    alive = state["alive_col"][(state["head"] + np.arange(n)) % cap]
    assert 0 < n < cap and not np.array_equal(alive, np.sort(alive)), (n, cap)


def check_against_model(ctx, fx, flags, reaps, what, **literal):
    """check() on the state as it stands, field by field against model_check over the raw columns and planes, then against the literal expectations"""
    got = fx.check()                                       # (materialises AGE where the effect keeps cohorts: the raw planes are read behind it)
    s = vm.read_state(ctx, fx, planes=[AGE, LIFETIME])
    planes = {a: p.view(F32) for a, p in s["planes"]}
    want = vm.model_check(s["alive_col"], s["head"], s["dead_col"], s["alive_count"], flags, planes.get(AGE), planes.get(LIFETIME), reaps)
    for k in CHECK_COUNTS:
        assert got[k] == want[k], (what, k, got, want)
    assert got["ok"] == int(not any(want.values())) and got["fault"] == 0, (what, got, want)
    assert got["capacity"] == s["capacity"] and got["alive_count"] == s["alive_count"], (what, got)
    for k, v in literal.items():
        assert got[k] == v, (what, k, got)
    return got


def compare_both_ways(a, b, what, model=True, **literal):
    """compare(a, b) == compare(b, a) on every field, == model_compare over the raw states, and the literal expectations"""
    (ca, fa), (cb, fb) = a, b
    d, r = fa.compare(fb), fb.compare(fa)
    assert d == r, (what, d, r)
    if model:                                              # (compare has materialised both sides: the raw planes are current)
        want = vm.model_compare(vm.read_state(ca, fa), vm.read_state(cb, fb))
        assert d == want, (what, d, want)
    for k, v in literal.items():
        assert d[k] == v, (what, k, d)
    return d


# ---- check: every class at every edge -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,phase", [(1, "alive"), (1, "dead"), (255, "churned"), (256, "churned"), (257, "churned"), (4097, "churned")])
def test_check_reports_every_class_of_fault_at_every_edge(cap, phase):
    """Rows 0, alive_count - 1, alive_count, capacity - 1, 255 and 256, where they exist, of the effect under default options (firework_trails reaps by
    lifetime there) and of its PLAIN twin (HNB_OPT_CULL_LIFETIME 0: no reaping rule)."""
    frames = {"alive": [(1, 1 / 600)], "dead": [(1, 1 / 600)] + [(0, 0.25)] * 6, "churned": churned(cap)}[phase]
    pair = twins(effects.firework_trails, cap, frames)
    for (ctx, fx), (_, twin), reaps in ((pair[0], pair[1], True), (pair[1], pair[0], False)):
        assert_healthy(fx, twin)
        assert fx.device_view().stale_attr_mask == 0
        s0 = vm.read_state(ctx, fx, planes=[AGE, LIFETIME])
        flags, n = vm.healthy_flags(s0), s0["alive_count"]
        if phase == "churned":
            assert_permuted_and_partial(s0)
        else:
            assert n == (1 if phase == "alive" else 0)
        life = vm.plane_of(s0, LIFETIME)

        def slot_of(r):
            return int(s0["alive_col"][(s0["head"] + r) % cap] if r < n else s0["dead_col"][r])

        def addr_of(r):
            return vm.alive_row_addr(fx, s0, r) if r < n else vm.dead_addr(fx, r)

        def run(words, what, **literal):
            with vm.planted(ctx, words):
                got = check_against_model(ctx, fx, flags, reaps, f"capacity {cap}, reaps {reaps}: {what}", **literal)
            assert_healthy(fx, twin)
            return got

        for r in sorted({r for r in (0, n - 1, n, cap - 1, 255, 256) if 0 <= r < cap}):
            is_alive = r < n
            other = (cap - 1 if r != cap - 1 else n) if is_alive else 0        # a row of the OTHER list, where that list has one
            has_other = (n < cap) if is_alive else (n > 0)
            for value in (cap, 0xFFFFFFFF):
                run([(addr_of(r), value)], f"row {r} names {value:#x}", bad_slots=1, duplicate_slots=0, alive_byte_mismatches=0, alive_past_lifetime=0, ok=0)
            lo, hi = (0, n) if is_alive else (n, cap)                          # this row's list
            if hi - lo >= 2:
                j = r + 1 if r + 1 < hi else r - 1
                run([(addr_of(r), slot_of(j))], f"row {r} names row {j}'s slot", bad_slots=0, duplicate_slots=1, alive_byte_mismatches=0, alive_past_lifetime=0, ok=0)
            if has_other:
                run([(addr_of(r), slot_of(other))], f"row {r} names the slot of row {other} of the other list", bad_slots=0, duplicate_slots=1, alive_byte_mismatches=1, ok=0)
                run([(addr_of(r), slot_of(other)), (addr_of(other), slot_of(r))], f"rows {r} and {other} swapped", bad_slots=0, duplicate_slots=0, alive_byte_mismatches=2, ok=0)
            # the reaping rule, on this row's slot: !(age < lifetime) counts for an alive particle of a program that reaps, and for nothing else
            slot = slot_of(r)
            age_addr, life_addr = vm.plane_addr(fx, AGE, slot), vm.plane_addr(fx, LIFETIME, slot)
            e = 1 if (reaps and is_alive) else 0
            objects = dict(CLEAN, alive_past_lifetime=e, ok=1 - e)
            assert np.isfinite(life.view(F32)[slot]) and life.view(F32)[slot] > 0
            below = int(np.nextafter(life.view(F32)[slot], F32(-np.inf)).view(U32))
            run([(age_addr, int(life[slot]))], f"slot {slot} (row {r}): AGE := LIFETIME", **objects)
            run([(age_addr, below)], f"slot {slot} (row {r}): AGE := the float below LIFETIME", **CLEAN)          # the negative control
            run([(age_addr, QNAN)], f"slot {slot} (row {r}): AGE := NaN", **objects)
            run([(life_addr, QNAN)], f"slot {slot} (row {r}): LIFETIME := NaN", **objects)
        if n >= 4 and cap - n >= 3:                        # five faults of four classes in one state
            words = [(addr_of(0), cap), (addr_of(1), slot_of(2)), (addr_of(n - 1), slot_of(n)), (addr_of(n), slot_of(n - 1)),
                     (vm.plane_addr(fx, AGE, slot_of(2)), QNAN), (addr_of(cap - 1), 0xFFFFFFFF)]
            run(words, "five faults", bad_slots=2, duplicate_slots=1, alive_byte_mismatches=2, ok=0)       # (alive_past_lifetime: from the model)
        for planted_n in (n - 1, n + 1):                   # the boundary between the lists moves by a row: the stale rows it reaches are whatever they are
            if 0 <= planted_n <= cap:
                run([(vm.meta_addr(fx, "alive_count"), planted_n)], f"alive_count {n} planted as {planted_n}", alive_count=planted_n)
    for ctx, _ in pair:
        ctx.close()


def test_a_layout_without_age_and_lifetime_has_no_reaping_rule_and_keeps_the_others():
    """single_particle stores POSITION and SIZE3 only: k_check_rows gets no AGE and no LIFETIME plane. (No shipped asset has AGE without LIFETIME.)"""
    cap = 16
    ctx, fx = make(effects.single_particle(cap), {})
    _, twin = other = make(effects.single_particle(cap), PLAIN)
    for c, f in ((ctx, fx), other):
        step(c, f, 0, 5)
    assert_healthy(fx, twin)
    s0 = vm.read_state(ctx, fx)
    assert s0["alive_count"] == 5 and {a for a, _ in s0["planes"]} == {POSITION, A.SIZE3.id}
    flags = vm.healthy_flags(s0)
    check_against_model(ctx, fx, flags, True, "healthy", **CLEAN)            # (reaps = True: the model has no planes to apply it to either)
    for words, literal in (([(vm.alive_row_addr(fx, s0, 4), cap)], dict(bad_slots=1, duplicate_slots=0, alive_byte_mismatches=0)),
                           ([(vm.alive_row_addr(fx, s0, 0), int(s0["dead_col"][cap - 1]))], dict(bad_slots=0, duplicate_slots=1, alive_byte_mismatches=1)),
                           ([(vm.dead_addr(fx, 5), int(s0["dead_col"][6]))], dict(bad_slots=0, duplicate_slots=1, alive_byte_mismatches=0))):
        with vm.planted(ctx, words):
            check_against_model(ctx, fx, flags, True, f"{literal}", alive_past_lifetime=0, ok=0, **literal)
        assert_healthy(fx, twin)
    ctx.close(); other[0].close()


# ---- a ring list --------------------------------------------------------------------------------------------------------------------------------------
def test_check_and_compare_read_a_ring_list_behind_its_head():
    cap = 4096
    asset = effects.ribbon(cap)
    pair = []
    for ring in (1, 0):
        ctx, fx = make(asset, {"ring_lists": ring})
        pair.append((ctx, fx, bh.EffectSpawner(asset.spawner), bh.Pcg32()))

    def frames(first, count):
        for f in range(first, first + count):
            for ctx, fx, sp, rng in pair:
                ctx.frame_begin(1 / 60, f / 60)
                fx.set_frame(sp.tick(1 / 60, rng), frame_seed(f))
                ctx.simulate()

    (ca, fa, _, _), (cb, fb, _, _) = pair
    done = 0
    for done in range(100, 200, 7):                        # until the head stands inside the column and the list runs across the column's end
        frames(done - (100 if done == 100 else 7), 100 if done == 100 else 7)
        sa = vm.read_state(ca, fa, planes=[AGE, LIFETIME])
        if sa["head"] != 0 and sa["head"] + sa["alive_count"] > cap:
            break
    sb = vm.read_state(cb, fb, planes=False)
    head, n = sa["head"], sa["alive_count"]
    assert head != 0 and head + n > cap and n > 64 and sb["head"] == 0 and sb["alive_count"] == n
    assert not np.array_equal(sa["alive_col"], sb["alive_col"])              # the columns and the heads differ ...
    assert_healthy(fa, fb)                                                   # ... and the lists are the same
    assert_healthy(fb, fa)
    flags = vm.healthy_flags(sa)
    rows = {0: "the first row", n - 1: "the last row", cap - 1 - head: "the row at the column's last index", cap - head: "the row at index 0"}
    assert len(rows) == 4 and all(0 <= r < n for r in rows)
    for r, name in rows.items():
        physical = (head + r) % cap
        assert name != "the row at the column's last index" or physical == cap - 1
        assert name != "the row at index 0" or physical == 0
        j = (r + 7) % n                                                      # another row's slot: in range, wrong, and now named twice
        wrong = int(sa["alive_col"][(head + j) % cap])
        with vm.planted(ca, [(vm.alive_row_addr(fa, sa, r), wrong)]):
            # (every slot the planted list names is alive and young: the reaping rule has nothing to count, whether the program reaps or not)
            check_against_model(ca, fa, flags, True, f"ring, {name}", bad_slots=0, duplicate_slots=1, alive_byte_mismatches=0, alive_past_lifetime=0, ok=0)
            compare_both_ways((ca, fa), (cb, fb), f"ring, {name}", equal=0, counter_diffs=0, alive_list_diffs=1, dead_list_diffs=0, attr_diffs=0,
                              first_section=0, first_index=r)
        assert_healthy(fa, fb)
    ca.close(); cb.close()


# ---- compare: every section, both ends ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("asset_of", [trails_mixed, effects.firework_trails], ids=["trails_mixed", "firework_trails"])
def test_compare_finds_one_wrong_word_in_every_section_at_both_ends(asset_of):
    """trails_mixed: planes of 1, 2, 3 and 4 components; firework_trails: the integer COLOR. Everything is planted into the PLAIN twin (its ages are in
    its plane); the effect under default options is the untouched side."""
    cap = 1000
    a, b = twins(asset_of, cap, churned(cap))
    (ca, fa), (cb, fb) = a, b
    assert_healthy(fa, fb)
    assert_healthy(fb, fa)
    assert fa.compare(fa)["equal"] == 1 and fb.compare(fb)["equal"] == 1
    s0 = vm.read_state(cb, fb)
    assert_permuted_and_partial(s0)
    n = s0["alive_count"]
    layout = [(attr, len(p) // cap) for attr, p in s0["planes"]]
    assert {nc for _, nc in layout} >= ({1, 2, 3, 4} if asset_of is trails_mixed else {1, 3}) and len(layout) >= 5
    dead_slot = int(s0["dead_col"][cap - 1])
    none = dict(equal=0, counter_diffs=0, alive_list_diffs=0, dead_list_diffs=0, attr_diffs=0)

    def flip(attr, word, bits=1):
        return (vm.plane_addr(fb, attr, word), int(vm.plane_of(s0, attr)[word]) ^ bits)

    def run(ctxs, words, what, **literal):
        with vm.planted(ctxs, words):
            d = compare_both_ways(a, b, f"{asset_of.__name__}: {what}", **literal)
        assert_healthy(fb, fa)
        return d

    for attr, nc in layout:                                # the first word, the last word, a word of a dead slot
        for word in (0, cap * nc - 1, dead_slot * nc + nc - 1):
            run(cb, [flip(attr, word)], f"attribute {attr}, word {word}", **dict(none, attr_diffs=1, first_section=2 + attr, first_index=word))
    # bits: the sign of a zero, the payload of a NaN
    word = dead_slot * 3 + 1
    both = (vm.plane_addr(fa, POSITION, word), vm.plane_addr(fb, POSITION, word))
    pos = dict(none, attr_diffs=1, first_section=2 + POSITION, first_index=word)
    run((ca, cb), [(both[0], 0), (both[1], 0)], "+0 on both sides", equal=1, attr_diffs=0, first_section=-1)
    run((ca, cb), [(both[0], 0), (both[1], 0x80000000)], "+0 against -0", **pos)
    run((ca, cb), [(both[0], QNAN), (both[1], QNAN | 1)], "two NaNs", **pos)
    run((ca, cb), [(both[0], 0xFFC00001), (both[1], 0xFFC00001)], "the same NaN", equal=1, attr_diffs=0, first_section=-1)
    run(cb, [flip(POSITION, word, 0x80000000)], "bit 31", **pos)
    # the lists
    for r in (n, cap - 1):
        run(cb, [(vm.dead_addr(fb, r), int(s0["dead_col"][r]) ^ 1)], f"dead row {r}", **dict(none, dead_list_diffs=1, first_section=1, first_index=r - n))
    for r in (0, n - 1):
        run(cb, [(vm.alive_row_addr(fb, s0, r), int(s0["alive_col"][(s0["head"] + r) % cap]) ^ 1)], f"alive row {r}",
            **dict(none, alive_list_diffs=1, first_section=0, first_index=r))
    # several at once
    run(cb, [flip(POSITION, 700), flip(POSITION, 5, 0x100), flip(POSITION, cap * 3 - 1)], "three words of one plane, in three blocks",
        **dict(none, attr_diffs=3, first_section=2 + POSITION, first_index=5))
    run(cb, [flip(LIFETIME, cap - 1), flip(VELOCITY, 10), (vm.alive_row_addr(fb, s0, 3), cap + 3), (vm.dead_addr(fb, cap - 2), cap + 4)],
        "both lists and two planes", **dict(none, alive_list_diffs=1, dead_list_diffs=1, attr_diffs=2, first_section=0, first_index=3))
    run(cb, [flip(LIFETIME, cap - 1), flip(VELOCITY, 10), (vm.dead_addr(fb, cap - 2), cap + 4)],
        "the dead list and two planes", **dict(none, dead_list_diffs=1, attr_diffs=2, first_section=1, first_index=cap - 2 - n))
    # the counters, through the meta row
    for i in vm.COMPARED_WORDS:
        run(cb, [(vm.meta_addr(fb, i), int(s0["meta"][i]) + 1)], f"counter word {vm.META_WORDS[i]} + 1", **dict(none, counter_diffs=1, first_section=-1))
    for planted_n in (n - 1, n + 1):                       # the rows no longer correspond: neither list is compared, whatever its rows hold
        d = run(cb, [(vm.meta_addr(fb, "alive_count"), planted_n), (vm.alive_row_addr(fb, s0, 0), cap + 1), (vm.dead_addr(fb, cap - 1), cap + 2)],
                f"alive_count {n} planted as {planted_n}", equal=0, alive_list_diffs=0, dead_list_diffs=0, attr_diffs=0, first_section=-1)
        assert d["counter_diffs"] >= 1
    ca.close(); cb.close()


# ---- the grid-stride tail -----------------------------------------------------------------------------------------------------------------------------
def test_words_past_the_launch_cap_are_compared_and_the_last_rows_checked():
    """k_compare_words runs at most 16,384 blocks of 256 threads: words from 4,194,304 on are reached only by its grid-stride loop. Capacity 1,400,077
    is the smallest whose vec3 planes (4,200,231 words) are longer; it is no multiple of 256 either, for the last partial block of k_check_rows."""
    cap = 1_400_077
    words = cap * 3
    span = 16_384 * 256
    assert words - 1 > span and cap % 256 != 0
    a, b = twins(effects.firework_trails, cap, [(cap, 1 / 600), (0, 0.45), (0, 0.45)])     # lifetimes from 0.8 s: part of the burst is gone
    (ca, fa), (cb, fb) = a, b
    assert_healthy(fa, fb)
    s0 = vm.read_state(cb, fb, planes=[POSITION])
    n = s0["alive_count"]
    assert 0 < n < cap
    pos = vm.plane_of(s0, POSITION)
    flip = lambda w: (vm.plane_addr(fb, POSITION, w), int(pos[w]) ^ 1)
    section = 2 + POSITION
    for ws, model in (([span - 1], False), ([span], False), ([words - 1], False), ([words - 1, span, span - 1], True),
                      ([words - 1, words - 1 - span], False)):                              # the last pair: two words of ONE thread, the later one planted first
        with vm.planted(cb, [flip(w) for w in ws]):
            compare_both_ways(a, b, f"POSITION words {ws}", model=model, equal=0, counter_diffs=0, alive_list_diffs=0, dead_list_diffs=0, attr_diffs=len(ws),
                              first_section=section, first_index=min(ws))
        assert_healthy(fb, fa)
    # the last row, in the last partial block of k_check_rows: swapped with row 0. The side under default options reaps by lifetime.
    sf = vm.read_state(ca, fa, planes=False)
    assert sf["alive_count"] == n and sf["head"] == 0
    first, last = int(sf["alive_col"][0]), int(sf["dead_col"][cap - 1])
    with vm.planted(ca, [(vm.alive_row_addr(fa, sf, 0), last), (vm.dead_addr(fa, cap - 1), first)]):
        check_against_model(ca, fa, vm.healthy_flags(sf), True, "rows 0 and capacity - 1 swapped", bad_slots=0, duplicate_slots=0, alive_byte_mismatches=2, ok=0)
    assert_healthy(fa, fb)
    ca.close(); cb.close()


# ---- neighbours ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_fault_in_one_instance_is_reported_for_that_instance_alone():
    """Five instances of one program in one slab table. Instances 2 and 4 get the same slot_base, spawn counts and seeds: the same state."""
    cap, n_inst = 4096, 5
    ctx = bh.Context(0)
    prog = ctx.create_program(bh.lower(effects.instancing(cap, rate=cap / 0.25)))
    bases = [1000, 2000, 3000, 4000, 3000]
    fxs = [prog.create_effect(slot_base=bases[k]) for k in range(n_inst)]
    spawns = [37, 0, 700, 301, 700]                                # instance 1 stays empty
    for f in range(6):
        ctx.frame_begin(1 / 60, f / 60)
        for k, fx in enumerate(fxs):
            fx.set_frame(spawns[k] if f < 4 else 0, frame_seed(f * n_inst + (2 if k == 4 else k)))
        ctx.simulate()
    ctx.synchronize()
    assert all(fx.check()["ok"] == 1 for fx in fxs)
    d = fxs[2].compare(fxs[4])
    assert d["equal"] == 1 and d["first_section"] == -1, d
    assert fxs[2].compare(fxs[3])["equal"] == 0                     # (other inputs: another state)
    s2 = vm.read_state(ctx, fxs[2], planes=False)
    n = s2["alive_count"]
    assert n == 4 * 700 and s2["head"] == 0
    with vm.planted(ctx, [(vm.alive_row_addr(fxs[2], s2, 5), int(s2["dead_col"][cap - 1]))]):      # an alive row names a dead slot
        for k in (0, 1, 3, 4):
            c = fxs[k].check()
            assert c["ok"] == 1, (k, c)
        c = fxs[2].check()
        assert c["ok"] == 0 and c["bad_slots"] == 0 and c["duplicate_slots"] == 1 and c["alive_byte_mismatches"] == 1, c
        for x, y in ((2, 4), (4, 2)):
            d = fxs[x].compare(fxs[y])
            assert (d["equal"], d["counter_diffs"], d["alive_list_diffs"], d["dead_list_diffs"], d["attr_diffs"], d["first_section"], d["first_index"]) == (0, 0, 1, 0, 0, 0, 5), d
    with vm.planted(ctx, [(vm.dead_addr(fxs[2], cap - 1), cap)]):                                 # ... and a dead row names no slot
        assert [fxs[k].check()["ok"] for k in range(n_inst)] == [1, 1, 0, 1, 1]
        assert fxs[2].check()["bad_slots"] == 1
    word = 3 * int(s2["alive_col"][n - 1]) + 2
    old = int(vm.read_words(vm.plane_addr(fxs[4], POSITION, word), 1)[0])
    with vm.planted(ctx, [(vm.plane_addr(fxs[4], POSITION, word), old ^ 0x00400000)]):
        d = fxs[2].compare(fxs[4])
        assert d["equal"] == 0 and d["attr_diffs"] == 1 and d["first_section"] == 2 + POSITION and d["first_index"] == word, d
        assert all(fx.check()["ok"] == 1 for fx in fxs)             # (a position is no invariant)
    assert all(fx.check()["ok"] == 1 for fx in fxs) and fxs[2].compare(fxs[4])["equal"] == 1
    ctx.close()
