"""The scripts of tests/test_gpu_event_edges.py on the ORACLE alone (no device): every (pattern, capacity) pair reaches the state it is named
for, the whole stored prefix of an event buffer is observable through the child, the parent's list is not the identity, and the frozen-link
rule the drivers implement is hand-evaluated. So no GPU case can become trivially true without this file noticing."""
import os
import re

import numpy as np
import pytest

import event_scripts as es
from event_scripts import CHUNK, HEAVY
from helpers import A, ROOT, Frame, LinkedOracle, assert_same_linked_state
from test_events import tiny_child, tiny_parent


def test_size_event_grid_is_the_rule_of_hnb_plan_h():
    src = open(os.path.join(ROOT, "bevy_hanabi_amd", "csrc", "hnb_plan.h")).read()
    body = src[src.index("inline uint32_t size_event_grid("):]
    body = body[:body.index("\n}") + 2]
    assert re.search(r"per_chunk = max_event_capacity / \(total_chunks \? total_chunks : 1u\)", body)
    assert "(per_chunk + 16383u) / 16384u" in body and "splits > 64u ? 64u : splits" in body and "splits < 1u ? 1u" in body
    kern = open(os.path.join(ROOT, "bevy_hanabi_amd", "csrc", "hnb_kernels.hip.h")).read()
    assert f"constexpr uint32_t kEmitHeavy = {HEAVY}u;" in kern
    assert {s for _, _, s, _ in es.SPLIT_CASES} == {1, 2, 3, 5}
    for cap, ev_cap, splits, name in es.SPLIT_CASES:
        assert es.size_event_grid(ev_cap, es.chunks_of(cap)) == splits, (cap, ev_cap)
        pat = es.split_patterns(cap)[name]
        heavy_rows = np.nonzero(pat.c0 >= HEAVY)[0]
        owners = set((heavy_rows % splits).tolist())
        if name == "mod3_eq1_heavy" and splits == 3:
            assert owners == {1}                                      # one split owns every heavy row, the others own none
        if (name, splits) in (("every3rd_heavy", 3), ("every5th_heavy", 5)):
            assert owners == {0}
        if (name, splits) in (("every5th_heavy", 3), ("mod3_eq1_heavy", 5), ("every3rd_heavy", 5)):
            assert owners == set(range(splits))                       # ... and here every split owns some
        assert splits == 1 or int(es.prefix(pat.c0)[-1]) <= ev_cap    # nothing dropped: every split's rows are observable
    assert es.size_event_grid(es.SPLIT64_CAPACITY, 1) == 64 and es.size_event_grid(1 << 30, 1) == 64
    p64 = es.split64_pattern()
    assert (p64.c0 >= HEAVY).all() and es.SPLIT64_CAPACITY < int(es.prefix(p64.c0)[-1]) < 1 << 31
    d = es.describe_cut(p64.c0, es.SPLIT64_CAPACITY)
    assert d["last_count"] == 257 and 0 < d["last_offset"] < 256      # the cut lies inside a heavy row


def _assert_named_state(name, counts, cap):
    """the state a capacity is named for, from the numpy prefix sum of the written counts"""
    d = es.describe_cut(counts, cap)
    P = es.prefix(counts)
    n = len(counts)
    first_chunk = int(P[min(CHUNK, n)])
    if name == "one":
        assert cap == 1
    elif name == "row_first_event":
        assert d["last_offset"] == 0 and d["stored"] == cap
    elif name == "into_light_row":
        assert d["last_offset"] == 0 and 2 <= d["last_count"] < HEAVY and d["dropped"] > 0
    elif name == "into_heavy_row":
        assert d["last_offset"] == 0 and d["last_count"] >= HEAVY and d["dropped"] >= d["last_count"] - 1
    elif name == "first_chunk_total":
        assert cap == first_chunk and (n <= CHUNK or d["last_row"] < CHUNK)
    elif name == "first_chunk_minus1":
        assert cap == first_chunk - 1 and d["dropped"] >= 1
    elif name == "first_chunk_plus1":
        assert cap == first_chunk + 1
    elif name == "below_first_chunk":
        assert cap <= first_chunk and n > CHUNK
        assert d["chunks_past_capacity"] == sum(1 for j in range(1, es.chunks_of(n)) if P[min((j + 1) * CHUNK, n)] > P[j * CHUNK])
    elif name == "total":
        assert cap == d["total"] and d["dropped"] == 0
    elif name == "total_plus1":
        assert cap == d["total"] + 1 and d["dropped"] == 0
    else:
        raise AssertionError(name)


def test_patterns_reach_the_states_the_issue_lists():
    """properties of the builders alone (no simulation)"""
    for cap in es.PARENT_CAPS:
        pats = es.count_patterns(cap)
        names = set(pats)
        assert {"all31", "all32", "alt31_32", "every17th_33", "one_2pow30", "only_last_row", "zero", "ondie"} <= names
        assert {f"heavy1000_row{r}_rest{k}" for r in {0, CHUNK - 1, cap - 1} | ({CHUNK} if cap > CHUNK else set()) for k in (0, 1)} <= names
        assert (pats["all32"].c0 >= HEAVY).all() and (pats["all31"].c0 < HEAVY).all()
        assert int(es.prefix(pats["all32"].c0)[CHUNK]) == 131072                            # a full LDS queue: 4096 heavy rows in one chunk
        big = pats["one_2pow30"].c0
        assert big.max() == 1 << 30 and int(es.prefix(big)[-1]) < 1 << 31
        caps = es.named_capacities(big)
        assert "into_heavy_row" in caps and "total" not in caps                             # cut inside the heavy row, far from its end
        assert es.describe_cut(big, caps["into_heavy_row"])["dropped"] > 1 << 29
        assert np.nonzero(pats["only_last_row"].c0)[0].tolist() == [cap - 1]
        assert es.named_capacities(pats["zero"].c0) == {"one": 1}
        od = pats["ondie"]
        assert od.die.any() and (od.emitted(0)[od.die] == 0).all() and (od.emitted(1)[~od.die] == 0).all()
        assert (od.emitted(1) >= HEAVY).any() and ((od.emitted(1) > 0) & (od.emitted(1) < HEAVY)).any()
        if cap > CHUNK:
            for k in (0, 1):                                                                  # a heavy row at a chunk's last and first row
                assert pats[f"heavy1000_row{CHUNK - 1}_rest{k}"].c0[CHUNK - 1] == 1000 and pats[f"heavy1000_row{CHUNK}_rest{k}"].c0[CHUNK] == 1000
            assert "below_first_chunk" in es.named_capacities(pats["all31"].c0)
        for pname, pat in pats.items():
            for name, c0, c1 in es.probe_plan(pat):
                ch = 1 if pat.die.any() else 0
                _assert_named_state(name, pat.emitted(ch), c1 if ch else c0)
                assert es.child_class(c1 if ch else c0) >= (c1 if ch else c0)
        # a chunk that mixes light and heavy rows; every name of the issue's list is reached by some pattern
        assert ((pats["every17th_33"].c0[:CHUNK] >= HEAVY).any() and (pats["every17th_33"].c0[:CHUNK] < HEAVY).any())
        reached = set().union(*[{n for n, _, _ in es.probe_plan(p)} for p in pats.values()])
        want = {"one", "row_first_event", "into_light_row", "into_heavy_row", "first_chunk_total", "first_chunk_minus1", "first_chunk_plus1", "total", "total_plus1"}
        assert reached >= want | ({"below_first_chunk"} if cap > CHUNK else set())


def _oracle_probes(cap, patterns):
    pr = es.Probes([LinkedOracle()], cap)
    alive0 = pr.oracle.fx["P"].alive_list()
    assert len(alive0) == cap and not np.array_equal(alive0, np.arange(cap))       # the list is not the identity: events follow rows, not slots
    assert np.array_equal(np.sort(alive0), np.arange(cap))
    for pname, pat in patterns.items():
        for name, c0, c1 in es.probe_plan(pat):
            caps = {0: c0, 1: c1}

            def on_emitted(parent, alive):
                for ch, ev_cap in caps.items():
                    if ev_cap is None:
                        continue
                    counts = pat.emitted(ch)
                    n, ev = parent.events(ch)
                    assert n == int(es.prefix(counts)[-1]), (pname, name, ch)           # event_count keeps counting past the capacity
                    want_n, want = es.expected_recording(pat, ch, ev_cap, alive)
                    assert want_n == min(n, ev_cap) and np.array_equal(ev[:want_n], want), (pname, name, ch)

            children, parent_state, alive = pr.probe(pat, c0, c1, on_emitted=on_emitted, what=f"{pname}/{name}")
            for ch, ev_cap in caps.items():
                if ev_cap is None:
                    continue
                st = children[f"c{ch}"]
                want_n, want = es.expected_recording(pat, ch, ev_cap, alive)
                # the child IS the buffer: row i of its list is slot i, and U32_3 there is the ID of the particle behind event i
                assert st["counters"]["alive_count"] == want_n and np.array_equal(st["alive"], np.arange(want_n)), (pname, name, ch)
                assert np.array_equal(st["attrs"][A.U32_3.name][:want_n, 0], want), (pname, name, ch)
            if pat.die.any():
                assert not np.array_equal(pr.oracle.fx["P"].alive_list(), alive)      # rows died and were refilled: the next probe sees another list
    pr.close()


@pytest.mark.parametrize("cap", es.PARENT_CAPS)
def test_oracle_reaches_every_named_state_and_the_child_is_the_buffer(cap):
    _oracle_probes(cap, es.count_patterns(cap))


def test_oracle_split_patterns_store_everything():
    for cap in sorted({c for c, _, _, _ in es.SPLIT_CASES}):
        pr = es.Probes([LinkedOracle()], cap)
        for pcap, ev_cap, _, name in es.SPLIT_CASES:
            if pcap != cap:
                continue
            pat = es.split_patterns(cap)[name]
            children, _, alive = pr.probe(pat, ev_cap, None)
            n, want = es.expected_recording(pat, 0, ev_cap, alive)
            assert n == min(int(es.prefix(pat.c0)[-1]), ev_cap) and children["c0"]["counters"]["alive_count"] == n
            assert np.array_equal(children["c0"]["attrs"][A.U32_3.name][:n, 0], want)
        pr.close()


# ---- the frozen-link rule, hand-evaluated ----------------------------------------------------------------------------------------------------
def _tiny(frozen_at):
    """test_events.tiny_system by name: 4 parents of 3 frames' lifetime emit 2 events each per frame on channel 0 (capacity 5) and 3 each on
    death on channel 1; returns the children's alive counts after every frame."""
    o = LinkedOracle()
    o.add("P", tiny_parent())
    o.add("C0", tiny_child())
    o.add("C1", tiny_child())
    o.link("C0", "P", 0, 5)
    o.link("C1", "P", 1, 256)
    out = []
    for f in range(8):
        frames = {"P": Frame(1 / 60, 4 if f == 0 else 0, 7 + f, time=f / 60), "C0": Frame(1 / 60, 0, 100 + f, time=f / 60), "C1": Frame(1 / 60, 0, 200 + f, time=f / 60)}
        o.step(frames, frozen_at.get(f, ()))
        out.append((o.fx["P"].alive_count(), o.fx["C0"].alive_count(), o.fx["C1"].alive_count(), o.fx["P"].events(0)[0], o.fx["P"].events(1)[0]))
    return out


def test_frozen_rule_hand_evaluated():
    # nobody frozen (test_events.test_oracle_event_semantics_hand_evaluated): 8 events requested, 5 stored per frame while the parents live
    assert _tiny({})[:5] == [(4, 0, 0, 8, 0), (4, 5, 0, 8, 0), (0, 10, 0, 0, 12), (0, 10, 12, 0, 0), (0, 10, 12, 0, 0)]
    # the parent frozen in frames 1 and 2: frame 1's children still consume frame 0's events, frame 2's read a count of 0 (not the stale 8);
    # the parent neither ages nor emits while frozen; thawed in frame 3 it goes on where it stood
    got = _tiny({1: ("P",), 2: ("P",)})
    assert got[:7] == [(4, 0, 0, 8, 0), (4, 5, 0, 0, 0), (4, 5, 0, 0, 0), (4, 5, 0, 8, 0), (0, 10, 0, 0, 12), (0, 10, 12, 0, 0), (0, 10, 12, 0, 0)]
    # child C0 frozen in frame 1: it consumes nothing, frame 0's events are lost; thawed in frame 2 it sees frame 1's events only
    got = _tiny({1: ("C0",)})
    assert got[:4] == [(4, 0, 0, 8, 0), (4, 0, 0, 8, 0), (0, 5, 0, 0, 12), (0, 5, 12, 0, 0)]
    # child C1 frozen in the frame that would have consumed the parents' deaths: all 12 are lost
    got = _tiny({3: ("C1",)})
    assert [g[2] for g in got] == [0] * 8


# ---- instance tables ---------------------------------------------------------------------------------------------------------------------------
def test_instance_table_script_on_the_oracle():
    a, b = LinkedOracle(), LinkedOracle()
    fa = es.run_instance_tables([a], 1)
    fb = es.run_instance_tables([b], 2)
    assert fa["frames"] == 30 and fb["calls_of_two"] >= 8 and fb["frames"] == 30 - fb["calls_of_two"]
    assert_same_linked_state(a.state(), b.state(), "one frame per call / two")
    assert set(a.fx) == {"P1", "P2", "P3", "C1", "C2", "C3", "C4", "C5"}
    cnt, ev = fa["counter"], fa["events"]
    t0, t1, t2 = es.TABLE_ALL_PARENTS_FROZEN
    kids = ("C1", "C2", "C3", "C4")
    assert any(cnt[t0][c] > cnt[t0 - 1][c] for c in kids)                 # the first frozen frame still consumes what was emitted before
    assert all(cnt[t2][c] == cnt[t1][c] == cnt[t0][c] for c in kids)      # then the counts read as 0: nothing stale is consumed again
    assert all(cnt[t2 + 2][c] > cnt[t2][c] for c in ("C2", "C3"))         # thawed (and rewritten), the links work again
    # every buffer overflows at some frame and holds less than its capacity at another; heavy and light rows; both channels in use
    assert max(ev[f]["P0"][0] for f in range(1, 12)) > 16 and max(ev[f]["P1"][0] for f in range(1, 12)) > 5000 and max(ev[f]["P2"][0] for f in range(1, 12)) > 70_000
    assert any(ev[f]["P0"][1] > 300 for f in range(1, 12)) and any(0 < ev[f]["P1"][1] < 300 for f in range(1, 12))
    assert cnt[29]["C5"] > 0 and cnt[22]["C1"] > cnt[17]["C1"]           # the late instance's child and the re-parented child spawn
    assert cnt[9]["C3"] == cnt[6]["C3"] and cnt[11]["C3"] > cnt[9]["C3"]  # the frozen child consumed nothing for three frames


# ---- slot reuse ----------------------------------------------------------------------------------------------------------------------------------
def test_slot_reuse_script_on_the_oracle():
    o = LinkedOracle()
    old, st = es.run_slot_reuse([o])
    child, parent = st["C"], st["P"]
    n = child["counters"]["alive_count"]
    assert n == 2 * CHUNK and parent["counters"]["alive_count"] == CHUNK        # every particle died, emitted 2 events, and every slot was re-burst
    new = parent["attrs"][A.F32_0.name].view(np.float32)[:, 0]
    assert (new != old[:, 0]).mean() > 0.99
    got = child["attrs"][A.F32_1.name].view(np.float32)[:n, 0]
    slots = np.repeat(np.arange(CHUNK), 2)                                       # the list was the identity when they died: event 2 r and 2 r + 1 name slot r
    read_new = got == new[slots]
    assert read_new.all() and (got != old[slots, 0]).any()                       # the child read the slot's NEW occupant (the init passes run parents first)
    assert np.array_equal(child["attrs"][A.POSITION.name][:n], parent["attrs"][A.POSITION.name][slots])


# ---- the sibling fuzz ------------------------------------------------------------------------------------------------------------------------------
def test_fuzz_generator_covers_heavy_rows_and_is_stable():
    heavy, spawned = 0, 0
    for seed in es.FUZZ_SEEDS[:4]:
        h, st = es.run_fuzz(seed, [LinkedOracle()], n_frames=12)
        heavy += h
        spawned += sum(s["counters"]["particle_counter"] for n, s in st.items() if n != "P")
    assert heavy > 100 and spawned > 1000
    p1, planes1, ch1 = es.fuzz_system(700)
    p2, planes2, ch2 = es.fuzz_system(700)
    import bevy_hanabi_amd as bh
    assert bh.serialize_asset(p1) == bh.serialize_asset(p2) and planes1 == planes2 and [c for _, c in ch1] == [c for _, c in ch2]
