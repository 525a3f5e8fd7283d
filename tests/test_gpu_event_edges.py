"""GPU spawn events at adversarial counts, splits and instance tables: k_emit_count / k_emit_events (and the event branch of k_init) against the
oracle, bit for bit, with the scripts of tests/event_scripts.py, on the specialised and on the interpreted kernels side by side against one run
of the oracle - tests/test_event_scripts.py asserts on the oracle alone that every case reaches the state it is named for and that the children
show the whole stored prefix of every buffer.

Which planted fault each case would notice (by reading the kernels; nothing is planted on a device):
  - ev_parity not flipped: every case. A child reads count[parity ^ 1]; with one parity for both sides it reads a count nobody wrote, and no child
    ever spawns - every probe stores at least one event, except the `zero` pattern, which pins the other direction (count 0 is published).
  - `c.k` dropped from the ev_totals index: the instance tables. Instances 1 and 2 would take instance 0's chunk totals: the one row of their
    second chunk lands at another event index and `excl + mine` is another count (the three parents emit different totals per chunk).
  - the count not republished by a frozen parent: the instance tables, frames 4-5 (one parent frozen: its children would read the count of
    two frames earlier) and 13-14 (every instance of the emitting program frozen).
  - the capacity clamp dropped from a writer: the store lands BEHIND the buffer, which no state read shows by itself. The cases in which a
    parent fills two buffers allocated one after the other (the `ondie` pattern: channel 0 overflows by half its total; the instance tables:
    16, 300, 5000 and 70,000 next to each other) are the ones in which such a store can land in a neighbour's header or prefix and be seen.
  - kEmitHeavy off by one, `row % n_split` replaced by `row / 16 % n_split`: both writers produce the same buffer and both rules are partitions of
    the rows, so neither changes a result; the cases around 31 / 32 / 33 and the odd split counts pin that the two writers and every split's
    share agree with the oracle at the boundary, which is what either change would have to preserve."""
import pytest

import bevy_hanabi_amd as bh
import event_scripts as es
from helpers import LinkedGpu, LinkedOracle

pytestmark = pytest.mark.gpu

_PROGRAMS = {}   # {kernels: {asset key: Program}}: a program per asset in that flavour's context, instances come and go


@pytest.fixture(scope="module")
def ctx():
    """a context per kernel flavour (hnb_simulate runs every effect of its context: two systems that step by themselves cannot share one)"""
    c = {"jit": bh.Context(0), "interp": bh.Context(0)}
    yield c
    _PROGRAMS.clear()
    for x in c.values():
        x.close()


def _both_kernels(ctx, monkeypatch, assets):
    """Two systems, one on the specialised and one on the interpreted kernels (HNB_JIT is read when a program is created: `assets`, the
    (key, asset) pairs the script will use, get their programs here) - both run the same script against ONE oracle."""
    out = []
    for mode in ("jit", "interp"):
        monkeypatch.setenv("HNB_JIT", "1" if mode == "jit" else "0")
        progs = _PROGRAMS.setdefault(mode, {})
        for key, a in assets:
            if key not in progs:
                progs[key] = ctx[mode].create_program(bh.lower(a))
        g = LinkedGpu(ctx[mode], progs)
        g.name = f"gpu, {mode} kernels"
        out.append(g)
    assert "jit" in out[0].programs[assets[0][0]].kernel_info()
    return out


def _probe_assets(cap, child_caps=es.CHILD_CLASSES):
    return [es.asset("parent", cap)] + [es.asset("child", c, None) for c in child_caps]


def _pattern_cases():
    return [(cap, name) for cap in es.PARENT_CAPS for name in es.count_patterns(cap)]


@pytest.mark.parametrize("cap,name", _pattern_cases(), ids=lambda v: str(v))
def test_gpu_count_pattern_at_every_named_capacity(ctx, monkeypatch, cap, name):
    """One pattern of per-row counts on a parent whose list is not the identity, at every capacity its running sum names: 1, a row's first event,
    one event into a light / a heavy row, the first chunk's total and +-1, below it on a parent of several chunks, the total and total + 1."""
    pat = es.count_patterns(cap)[name]
    pr = es.Probes([LinkedOracle()] + _both_kernels(ctx, monkeypatch, _probe_assets(cap)), cap)
    try:
        for cname, c0, c1 in es.probe_plan(pat):
            pr.probe(pat, c0, c1, what=f"{name}/{cname} capacity {c0}/{c1}")
    finally:
        pr.close()


@pytest.mark.parametrize("case", es.SPLIT_CASES, ids=lambda c: f"{c[0]}-{c[1]}-splits{c[2]}-{c[3]}")
def test_gpu_heavy_rows_dealt_over_1_2_3_5_splits(ctx, monkeypatch, case):
    cap, ev_cap, splits, name = case
    gpus = _both_kernels(ctx, monkeypatch, _probe_assets(cap))
    pr = es.Probes([LinkedOracle()] + gpus, cap)
    try:
        for g in gpus:
            assert len(g.programs[es.asset("parent", cap)[0]]._effects) == 1        # the grid is sized over every instance of the program: one here
        assert es.size_event_grid(ev_cap, es.chunks_of(cap)) == splits
        pr.probe(es.split_patterns(cap)[name], ev_cap, None, what=f"{name} over {splits} splits")
    finally:
        pr.close()


def test_gpu_heavy_rows_dealt_over_64_splits(ctx, monkeypatch):
    """4096 heavy rows, a buffer and a child of 1,048,576: the cap of plan::size_event_grid, the cut inside a heavy row of the last split's"""
    pr = es.Probes([LinkedOracle()] + _both_kernels(ctx, monkeypatch, _probe_assets(es.CHUNK, (es.SPLIT64_CAPACITY,))), es.CHUNK)
    try:
        assert es.size_event_grid(es.SPLIT64_CAPACITY, 1) == 64
        children, _, _ = pr.probe(es.split64_pattern(), es.SPLIT64_CAPACITY, None, child_caps={0: es.SPLIT64_CAPACITY}, what="64 splits")
        assert children["c0"]["counters"]["alive_count"] == es.SPLIT64_CAPACITY
    finally:
        pr.close()


@pytest.mark.parametrize("steps_per_call", [1, 2])
def test_gpu_instance_tables(ctx, monkeypatch, steps_per_call):
    """Three instances of one emitting program, five of one child program with their own parent, channel and capacity; frozen parents, a frozen
    child, every parent frozen at once; a parent destroyed (the last instance takes its index) after one child was re-parented and the other
    destroyed; a fourth parent on the freed slab. steps_per_call 2: through hnb_simulate_steps (programs with events take the single-frame path)."""
    gpus = _both_kernels(ctx, monkeypatch, [es.asset("parent", es.TABLE_PARENT_CAP), es.asset("child", es.TABLE_CHILD_CAPACITY, es.TABLE_CHILD_LIFETIME)])
    try:
        facts = es.run_instance_tables([LinkedOracle()] + gpus, steps_per_call)
        assert facts["frames"] + facts["calls_of_two"] == 30
        for g in gpus:
            assert g.fx["P2"].index() == 0 and g.fx["P3"].index() == 2
    finally:
        for g in gpus:
            g.destroy()


@pytest.mark.parametrize("overlap", [1, 0])
def test_gpu_child_reads_the_new_occupant_of_a_reused_slot(overlap):
    c = bh.Context(0)
    c.set_option("overlap_updates", overlap)
    try:
        es.run_slot_reuse([LinkedOracle(), LinkedGpu(c)])
    finally:
        c.close()


@pytest.mark.parametrize("order", ["spawn", "slot"])
@pytest.mark.parametrize("seed", es.FUZZ_SEEDS)
def test_gpu_fuzz_counts_around_the_heavy_threshold(seed, order, monkeypatch):
    """spawn order on the specialised kernels, slot order on the interpreters"""
    monkeypatch.setenv("HNB_JIT", "1" if order == "spawn" else "0")
    c = bh.Context(0)
    c.set_list_order(order)
    try:
        es.run_fuzz(seed, [LinkedOracle(slot_order=order == "slot"), LinkedGpu(c)])
    finally:
        c.close()
