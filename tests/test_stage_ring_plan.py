"""plan::stage_ring_begin / _end / _drained (bevy_hanabi_amd/csrc/hnb_plan.h) without a device: the bookkeeping of the staging ring of the frames'
parameter blocks - sixteen slots, one completion event per group of four staged frames - driven the way simulate_frame drives it, beside a
brute-force model of the stream. The invariant: the host rewrites a slot only after an event has completed that was recorded behind the last frame
that read the slot (or after the stream itself was waited for). The model is as pessimistic as a device can be: nothing enqueued is ever complete
unless the host has waited for an event recorded behind it, or for the stream."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "stage_ring")
NONE, STREAM = -1, -2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    """The shim is compiled here, from the file beside this test, into a temporary directory."""
    so = str(tmp_path_factory.mktemp("stage_ring") / "libstage_ring.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", os.path.join(HERE, "stage_ring.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.srp_new.restype = C.c_void_p
    L.srp_free.argtypes = [C.c_void_p]
    L.srp_consts.argtypes = [C.POINTER(C.c_uint32)]
    L.srp_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
    L.srp_drained.argtypes = [C.c_void_p]
    L.srp_end.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.srp_staged.restype = C.c_uint32
    L.srp_staged.argtypes = [C.c_void_p]
    L.srp_set_staged.argtypes = [C.c_void_p, C.c_uint32]
    return L


def consts(lib):
    out = (C.c_uint32 * 3)()
    lib.srp_consts(out)
    return tuple(out)


class Ctx:
    """A context as simulate_frame sees it: the plan's state, and the stream as the brute-force model knows it. Positions count what was enqueued
    on the stream (readers of a slot, event records); `done` is the last position the HOST knows to be complete."""

    def __init__(self, lib):
        self.lib, self.h = lib, lib.srp_new()
        self.slots, self.group, self.groups = consts(lib)
        self.pos, self.done = 0, 0
        self.last_reader = {}          # slot -> position of the last launch that reads it
        self.rec_pos = {}              # event -> position of its last record
        self.rec_frames = {}           # event -> whole staged frames at its last record
        self.ctx_frame = 0             # the context's frame counter: whole frames, empty ones included
        self.whole = 0                 # staged frames enqueued whole
        self.enqueued = 0              # frames that enqueued work (whole or not)
        self.records = 0
        self.log = []                  # per call of frame(): (kind, slot or None, wait, record)
        self.stream_waits = self.event_waits = 0
        self.failed_since_drain = False

    def close(self):
        self.lib.srp_free(self.h)

    def _wait(self, wait):
        if wait == STREAM:
            self.done = self.pos
            self.stream_waits += 1
            self.lib.srp_drained(self.h)
            self.failed_since_drain = False
        elif wait != NONE:
            assert wait in self.rec_pos, f"waits for event {wait}, which was never recorded"
            self.done = max(self.done, self.rec_pos[wait])
            self.event_waits += 1

    def realloc(self):
        """ensure_stage re-creates the slots (the block grew, the upload path changed): it waits for the stream first."""
        self.done = self.pos
        self.lib.srp_drained(self.h)
        self.failed_since_drain = False
        self.last_reader.clear()

    def frame(self, kind):
        """kind: 'empty' (nothing to enqueue), 'ok', 'fail_early' (fails in front of the slot's write: nothing enqueued), 'fail_late' (fails behind it:
        some launches are enqueued and read the slot). Returns (slot, wait, record)."""
        stages = kind != "empty"
        slot = C.c_uint32(0)
        wait = self.lib.srp_begin(self.h, int(stages), C.byref(slot))
        slot = slot.value if stages else None
        if not stages:
            assert wait == NONE
        if wait == STREAM:
            assert self.failed_since_drain, "waits for the stream although no frame failed"
        elif wait != NONE:
            assert slot % self.group == 0 and wait == slot // self.group
            assert self.whole - self.rec_frames[wait] == self.slots - self.group, "the host may run a whole ring minus one group ahead"
        self._wait(wait)
        record = NONE
        if kind == "fail_early":
            return slot, wait, record                       # (HIP_TRY returned in front of the write: the plan is not told anything)
        if stages:
            # THE INVARIANT: the host writes the slot now
            assert self.last_reader.get(slot, 0) <= self.done, f"slot {slot} rewritten while a launch at {self.last_reader[slot]} may still read it (done {self.done})"
            self.pos += 1
            self.last_reader[slot] = self.pos               # the frame's launches (a failed frame: some of them)
            self.enqueued += 1
        ok = kind in ("ok", "empty")
        record = self.lib.srp_end(self.h, int(stages), 1, int(ok))
        if not ok:
            assert record == NONE
            self.failed_since_drain = True
            return slot, wait, record
        if record != NONE:
            assert stages and 0 <= record < self.groups
            self.pos += 1
            self.rec_pos[record] = self.pos
            self.records += 1
        self.ctx_frame += 1
        if stages:
            self.whole += 1
            if record != NONE:
                self.rec_frames[record] = self.whole
        assert self.lib.srp_staged(self.h) == self.whole & 0xFFFFFFFF
        assert self.records * self.group <= self.whole       # at most one record per kStageGroup frames that enqueued work
        return slot, wait, record

    def run(self, kinds):
        return [self.frame(k) for k in kinds]


def test_constants(lib):
    assert consts(lib) == (16, 4, 4)


def test_first_lap_then_the_second(lib):
    c = Ctx(lib)
    got = c.run(["ok"] * 16)
    assert [s for s, _, _ in got] == list(range(16))
    assert all(w == NONE for _, w, _ in got)                                   # nothing to wait for: no slot has been used
    assert [r for _, _, r in got] == [NONE, NONE, NONE, 0, NONE, NONE, NONE, 1, NONE, NONE, NONE, 2, NONE, NONE, NONE, 3]
    got = c.run(["ok"] * 20)
    assert [s for s, _, _ in got] == [i % 16 for i in range(16, 36)]
    assert [w for _, w, _ in got] == [0, NONE, NONE, NONE, 1, NONE, NONE, NONE, 2, NONE, NONE, NONE, 3, NONE, NONE, NONE, 0, NONE, NONE, NONE]
    assert c.records == 9 and c.stream_waits == 0
    c.close()


def test_only_empty_frames(lib):
    c = Ctx(lib)
    got = c.run(["empty"] * 100)
    assert all(g == (None, NONE, NONE) for g in got)
    assert c.records == 0 and c.whole == 0 and c.ctx_frame == 100 and c.pos == 0
    assert c.frame("ok") == (0, NONE, NONE)                                    # ... and the first staged frame starts the ring
    c.close()


def test_an_empty_frame_where_a_group_would_close(lib):
    """Slots are counted in staged frames: the empty frames take none and close nothing; the group closes behind its fourth staged frame."""
    c = Ctx(lib)
    got = c.run(["ok", "ok", "ok", "empty", "empty", "ok", "ok"])
    assert got == [(0, NONE, NONE), (1, NONE, NONE), (2, NONE, NONE), (None, NONE, NONE), (None, NONE, NONE), (3, NONE, 0), (4, NONE, NONE)]
    c.run(["ok", "empty"] * 30)                                                # laps with an empty frame behind every staged one
    assert c.records == c.whole // 4
    c.close()


def test_a_failure_in_a_groups_closing_frame(lib):
    c = Ctx(lib)
    c.run(["ok"] * 3)
    assert c.frame("fail_late") == (3, NONE, NONE)                             # no record: the frame does not count
    assert c.ctx_frame == 3
    assert c.frame("fail_late") == (3, STREAM, NONE)                           # the retry rewrites slot 3 beside the first attempt's launches: the stream
    assert c.frame("ok") == (3, STREAM, 0)                                     # ... and again; now the group closes
    assert c.frame("ok") == (4, NONE, NONE)
    c.run(["ok"] * 11)
    assert c.frame("ok") == (0, 0, NONE)                                       # the second lap waits for the record of the retried frame
    # a failure in front of the write leaves nothing behind
    c2 = Ctx(lib)
    c2.run(["ok"] * 3)
    assert c2.frame("fail_early") == (3, NONE, NONE)
    assert c2.frame("ok") == (3, NONE, 0)
    assert c2.stream_waits == 0
    # a failed closing frame on a later lap: the drained ring waits for no event of the lap before, and still never breaks the invariant
    c3 = Ctx(lib)
    c3.run(["ok"] * 19)
    assert c3.frame("fail_late") == (3, NONE, NONE)
    assert c3.frame("ok") == (3, STREAM, 0)
    got = c3.run(["ok"] * 16)
    assert [w for _, w, _ in got] == [NONE] * 12 + [0, NONE, NONE, NONE]       # groups 1 .. 3 were drained with the stream; group 0 has a new record
    c.close(); c2.close(); c3.close()


def test_a_span_that_straddles_a_group_boundary(lib):
    """hnb_simulate_steps: the fused launch of a span is enqueued in the span's first frame and reads ITS slot; the frames it covers stage nothing
    (a context with one program) or stage the other programs' blocks (several). Either way the record that guards the span's slot stands behind
    the span's launch."""
    c = Ctx(lib)
    got = c.run(["ok", "ok", "ok"] + ["empty"] * 4 + ["ok"])                   # frame 2 launches a span of five: frames 3 .. 6 are covered
    assert got[2] == (2, NONE, NONE) and got[7] == (3, NONE, 0)
    assert c.last_reader[2] < c.rec_pos[0]
    c.run(["ok"] * 12)
    assert c.frame("ok") == (0, 0, NONE)
    # several programs: the covered frames are staged frames of the others
    c2 = Ctx(lib)
    got = c2.run(["ok"] * 8)                                                   # frame 2's span reaches over the boundary at frame 3 / 4
    assert got[3] == (3, NONE, 0) and c2.last_reader[2] < c2.rec_pos[0]
    c.close(); c2.close()


def test_reallocation_drains_the_ring(lib):
    c = Ctx(lib)
    c.run(["ok"] * 22)
    c.realloc()
    got = c.run(["ok"] * 26)                                                   # frames 22 .. 47
    assert c.stream_waits == 0
    # no event of the laps before the drain is waited for (groups 2, 3, 0 at frames 24, 28, 32); the events recorded since are (frames 36, 40, 44)
    waits = [(s, w) for s, w, _ in got if w != NONE]
    assert waits == [(4, 1), (8, 2), (12, 3)], waits
    c.close()


def test_the_counter_wraps_onto_the_same_slot(lib):
    c = Ctx(lib)
    lib.srp_set_staged(c.h, 0xFFFFFFFE)
    c.whole = 0xFFFFFFFE
    assert c.frame("ok")[0] == 14
    s, _, r = c.frame("ok")
    assert (s, r) == (15, 3)
    c.whole = c.records = 0                                                    # (the model's counts follow the 32-bit counter)
    assert c.frame("ok")[0] == 0
    c.close()


def test_random_sequences_hold_the_invariant(lib):
    rng = random.Random(4016)
    total_waits = total_fail = total_span = 0
    for trial in range(2000):
        c = Ctx(lib)
        p_empty = rng.choice([0.0, 0.1, 0.5, 0.9])
        p_fail = rng.choice([0.0, 0.02, 0.1])
        p_span = rng.choice([0.0, 0.1, 0.4])
        several = rng.random() < 0.5                                           # programs beside the one that fuses: covered frames still stage
        n = rng.randint(1, 140)
        f = 0
        while f < n:
            r = rng.random()
            if r < p_empty:
                c.frame("empty"); f += 1
            elif r < p_empty + p_fail:
                c.frame(rng.choice(["fail_early", "fail_late"])); f += 1       # (the caller tries again, or goes on to other frames: both follow)
                total_fail += 1
            elif r < p_empty + p_fail + p_span:
                span = rng.randint(1, 8)
                _, _, _ = c.frame("ok")
                for _ in range(span - 1):                                      # the frames the span covers
                    kind = "ok" if several and rng.random() < 0.7 else "empty"
                    if rng.random() < p_fail:
                        c.frame("fail_late" if kind == "ok" else "empty")      # a failed frame ends the call: the rest of the span's frames never come
                        break
                    c.frame(kind)
                f += span
                total_span += 1
            else:
                c.frame("ok"); f += 1
            if rng.random() < 0.01:
                c.realloc()
        assert c.records * c.group <= c.whole
        assert c.records <= c.enqueued // c.group
        total_waits += c.event_waits
        c.close()
    assert total_fail > 500 and total_span > 5000 and total_waits > 1000      # (the generator does reach laps, failures and spans)
