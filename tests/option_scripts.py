"""The option space of hnb_ctx_set_option (include/hanabi_amd.h: "same results bit for bit with either value") as data for tests:

  CLASSES        every key of runtime.OPTIONS in exactly one class: "creation" (fixed in a program when it is created), "frame" (applies from the
                 next hnb_simulate on) or "excluded" (with the reason). tests/test_option_scripts.py fails when runtime.OPTIONS gains a key that is
                 not classified here; tests/test_gpu_option_matrix.py runs every creation / frame option, singly and switched between frames.
  scripts        life cycles of four assets that take the chunks of the streaming update kernel through every state its per-chunk words encode
                 (completely alive, uniform age, mixed ages, the one-in-sixteen staggered re-check, empty, refilled). Which states a script reaches is
                 asserted ON THE ORACLE ALONE (tests/test_option_scripts.py), so that the GPU tests cannot pass without having been through them.
  Trace          the oracle's run of a script, computed once per process and shared: one digest of the whole state per frame (counters, both lists,
                 every plane) and the per-chunk facts. A GPU state whose digest differs is compared plane by plane against a re-run of the oracle.
  fuzz frames    random_frames with a burst of the whole capacity, so that random programs hold completely alive chunks.
  kernel_info    a parser of the counters hnb_program_kernel_info prints.

`stream_hints` stays in the frame class so that its plumbing runs (SlotArgs::stream_hint, the list kernels' load policy), but its nontemporal kernel
variants engage only above 256 MiB of traffic per frame (plan::use_streaming_hints): nothing here is that large, and these tests do not claim to cover
those variants. The same holds for `overlap_updates`: the second stream is used only when one program of a context holds a million slots or more and
at least four times the slots of all the others together (hanabi_amd.h, HNB_OPT_OVERLAP_UPDATES); no context here is that large, so only the option's
plumbing runs (tests/test_device_view.py has a two-stream frame). `fuse_steps` acts on hnb_simulate_steps alone and fuses only programs of more than
16 chunks: it has a case of its own at 17 chunks, with hnb_ctx_step_stats asserted in both directions.
"""
import functools
import hashlib
import re

import numpy as np

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects
from helpers import A, Frame, OracleRunner, assert_same_state, frame_seed, translation

CHUNK = 4096   # slots per chunk of the streaming update kernel (kChunk): the granularity of lmin / cfull / the cohort state

# ---- classification ------------------------------------------------------------------------------------------------------------------------
# class, legal values (default first for "frame" / "creation"), or the reason of an exclusion
CLASSES = {
    "age_cohort": ("creation", (3, 0, 1, 2)),
    "cull_lifetime": ("creation", (1, 0)),
    "horizon": ("creation", (1, 0)),
    "alternate": ("frame", (1, 0)),
    "skip_lists": ("frame", (1, 0)),
    "transpose": ("frame", (1, 0)),
    "scene_merge": ("frame", (1, 0)),
    "suffix_proof": ("frame", (1, 0)),
    "ring_lists": ("frame", (1, 0)),
    "slot_init": ("frame", (1, 0, 2)),
    "overlap_updates": ("frame", (1, 0)),
    "stream_hints": ("frame", (1, 0)),
    "direct_upload": ("frame", (1, 0)),
    "fuse_steps": ("frame", (1, 0)),
    "test_break_proof": ("excluded", "a fault hook: it breaks a proof on purpose (tests/test_verification.py, tests/test_gpu_verification_faults.py)"),
    "jit_async": ("excluded", "has its own file and costs compile minutes (tests/test_gpu_simulate_steps_jit.py, tests/test_jit_fused_steps.py)"),
    "set_module": ("excluded", "has its own file and costs compile minutes (tests/test_set_module.py); the merged-launch case here runs OFF and CACHED"),
    "list_order": ("excluded", "changes the result (a second legal list order) and is covered widely (tests/test_gpu_parity.py test_slot_order_*)"),
}
CREATION = tuple(k for k, v in CLASSES.items() if v[0] == "creation")
FRAME = tuple(k for k, v in CLASSES.items() if v[0] == "frame")
EXCLUDED = {k: v[1] for k, v in CLASSES.items() if v[0] == "excluded"}
DEFAULTS = {k: CLASSES[k][1][0] for k in CREATION + FRAME}
# every proof and hint off: bench.py's PLAIN_OPTIONS restated (tests/test_option_scripts.py holds the two against each other)
PLAIN = {"horizon": 0, "age_cohort": 0, "cull_lifetime": 0, "skip_lists": 0, "stream_hints": 0, "overlap_updates": 0,
         "suffix_proof": 0, "ring_lists": 0, "alternate": 0, "transpose": 0, "scene_merge": 0, "slot_init": 0, "direct_upload": 0}


def values_of(option):
    return CLASSES[option][1]


def base_value(base, option):
    """the value `option` has in a context that was given the options `base` (a dict over the defaults)"""
    return base.get(option, DEFAULTS[option])


def single_flips(base, options=None):
    """[(option, value)]: every creation / frame option (or those of `options`) at every legal value it does not have in `base`"""
    return [(k, v) for k in (options or CREATION + FRAME) for v in values_of(k) if v != base_value(base, k)]


def flip_id(flip):
    return f"{flip[0]}={flip[1]}"


def make_context(options, device=0):
    c = bh.Context(device)
    for k, v in options.items():
        c.set_option(k, v)
    return c


# ---- scripts ---------------------------------------------------------------------------------------------------------------------------------
FIREWORK_CAP = 3 * CHUNK + 77


def _quiet(first, last, dt=1 / 60):
    return [Frame(dt, 0, frame_seed(f), time=f / 60) for f in range(first, last + 1)]


def firework_frames(cap):
    """effects.firework_trails(cap), lifetimes 0.8 - 1.2 s: burst; flight (every chunk completely alive, one age); the die-off from frame 48 on;
    cap // 14 spawns at frame 70 into every chunk (mixed ages); 33 quiet frames in which the chunks hold one age again, partly filled (two re-check
    periods of 16), one of them with another dt and one with dt = 0; a re-burst at 104 (completely alive AND mixed); everything dies; a last burst into
    the empty effect, its flight, and its first deaths."""
    few = 900 if cap == FIREWORK_CAP else max(1, cap // 14)
    fr = [Frame(1 / 60, cap, frame_seed(0))] + _quiet(1, 69)
    fr += [Frame(1 / 60, few, frame_seed(70), time=70 / 60)] + _quiet(71, 89)
    fr += [Frame(1 / 24, 0, frame_seed(90), time=90 / 60), Frame(0.0, 0, frame_seed(91), time=91 / 60)] + _quiet(92, 103)
    fr += [Frame(1 / 60, cap, frame_seed(104), time=104 / 60)] + _quiet(105, 124)
    fr += _quiet(125, FIREWORK_EMPTY_BY)
    fr += [Frame(1 / 60, cap, frame_seed(FIREWORK_EMPTY_BY + 1), time=(FIREWORK_EMPTY_BY + 1) / 60)] + _quiet(FIREWORK_EMPTY_BY + 2, FIREWORK_EMPTY_BY + 21)
    # ... and on to the first deaths of that burst, met by a tick chosen so that they come as early behind the smallest lifetime (0.8 s) as a frame can
    # bring them: the death horizons (a row chunk's "nobody dies before this clock value") are then within 2^-9 of being wrong
    fr += _quiet(FIREWORK_EMPTY_BY + 22, FIREWORK_TIGHT - 1)
    fr += [Frame(FIREWORK_TIGHT_DT, 0, frame_seed(FIREWORK_TIGHT), time=FIREWORK_TIGHT / 60)] + _quiet(FIREWORK_TIGHT + 1, FIREWORK_TIGHT + 2)
    return fr


FIREWORK_EMPTY_BY = 180   # 1.2 s after the re-burst of frame 104 is frame 176: the oracle's alive_count is 0 here (asserted)
FIREWORK_TIGHT = FIREWORK_EMPTY_BY + 1 + 47        # the burst's frame and 46 more at 1/60 s: every age is 47/60 = 0.78333 s ...
FIREWORK_TIGHT_DT = 0.8 + 0.0005 - 47 / 60         # ... and this tick takes it to 0.8005 s: past the lifetimes in [0.8, 0.8005)


def firework_short_frames(cap):
    """the same shape in 96 frames for the 65,535 / 65,536-slot runs: burst, flight, die-off, partial respawn, re-burst, die-off"""
    fr = [Frame(1 / 60, cap, frame_seed(0))] + _quiet(1, 59)
    fr += [Frame(1 / 60, cap // 14, frame_seed(60), time=1.0)] + _quiet(61, 79)
    fr += [Frame(1 / 60, cap, frame_seed(80), time=80 / 60)] + _quiet(81, 95)
    return fr


def force_field_frames(cap):
    """effects.force_field(cap): lifetime 10 s, two kill modifiers (not horizon eligible, a non-flat vec3 stack: the transpose path). Burst; 60 frames
    with a property change; ten quarter-second ticks that throw particles out of the allowed box (deaths by the kill modifiers, age < lifetime); a
    partial respawn into the freed slots; then quarter-second ticks that age everything to death; a re-burst and 20 frames."""
    fr = [Frame(1 / 60, cap, frame_seed(0))] + _quiet(1, 59)
    fr[40].props = {"repulsor_position": (0.1, 0.2, 0.0), "repulsor_accel": -25.0}
    fr += [Frame(0.25, 0, frame_seed(f), time=f / 60) for f in range(60, 70)]
    fr += [Frame(1 / 60, max(1, cap // 14), frame_seed(70), time=70 / 60)] + _quiet(71, 79)
    fr += [Frame(0.25, 0, frame_seed(f), time=f / 60) for f in range(80, 80 + FORCE_FIELD_AGEING)]
    n = 80 + FORCE_FIELD_AGEING
    fr += [Frame(1 / 60, cap, frame_seed(n), time=n / 60)] + _quiet(n + 1, n + 20)
    return fr


FORCE_FIELD_AGEING = 44   # 44 x 0.25 s = 11 s > the 10 s lifetime


def ribbon_frames(cap):
    """effects.ribbon(cap) under its rate spawner (capacity / lifetime per second) and a moving emitter: fill (90 frames), steady churn in which the
    oldest rows die while spawns arrive (ring lists, the suffix proof, the sort), the spawner switched off until the trail has died out, switched on
    again."""
    asset = effects.ribbon(cap)
    sp, rng = bh.EffectSpawner(asset.spawner), bh.Pcg32()
    fr = []
    for f in range(230):
        t = f / 60.0
        n = sp.tick(1 / 60, rng)
        spawn = n if f < 110 or f >= 205 else 0
        fr.append(Frame(1 / 60, spawn, frame_seed(f), translation(np.sin(t), np.cos(t), 0.0), time=t))
    return fr


SCRIPTS = {
    "firework": (effects.firework_trails, firework_frames),
    "firework_short": (effects.firework_trails, firework_short_frames),
    "force_field": (effects.force_field, force_field_frames),
    "ribbon": (effects.ribbon, ribbon_frames),
}
FORCE_FIELD_CAP = CHUNK + 77
RIBBON_CAP = 2 * CHUNK + 5
FUSE_CAP = 17 * CHUNK     # hnb_simulate_steps fuses spans only for programs that are never candidates for the merged launches: more than 16 chunks
AUTO_THRESHOLD = 65536   # HNB_AGE_COHORT_AUTO keeps the cohorts (and the plane current) from this many slots on, where the render modifiers read AGE


# ---- the oracle's run of a script ---------------------------------------------------------------------------------------------------------------
def state_digest(st):
    h = hashlib.blake2b(digest_size=16)
    h.update(repr(sorted((k, int(v)) for k, v in st["counters"].items())).encode())
    for x in (st["alive"], st["dead"]):
        h.update(np.ascontiguousarray(x, dtype=np.uint32).tobytes())
        h.update(b"|")
    for k in sorted(st["attrs"]):
        h.update(k.encode())
        h.update(np.ascontiguousarray(st["attrs"][k]).view(np.uint32).tobytes())
    return h.digest()


def chunk_facts(st, cap):
    """per chunk of 4096 slots: (slots, alive, distinct AGE bit patterns among the alive) from the alive list and the AGE plane"""
    n_chunks = (cap + CHUNK - 1) // CHUNK
    alive = np.asarray(st["alive"], dtype=np.int64)
    ages = np.asarray(st["attrs"]["age"]).view(np.uint32).reshape(-1)[alive]
    chunk_of = alive // CHUNK
    out = []
    for j in range(n_chunks):
        sel = chunk_of == j
        out.append((min(CHUNK, cap - j * CHUNK), int(sel.sum()), len(np.unique(ages[sel]))))
    return out


class Trace:
    """The oracle's states of one script, frame by frame, as digests and chunk facts."""

    def __init__(self, name, cap):
        self.name, self.cap = name, cap
        make_asset, make_frames = SCRIPTS[name]
        self.asset = make_asset(cap)
        self.frames = make_frames(cap)
        self.digests, self.facts, self.alive_counts, self.row_ages, self.kill_deaths = [], [], [], [], 0
        orc = OracleRunner(self.asset, omp=self.cap >= 1 << 15)
        has_life = any(a.name == "lifetime" for a in self.asset.particle_layout())
        prev = None
        for fr in self.frames:
            orc.step(fr)
            st = orc.state()
            self.digests.append(state_digest(st))
            self.facts.append(chunk_facts(st, cap))
            self.alive_counts.append(len(st["alive"]))
            ages = st["attrs"]["age"].reshape(-1)
            self.row_ages.append(hashlib.blake2b(np.ascontiguousarray(ages[st["alive"]]).tobytes(), digest_size=16).digest())
            if has_life and prev is not None:   # gone from the alive list although the age it left behind is below its lifetime: a kill modifier
                gone = np.setdiff1d(prev, st["alive"], assume_unique=True)
                self.kill_deaths += int((ages[gone].view(np.float32) < st["attrs"]["lifetime"].reshape(-1)[gone].view(np.float32)).sum())
            prev = st["alive"]

    # -- chunk states, as the update kernel's words see them
    def full(self, f, j):
        slots, alive, _ = self.facts[f][j]
        return alive == slots

    def kernel_full(self, f, j):
        return self.facts[f][j][1] == CHUNK     # cfull: 4096 alive slots counted (a ragged last chunk never is)

    def uniform(self, f, j):
        return self.facts[f][j][1] > 0 and self.facts[f][j][2] == 1

    def mixed(self, f, j):
        return self.facts[f][j][2] > 1

    def n_chunks(self):
        return len(self.facts[0])

    def transitions(self):
        """{name: first frame at which the transition is seen (the state AFTER that frame), or None}; "uniform_run": the longest run of frames in
        which some chunk that was mixed before stays uniform"""
        t = {"full_to_not_full": None, "uniform_to_mixed": None, "mixed_to_uniform": None, "full_and_mixed": None, "all_dead": None, "empty_to_full": None, "refilled_to_not_full": None}
        best_run = 0
        for j in range(self.n_chunks()):
            run, was_mixed = 0, False
            for f in range(len(self.frames)):
                if f:
                    if self.full(f - 1, j) and not self.full(f, j):
                        t["full_to_not_full"] = _first(t["full_to_not_full"], f)
                    if self.uniform(f - 1, j) and self.mixed(f, j):
                        t["uniform_to_mixed"] = _first(t["uniform_to_mixed"], f)
                    if self.mixed(f - 1, j) and self.uniform(f, j):
                        t["mixed_to_uniform"] = _first(t["mixed_to_uniform"], f)
                    if self.facts[f - 1][j][1] == 0 and self.full(f, j) and self.uniform(f, j):
                        t["empty_to_full"] = _first(t["empty_to_full"], f)
                if self.full(f, j) and self.mixed(f, j):
                    t["full_and_mixed"] = _first(t["full_and_mixed"], f)
                was_mixed = was_mixed or self.mixed(f, j)
                run = run + 1 if was_mixed and self.uniform(f, j) else 0
                best_run = max(best_run, run)
        for f, n in enumerate(self.alive_counts):
            if n == 0 and f and self.alive_counts[f - 1] > 0:
                t["all_dead"] = _first(t["all_dead"], f)
        e = t["empty_to_full"]   # ... and the first deaths of the burst that refilled the empty effect
        t["refilled_to_not_full"] = None if e is None else next((f for f in range(e + 1, len(self.frames)) if any(self.full(f - 1, j) and not self.full(f, j) for j in range(self.n_chunks()))), None)
        t["uniform_run"] = best_run
        return t

    def transition_frames(self):
        return sorted({f for k, f in self.transitions().items() if k != "uniform_run" and f is not None} | {0, len(self.frames) - 1})

    def flight_frame(self):
        """a frame of the first flight: every particle of the burst alive, none dead yet (None: the script has no burst)"""
        return next((f for f in range(3, len(self.frames) - 1) if self.alive_counts[f] == self.cap and self.alive_counts[f + 1] == self.cap), None)

    # -- comparison
    def oracle_state(self, f):
        orc = OracleRunner(self.asset, omp=self.cap >= 1 << 15)
        for fr in self.frames[: f + 1]:
            orc.step(fr)
        return orc.state()

    def assert_frame(self, f, got, what=""):
        """bit for bit against the oracle's state after frame f (NaN == NaN, as helpers.assert_same_state has it)"""
        if state_digest(got) != self.digests[f]:
            assert_same_state(self.oracle_state(f), got, f"{what} {self.name}@{self.cap} frame {f}")


def _first(a, b):
    return b if a is None else min(a, b)


@functools.lru_cache(maxsize=None)
def trace(name, cap):
    return Trace(name, cap)


# ---- fuzz frames that fill chunks ------------------------------------------------------------------------------------------------------------------
FUZZ_CAPS = (CHUNK, CHUNK + 1, 2 * CHUNK + 5)
# (chosen so that every seed lowers, and - asserted with the oracle alone - at least half hold a completely alive chunk at some frame)
FUZZ_FLOAT_SEEDS = (100, 101, 102, 103, 104, 105, 106, 107)
FUZZ_TYPED_SEEDS = (2100, 2101, 2102, 2103, 2104, 2105, 2106, 2107)
FUZZ_PROFILES = {"defaults": {}, "plain": PLAIN, "cohort_all": {"age_cohort": 2}, "no_transpose": {"transpose": 0}, "no_cull": {"cull_lifetime": 0}}


def fuzz_capacity(seed):
    return FUZZ_CAPS[seed % len(FUZZ_CAPS)]


def full_chunk_frames(seed, capacity, n=36):
    """fuzz_assets.random_frames (same generator, same draws), except that frame 0 bursts the whole capacity and frame n // 2 asks for 2 * capacity + 1"""
    rng = np.random.default_rng(seed + 977)
    xf = np.array([1, 0, 0, rng.uniform(-2, 2), 0, 1, 0, rng.uniform(-2, 2), 0, 0, 1, rng.uniform(-2, 2)], dtype=np.float32)
    out = []
    for f in range(n):
        drawn = 0 if f == 0 else (int(rng.integers(0, capacity // 3)) if rng.random() < 0.25 else 0)   # (random_frames' draws, in its order)
        spawn = capacity if f == 0 else (2 * capacity + 1 if f == n // 2 else drawn)
        out.append(Frame(1 / 60 if rng.random() < 0.8 else 1 / 30, spawn, frame_seed(seed * 131 + f), xf, time=f / 60))
    return out


def holds_a_full_chunk(asset, frames):
    """with the oracle alone: does some chunk hold 4096 alive particles after some frame?"""
    orc = OracleRunner(asset)
    for fr in frames:
        orc.step(fr)
        alive = orc.fx.alive_list().astype(np.int64)
        if len(alive) >= CHUNK and np.bincount(alive // CHUNK).max() == CHUNK:
            return True
    return False


# ---- hnb_program_kernel_info --------------------------------------------------------------------------------------------------------------------
_INFO = {
    "lists_skipped": r"^lists skipped: (\d+) of (\d+) frames",
    "horizon_frames": r"^death horizons in use: (\d+) frames",
    "cohort_chunks": r"^age cohorts: (\d+) of (\d+) chunks",
    "slot_init_frames": r"^slot-major init \(large spawns\): (\d+) frames",
    "merged_frames": r"^update served by a merged launch .*: (\d+) frames",
    "set_module_frames": r"^\.\.\. by the context's set module .*: (\d+) frames",
    "suffix_frames": r"^casualties proven to be the list's last rows \(no k_count_rows\): (\d+) frames",
    "ring_frames": r"^list kept as a ring \(no row rewritten\): (\d+) frames",
    "sort_skipped_frames": r"^ribbon sorts skipped in list-free frames: (\d+) frames",
    "sort_rotated_frames": r"^ribbon sorts by rotation: (\d+) of (\d+) frames",
    "direct_frames": r"^frame parameters \(context\): written by the host into device memory in (\d+) frames, copied in (\d+)",
}


def parse_kernel_info(text):
    """{counter: int} for every counter line of hnb_program_kernel_info; a line that is not printed (the library omits most zero counters) reads 0.
    Also "frames_run" (from the lists line), "cohort_total", "copied_frames" (the context's frames whose parameter block was copied, beside
    "direct_frames"), and the flags "lists_eligible", "cohort_auto_off", "cohort_plane_current", "large_bar"."""
    out = {k: 0 for k in _INFO}
    out.update(frames_run=0, cohort_total=0, copied_frames=0, lists_eligible=False, cohort_auto_off=False, cohort_plane_current=False, large_bar=True)
    for line in text.split("\n"):
        for key, pat in _INFO.items():
            m = re.match(pat, line)
            if not m:
                continue
            out[key] = int(m.group(1))
            if key == "lists_skipped":
                out["frames_run"] = int(m.group(2))
                out["lists_eligible"] = "(not eligible)" not in line
            elif key == "direct_frames":
                out["copied_frames"] = int(m.group(2))
                out["large_bar"] = "no large BAR" not in line and "failed their check" not in line
            elif key == "cohort_chunks":
                out["cohort_total"] = int(m.group(2))
                out["cohort_plane_current"] = "the update keeps the plane current" in line
        if line.startswith("age cohorts: off (HNB_AGE_COHORT_AUTO"):
            out["cohort_auto_off"] = True
    return out
