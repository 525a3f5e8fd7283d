"""Program validation, the slab layout and the creation-time proofs (csrc/hnb_program.h) as pure host code.

The header decides from the bytes of a blob alone whether it is safe to run, where an instance's sections lie, and which shortcuts the
frame code may take for the program's whole life (a wrong `true` in RibbonFacts::provable / front_static / SkipFacts::eligible gives a wrong
order or a stale list silently). Here it is built with g++ alone under the address and undefined-behaviour sanitizers
(tests/program_facts/driver.cpp: nothing is loaded into Python under a sanitizer) and held against
  - the verdicts the library gave before the code moved (tests/golden/validator_verdicts.json), and the library's own verdicts now,
  - restatements of the layout and of every rule in Python, over the assets of the package and over the smallest blobs that break each
    premise of each fact, one at a time.
"""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess
import sys

import pytest

import bevy_hanabi_amd as bh
from bevy_hanabi_amd import effects, reference_examples as rx, runtime
from fuzz_assets import random_asset, random_typed_asset
from helpers import _cvm_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bevy_hanabi_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_program_goldens as gold  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("program_facts") / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "program_facts", "driver.cpp"), "-o", out])
    return out


def _run(driver, args, stdin=None):
    r = subprocess.run([driver] + args, input=stdin, capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, f"driver exit {r.returncode}\n" + "\n".join(r.stderr.splitlines()[-25:])
    return r.stdout.splitlines()


# ---- the blob, in Python ----------------------------------------------------------------------------------------------------
def _enum(name):
    text = open(os.path.join(ROOT, "include", "hanabi_amd.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text[text.index(f"typedef enum {name} {{"):text.index(f"}} {name};")].split("{", 1)[1], flags=re.S)
    out, nxt = {}, 0
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        if "=" in item:
            item, v = (s.strip() for s in item.split("="))
            nxt = int(v, 0)
        out[item] = nxt
        nxt += 1
    return out


OP = _enum("HnbOp")
(W_CAPACITY, W_FLAGS, W_N_ATTRS, W_UNIFORM_LEN, W_INIT_LEN, W_UPDATE_LEN, W_INIT_REGS, W_UPDATE_REGS, W_ATTRS_OFF, W_INIT_OFF, W_UPDATE_OFF, W_N_CHANNELS,
 W_RENDER_LO) = (3, 4, 5, 8, 9, 10, 12, 13, 14, 17, 18, 19, 22)
REG_AGE, REG_LIFETIME, REG_NONE = 6, 7, 0xFF
ATTR_AGE, ATTR_LIFETIME, ATTR_RIBBON_ID = 4, 5, 38
HAS_RIBBONS, READS_PARENT = 2, 4
UPD_LOAD, UPD_STORE = 1, 2
COHORT_OFF, COHORT_LEAN, COHORT_ALL, COHORT_AUTO = 0, 1, 2, 3
U = 0x80
DEFAULTS = (COHORT_AUTO, True, True, False)   # age_cohort, cull_lifetime, horizon, list_order_slot
MACRO_FIRST = OP["HNB_OP_M_AGE_TICK"]
LEAN = {OP["HNB_OP_M_" + n] for n in ("AGE_TICK", "EULER", "VEL_SCALE", "VEL_ADD", "PIN_SET", "KILL_SPHERE", "KILL_AABB")}
NOT_A_REGISTER_WRITE = {OP["HNB_OP_STA"], OP["HNB_OP_ALIVE_SET"], OP["HNB_OP_ALIVE_AND"], OP["HNB_OP_KILL_IF"]}


class Blob:
    def __init__(self, blob):
        self.h = struct.unpack_from("<24I", blob)
        self.attrs = [dict(zip(("attr", "ncomp", "reg", "scalar_type", "upd", "reserved"), struct.unpack_from("<HBBBBH", blob, self.h[W_ATTRS_OFF] + 8 * i)))
                      for i in range(self.h[W_N_ATTRS])]
        self.init = [struct.unpack_from("<II", blob, self.h[W_INIT_OFF] + 8 * i) for i in range(self.h[W_INIT_LEN])]
        self.update = [struct.unpack_from("<II", blob, self.h[W_UPDATE_OFF] + 8 * i) for i in range(self.h[W_UPDATE_LEN])]


def _op(ins): return ins[0] & 0xFF
def _dst(ins): return (ins[0] >> 8) & 0xFF
def _width(ins): return ((ins[1] >> 8) & 3) + 1
def _a(ins): return (ins[0] >> 16) & 0xFF
def _operand_a(ins): return (0x100 | (_a(ins) & 0x7F) | (((ins[1] >> 13) & 1) << 7)) if _a(ins) & U else _a(ins)   # HNB_OPERAND_DECODE


def py_facts(blob, opt=DEFAULTS):
    """every rule of program::facts, restated"""
    age_cohort_mode, opt_cull, opt_horizon, list_order_slot = opt
    b = Blob(blob)
    h, f = b.h, {}
    f["has_ribbons"] = bool(h[W_FLAGS] & HAS_RIBBONS)
    f["slot_order"] = list_order_slot and not f["has_ribbons"]
    f["wide_file"] = max(h[W_INIT_REGS], h[W_UPDATE_REGS]) > 32
    # streamable: macro ops AGE_TICK .. KILL_AABB with every operand they read in the parameter block, no non-pinned attribute touched
    two = {OP["HNB_OP_M_" + n] for n in ("RADIAL_ACCEL", "TANGENT_ACCEL", "CONFORM_SPHERE", "KILL_SPHERE", "KILL_AABB")}
    streams = all(MACRO_FIRST <= _op(i) <= OP["HNB_OP_M_KILL_AABB"] and _a(i) & U and (_op(i) not in two or (i[0] >> 24) & U) and
                  (_op(i) != OP["HNB_OP_M_TANGENT_ACCEL"] or i[1] & U) for i in b.update)
    streams = streams and not any(a["upd"] and a["reg"] == REG_NONE for a in b.attrs)
    f["update_streams"] = streams
    f["slot_init_eligible"] = not (h[W_FLAGS] & (HAS_RIBBONS | READS_PARENT)) and not any(_op(i) in (OP["HNB_OP_LDPC"], OP["HNB_OP_LDPARENT"]) for i in b.init)
    # lifetime culling: the stream starts with the only AGE_TICK, which tests the lifetime; nothing else writes AGE or LIFETIME
    life = [a for a in b.attrs if a["reg"] == REG_LIFETIME]
    age = [a for a in b.attrs if a["reg"] == REG_AGE]
    cull = (streams and opt_cull and len(b.update) > 0 and _op(b.update[0]) == MACRO_FIRST and bool((b.update[0][1] >> 16) & 1) and
            not any(_op(i) == MACRO_FIRST or (_op(i) == OP["HNB_OP_M_PIN_SET"] and _dst(i) in (REG_AGE, REG_LIFETIME)) for i in b.update[1:]) and
            bool(life) and bool(life[-1]["upd"] & UPD_LOAD) and not life[-1]["upd"] & UPD_STORE and bool(age) and bool(age[-1]["upd"] & UPD_LOAD))
    f["cull_lifetime"] = cull
    f["cull_dt_operand"] = _operand_a(b.update[0]) if cull else 0
    reads_age = bool(h[W_RENDER_LO] >> ATTR_AGE & 1)
    f["lean"] = all(_op(i) in LEAN for i in b.update)
    cohort = cull and not f["has_ribbons"] and age_cohort_mode != COHORT_OFF
    if age_cohort_mode == COHORT_AUTO and reads_age and h[W_CAPACITY] < 65536:
        cohort = False
    if age_cohort_mode != COHORT_ALL:
        cohort = cohort and f["lean"]
    f["age_cohort"] = cohort
    f["auto_materialise"] = age_cohort_mode == COHORT_AUTO and cohort and reads_age
    f["stream_waves"] = min(6 if f["lean"] else 5, 4) if cohort else (6 if f["lean"] else 5)
    f["kills"] = any(_op(i) in (OP["HNB_OP_M_KILL_SPHERE"], OP["HNB_OP_M_KILL_AABB"]) for i in b.update)
    r = dict(provable=False, front_static=False, age_init_set=False, rid_set=False, tick_operand=0, age_init_operand=0, rid_operand=0, life_operand=0)
    if f["has_ribbons"] and streams:
        _py_ribbon(b, r)
    f.update(r)
    f["skip_eligible"] = streams and cull and not f["kills"] and h[W_N_CHANNELS] == 0 and not h[W_FLAGS] & READS_PARENT
    f["skip_dt_operand"] = f["cull_dt_operand"]
    f["horizon_eligible"] = streams and cull and not f["kills"] and not f["has_ribbons"] and not f["slot_order"] and opt_horizon
    return {k: int(v) for k, v in f.items()}


def _py_ribbon(b, r):
    """plan::RibbonFacts. The operands are those of the instructions seen until a premise failed, as the header records them."""
    ok, ticks = True, 0
    for i in b.update:
        if not ok:
            break
        if _op(i) == MACRO_FIRST:      # the update advances AGE through AGE_TICKs of a uniform tick ...
            ticks += 1
            r["tick_operand"] = _operand_a(i)
            ok = bool(r["tick_operand"] & 0x100)
        if _op(i) == OP["HNB_OP_M_PIN_SET"] and _dst(i) == REG_AGE:
            ok = False
    ok = ok and ticks == 1             # ... exactly one
    if any(a["attr"] == ATTR_RIBBON_ID and a["upd"] & UPD_STORE for a in b.attrs):
        ok = False

    def writes(i, reg):   # an instruction that is no macro op, no store and no alive-flag op, and whose destination span covers the register
        return _op(i) not in NOT_A_REGISTER_WRITE and _op(i) < MACRO_FIRST and _dst(i) <= reg < _dst(i) + _width(i)
    for i in b.init:
        if not ok:
            break
        if _op(i) == OP["HNB_OP_M_PIN_SET"] and _dst(i) == REG_AGE:   # the init sets AGE from a uniform value or not at all
            r["age_init_operand"], r["age_init_set"] = _operand_a(i), True
            ok = bool(r["age_init_operand"] & 0x100)
        elif writes(i, REG_AGE):
            ok = False
    r["provable"] = ok
    rid = [k for k, a in enumerate(b.attrs) if a["attr"] == ATTR_RIBBON_ID]
    front, rid_stores, life_sets = ok and bool(rid), 0, 0
    for i in b.init:                   # RIBBON_ID stored at most once by the init, from a uniform value
        if not front:
            break
        if _op(i) == OP["HNB_OP_STA"] and i[1] >> 16 == rid[-1]:
            rid_stores += 1
            r["rid_operand"] = _operand_a(i)
            front = bool(r["rid_operand"] & 0x100)
    r["rid_set"] = rid_stores == 1
    for i in b.init:                   # LIFETIME set exactly once, from a uniform value
        if not front:
            break
        if _op(i) == OP["HNB_OP_M_PIN_SET"] and _dst(i) == REG_LIFETIME:
            life_sets += 1
            r["life_operand"] = _operand_a(i)
            front = bool(r["life_operand"] & 0x100)
        elif writes(i, REG_LIFETIME):
            front = False
    killers = {OP["HNB_OP_M_KILL_SPHERE"], OP["HNB_OP_M_KILL_AABB"], OP["HNB_OP_KILL_IF"], OP["HNB_OP_ALIVE_SET"], OP["HNB_OP_ALIVE_AND"]}
    for i in b.update:                 # only old age kills
        if not front:
            break
        if _op(i) in killers or (_op(i) == OP["HNB_OP_M_PIN_SET"] and _dst(i) == REG_LIFETIME):
            front = False
    r["front_static"] = front and rid_stores <= 1 and life_sets == 1


def c_facts(driver, tmp_path, cases, mode="facts"):
    """program::facts (or, mode "ribbon", program::ribbon_facts alone) through the driver: cases = [(blob, options)] -> [dict]"""
    path = tmp_path / "facts.bin"
    with open(path, "wb") as f:
        for blob, opt in cases:
            f.write(struct.pack("<5I", len(blob), *[int(o) for o in opt]) + blob)
    out = []
    for line in _run(driver, [mode, str(path)]):
        assert not line.startswith("rejected"), line
        out.append({k: int(v) for k, v in (kv.split("=") for kv in line.split())})
    assert len(out) == len(cases)
    return out


def ribbon_alone(driver, tmp_path, blobs):
    """program::ribbon_facts called directly - facts() asks first whether the update streams, and some broken premises stop that too - against its
    restatement"""
    got = c_facts(driver, tmp_path, [(b, DEFAULTS) for b in blobs], mode="ribbon")
    for b, g in zip(blobs, got):
        bh.validate_program(b)
        want = dict(provable=False, front_static=False, age_init_set=False, rid_set=False, tick_operand=0, age_init_operand=0, rid_operand=0, life_operand=0)
        _py_ribbon(Blob(b), want)
        assert g == {k: int(v) for k, v in want.items()}
    return got


# ---- editing a blob ---------------------------------------------------------------------------------------------------------
def _set_word(blob, byte_off, value):
    b = bytearray(blob)
    struct.pack_into("<I", b, byte_off, value & 0xFFFFFFFF)
    return bytes(b)


def _set_header(blob, word, value): return _set_word(blob, 4 * word, value)


def _set_ins(blob, stream_word, i, x=None, y=None):
    off = struct.unpack_from("<24I", blob)[stream_word] + 8 * i
    if x is not None:
        blob = _set_word(blob, off, x)
    if y is not None:
        blob = _set_word(blob, off + 4, y)
    return blob


def _set_attr_flags(blob, attr_id, flags):
    B = Blob(blob)
    k = [i for i, a in enumerate(B.attrs) if a["attr"] == attr_id][0]
    b = bytearray(blob)
    b[B.h[W_ATTRS_OFF] + 8 * k + 5] = flags
    return bytes(b), B.attrs[k]["upd"]


def _find(stream, pred):
    return [k for k, i in enumerate(stream) if pred(i)][0]


# ---- 1. the verdicts the library gave before the validator moved -------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    from test_validator_fuzz import _bases
    bases = _bases()
    return bases, {seed: gold.corpus(seed, bases) for seed in gold.SEEDS}


@pytest.fixture(scope="module")
def library_verdicts(corpus):
    bases, mutants = corpus
    return [gold.verdict(b) for b in bases], {seed: [gold.verdict(m) for m in mutants[seed]] for seed in mutants}


def test_validator_verdicts_are_the_recorded_ones(library_verdicts):
    want = json.load(open(gold.VERDICTS_PATH))
    of_bases, of_mutants = library_verdicts
    got = {"bases": gold.summarise(of_bases), **{f"seed{seed}": gold.summarise(v) for seed, v in of_mutants.items()}}
    for key in want:
        assert (got[key]["accepted"], got[key]["rejected"]) == (want[key]["accepted"], want[key]["rejected"]), key
        assert got[key]["messages"] == want[key]["messages"], key     # (a difference here names the rule)
        assert got[key]["sha256"] == want[key]["sha256"], key
    assert set(got) == set(want)


# ---- 5. the validator under the sanitizers, on everything ---------------------------------------------------------------------------
def test_validator_reads_nothing_outside_any_blob_and_the_library_runs_the_header(driver, tmp_path, corpus, library_verdicts):
    bases, mutants = corpus
    of_bases, of_mutants = library_verdicts
    blobs = list(bases) + [m for seed in gold.SEEDS for m in mutants[seed]]
    want = list(of_bases) + [v for seed in gold.SEEDS for v in of_mutants[seed]]
    n_corpus = len(blobs)
    prefixes = [b[:n] for b in bases for n in range(len(b))]                                   # every proper prefix ...
    resized = [_set_header(b[:n], 2, n) for b in bases for n in range(24 * 4, len(b))]         # ... and with total_size rewritten to its length
    blobs += prefixes + resized
    path = tmp_path / "blobs.bin"
    with open(path, "wb") as f:
        for b in blobs:
            f.write(struct.pack("<I", len(b)) + b)
    lines = _run(driver, ["validate", str(path)])
    assert len(lines) == len(blobs)
    got = [(int(l.split("\t", 1)[0]), l.split("\t", 1)[1]) for l in lines]
    assert got[:n_corpus] == want                                        # byte for byte what the library says: it runs this header
    of_prefixes = got[n_corpus:n_corpus + len(prefixes)]
    assert all(rc == -2 for rc, _ in of_prefixes)                        # total_size and the minimum size: no exception
    assert {t for _, t in of_prefixes} <= {"program blob too small"} | {t for _, t in of_prefixes if t.startswith("program size mismatch (")}
    lib = runtime.load_library()
    assert got[n_corpus:] == [gold.verdict(b) for b in prefixes + resized]     # ... for every one of these as well
    # the later bounds checks catch what total_size no longer does: a truncated blob with a consistent size is rejected unless nothing was cut
    of_resized = got[n_corpus + len(prefixes):]
    assert all(rc == -2 for rc, _ in of_resized), [t for rc, t in of_resized if rc == 0][:3]
    assert lib.hnb_program_validate(None, 0) == -2 and lib.hnb_last_error() == b"program blob too small"


def test_a_long_message_is_cut_at_511_characters_as_before(driver):
    """no validator message is that long today; what vsnprintf into buf[512] did to one that were, program::reject does"""
    for n in (0, 510, 511, 512, 2000):
        assert _run(driver, ["reject", str(n)]) == ["-2 -2 %d %s" % (min(n, 511), "x" * min(n, 511))]
    lib = runtime.load_library()
    lib.hnb_ctx_set_option.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    assert lib.hnb_ctx_set_option(None, 0, 0) != 0      # (any failing entry point: the thread's message is replaced)
    blob = bh.lower(effects.single_particle(16))
    assert lib.hnb_program_validate(_set_header(blob, 0, 0x12345678), len(blob)) == -2 and lib.hnb_last_error() == b"bad program magic 0x12345678"
    src = open(os.path.join(CSRC, "hnb_program.h")).read()
    assert "char text[512]" in src and "vsnprintf(v.text, sizeof v.text, fmt, ap)" in src


# ---- 6. slab_layout --------------------------------------------------------------------------------------------------------
def _align(v): return (v + 255) // 256 * 256


def py_layout(cap, n_attrs, n_ch, ribbons):
    """program::slab_layout restated: [sections in order], total"""
    chunks, tiles, lst = -(-cap // 4096), -(-cap // 4096), _align(cap * 4)
    sizes = [lst, lst, lst] + [_align(cap * (1 + i % 4) * 4) for i in range(n_attrs)] + [_align(cap), _align(chunks * 16), _align(chunks * 512), _align(chunks * 512),
                                                                                        _align(256 + chunks * 24)] + [lst] * n_ch
    if ribbons:
        sizes += [_align(cap * 8)] * 2 + [lst] * 2 + [_align(256 * tiles * 4), _align(8 * -(-tiles // 32) * 256 * 4), 256]
    offs, off = [], 0
    for s in sizes:
        offs.append(off)
        off += s
    return chunks, tiles, offs, sizes, off


def test_slab_layout_sections_are_aligned_ordered_disjoint_and_bounded(driver):
    cases = [(cap, n_attrs, n_ch, rib) for cap in (1, 255, 256, 4095, 4096, 4097, 65536, 2 ** 31) for n_attrs in (1, 40) for n_ch in (0, 8) for rib in (0, 1)]
    # where the total passes 0xffffffff << 8: 40 attributes of 1..4 components at capacities around the limit
    limit = 0xFFFFFFFF << 8
    lo, hi = 1, 2 ** 32 - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if py_layout(mid, 40, 8, 1)[4] <= limit else (lo, mid)
    assert py_layout(lo, 40, 8, 1)[4] <= limit < py_layout(hi, 40, 8, 1)[4]
    cases += [(lo, 40, 8, 1), (hi, 40, 8, 1), (2 ** 32 - 1, 40, 8, 1), (2 ** 32 - 1, 1, 0, 0)]
    lines = _run(driver, ["layout"], stdin="".join("%d %d %d %d\n" % c for c in cases))
    assert len(lines) == len(cases)
    fits_seen = set()
    for (cap, n_attrs, n_ch, rib), line in zip(cases, lines):
        w = [int(x) for x in line.split()]
        chunks, tiles, ribbons, total, fits, offs = w[0], w[1], w[2], w[3], w[4], w[5:]
        want_chunks, want_tiles, want_offs, sizes, want_total = py_layout(cap, n_attrs, n_ch, rib)
        assert (chunks, tiles, ribbons, total) == (want_chunks, want_tiles, rib, want_total) and offs == want_offs, (cap, n_attrs, n_ch, rib)
        assert len(offs) == 3 + n_attrs + 5 + n_ch + (7 if rib else 0)
        assert all(o % 256 == 0 for o in offs) and total % 256 == 0
        assert all(offs[k] + sizes[k] <= offs[k + 1] for k in range(len(offs) - 1)) and offs[-1] + sizes[-1] <= total and offs[0] == 0   # the documented order, nothing overlaps
        assert fits == (total <= limit), (cap, total)
        fits_seen.add(fits)
    assert fits_seen == {0, 1}
    assert [int(l.split()[4]) for l in lines[-4:-2]] == [1, 0]            # it flips exactly there


# ---- 7. facts, premise by premise -------------------------------------------------------------------------------------------
def _asset_corpus():
    assets = [effects.single_particle(16), effects.firework_trails(64), effects.force_field(64), effects.instancing(64), effects.ribbon(64, rate=10.0),
              effects.firework_rocket(), effects.firework_sparkle_trail(), effects.firework_trails_child()]
    assets += [e.asset for entries in rx.catalog().values() for e in entries]
    assets += [random_asset(s, 64) for s in range(6)] + [random_typed_asset(2000 + s, 64) for s in range(10)]
    return [bh.lower(a) for a in assets]


def test_facts_of_every_asset_follow_the_restated_rules_and_the_cpu_vm_streams_the_same_updates(driver, tmp_path):
    blobs = _asset_corpus()
    options = [DEFAULTS, (COHORT_OFF, True, True, False), (COHORT_LEAN, True, False, True), (COHORT_ALL, False, True, False), (COHORT_ALL, True, True, True)]
    cases = [(b, o) for b in blobs for o in options]
    got = c_facts(driver, tmp_path, cases)
    for (b, o), g in zip(cases, got):
        assert g == py_facts(b, o), o
    assert len({tuple(sorted(g.items())) for g in got}) > 12            # the corpus tells the kinds apart
    cvm = _cvm_lib()
    for b, g in zip(blobs, got[::len(options)]):                          # tests/cpu_vm/cpu_vm.cpp keeps a copy of the streamable rule: pinned to the header's
        v = cvm.cvm_create(b, len(b), 0)
        assert v and bool(cvm.cvm_streamable(v)) == bool(g["update_streams"])
        cvm.cvm_destroy(v)


def _check(driver, tmp_path, cases):
    """every (blob, options) agrees with the restatement; returns the facts"""
    got = c_facts(driver, tmp_path, cases)
    for (b, o), g in zip(cases, got):
        bh.validate_program(b)
        assert g == py_facts(b, o)
    return got


def test_cull_lifetime_breaks_with_each_premise(driver, tmp_path):
    base = bh.lower(effects.firework_trails(64))       # update: AGE_TICK, VEL_SCALE, VEL_ADD, EULER
    B = Blob(base)
    assert [_op(i) for i in B.update] == [OP["HNB_OP_M_" + n] for n in ("AGE_TICK", "VEL_SCALE", "VEL_ADD", "EULER")]
    x0, y0 = B.update[0]
    x1, y1 = B.update[1]
    pin = lambda reg: (x1 & 0xFFFF0000) | (reg << 8) | OP["HNB_OP_M_PIN_SET"]
    broken = {
        "a second AGE_TICK": _set_ins(base, W_UPDATE_OFF, 1, x=(x1 & ~0xFF) | MACRO_FIRST),
        "the AGE_TICK not at position 0": _set_ins(_set_ins(base, W_UPDATE_OFF, 0, x1, y1), W_UPDATE_OFF, 1, x0, y0),   # (the first two instructions swapped)
        "an AGE_TICK that does not test the lifetime": _set_ins(base, W_UPDATE_OFF, 0, y=y0 & ~(1 << 16)),
        "M_PIN_SET of AGE in the update": _set_ins(base, W_UPDATE_OFF, 1, x=pin(REG_AGE)),
        "M_PIN_SET of LIFETIME in the update": _set_ins(base, W_UPDATE_OFF, 1, x=pin(REG_LIFETIME)),
        "LIFETIME stored by the update": _set_attr_flags(base, ATTR_LIFETIME, UPD_LOAD | UPD_STORE)[0],
    }
    got = _check(driver, tmp_path, [(base, DEFAULTS)] + [(b, DEFAULTS) for b in broken.values()] + [(base, (COHORT_AUTO, False, True, False))])
    assert got[0]["cull_lifetime"] == 1 and got[0]["skip_eligible"] == 1 and got[0]["horizon_eligible"] == 1 and got[0]["cull_dt_operand"] == got[0]["skip_dt_operand"] >= 0x100
    for name, g in zip(list(broken) + ["HNB_OPT_CULL_LIFETIME off"], got[1:]):
        assert g["update_streams"] == 1, name                             # the premise alone fails
        assert (g["cull_lifetime"], g["age_cohort"], g["skip_eligible"], g["horizon_eligible"], g["cull_dt_operand"]) == (0, 0, 0, 0, 0), name


def test_ribbon_provable_breaks_with_each_premise(driver, tmp_path):
    base = bh.lower(effects.ribbon(64, rate=10.0))     # update: AGE_TICK alone; the init sets AGE, LIFETIME, RIBBON_ID from literals
    rnd = bh.lower(gold._ribbon_random_lifetime(64))   # ... and one whose init draws the LIFETIME: a non-macro instruction to redirect
    B, R = Blob(base), Blob(rnd)
    assert [_op(i) for i in B.update] == [MACRO_FIRST]
    k_age = _find(B.init, lambda i: _op(i) == OP["HNB_OP_M_PIN_SET"] and _dst(i) == REG_AGE)
    k_draw = _find(R.init, lambda i: _op(i) < MACRO_FIRST and _op(i) not in NOT_A_REGISTER_WRITE and _width(i) == 1)
    v_operand = lambda x: (x & 0xFF00FFFF) | (REG_LIFETIME << 16)        # operand a = V register 7 instead of a parameter word
    broken = {
        "an AGE_TICK from a V operand": _set_ins(base, W_UPDATE_OFF, 0, x=v_operand(B.update[0][0])),
        "M_PIN_SET AGE from a V operand in the init": _set_ins(base, W_INIT_OFF, k_age, x=v_operand(B.init[k_age][0])),
        "RIBBON_ID stored by the update": _set_attr_flags(base, ATTR_RIBBON_ID, UPD_STORE)[0],
    }
    on_age = _set_ins(rnd, W_INIT_OFF, k_draw, x=(R.init[k_draw][0] & 0xFFFF00FF) | (REG_AGE << 8))   # a non-macro instruction whose destination is the AGE register
    got = _check(driver, tmp_path, [(base, DEFAULTS), (rnd, DEFAULTS), (on_age, DEFAULTS)] + [(b, DEFAULTS) for b in broken.values()])
    assert (got[0]["provable"], got[0]["front_static"], got[0]["age_init_set"], got[0]["rid_set"]) == (1, 1, 1, 1)
    assert got[0]["tick_operand"] >= 0x100 and got[0]["rid_operand"] >= 0x100 and got[0]["life_operand"] >= 0x100 and got[0]["age_init_operand"] >= 0x100
    assert (got[1]["provable"], got[1]["front_static"]) == (1, 0)        # a per-particle LIFETIME: the head stays sorted, the front is not static
    assert got[2]["update_streams"] == 1 and (got[2]["provable"], got[2]["front_static"]) == (0, 0)
    for name, g in zip(broken, got[3:]):
        assert (g["provable"], g["front_static"]) == (0, 0), name
    assert got[4]["update_streams"] == 1 and got[4]["age_init_operand"] == REG_LIFETIME
    # the other two also stop the update from streaming, which facts() asks first: ribbon_facts itself refuses them as well
    assert got[3]["update_streams"] == 0 and got[5]["update_streams"] == 0
    alone = ribbon_alone(driver, tmp_path, [base] + list(broken.values()))
    assert [g["provable"] for g in alone] == [1, 0, 0, 0] and alone[1]["tick_operand"] == REG_LIFETIME
    # the span part of "covers the AGE register": the draw widened to two registers from the one below AGE
    spans = _set_ins(rnd, W_INIT_OFF, k_draw, x=(R.init[k_draw][0] & 0xFFFF00FF) | ((REG_AGE - 1) << 8), y=(R.init[k_draw][1] & ~0x300) | (1 << 8))
    below = _set_ins(rnd, W_INIT_OFF, k_draw, x=(R.init[k_draw][0] & 0xFFFF00FF) | ((REG_AGE - 1) << 8))      # ... and one register wide there: AGE is not touched
    got = _check(driver, tmp_path, [(spans, DEFAULTS), (below, DEFAULTS)])
    assert [(g["update_streams"], g["provable"]) for g in got] == [(1, 0), (1, 1)]


def test_ribbon_front_static_breaks_with_each_premise(driver, tmp_path):
    base = bh.lower(effects.ribbon(64, rate=10.0))
    B = Blob(base)
    rid = _find(B.attrs, lambda a: a["attr"] == ATTR_RIBBON_ID)
    k_sta = _find(B.init, lambda i: _op(i) == OP["HNB_OP_STA"] and i[1] >> 16 != rid and B.attrs[i[1] >> 16]["ncomp"] == 1)      # the store of SIZE
    k_pos = _find(B.init, lambda i: _op(i) == OP["HNB_OP_M_PIN_SET"] and _dst(i) == 0)
    k_life = _find(B.init, lambda i: _op(i) == OP["HNB_OP_M_PIN_SET"] and _dst(i) == REG_LIFETIME)
    redirect = lambda k, reg: _set_ins(base, W_INIT_OFF, k, x=(B.init[k][0] & 0xFFFF00FF) | (reg << 8), y=B.init[k][1] & ~0x300)   # (one instruction: destination and width 1)
    broken = {
        "two RIBBON_ID stores": _set_ins(base, W_INIT_OFF, k_sta, y=(B.init[k_sta][1] & 0xFFFF) | (rid << 16)),
        "LIFETIME set twice": redirect(k_pos, REG_LIFETIME),
        "LIFETIME never set": redirect(k_life, REG_AGE),
    }
    # ... and a kill / alive opcode in the update: the ribbon with the default motion integration has an EULER to replace
    w = bh.ExprWriter()
    mods = [bh.SetAttributeModifier(bh.Attribute.POSITION, w.lit((0.0, 0.0, 0.0)).expr()), bh.SetAttributeModifier(bh.Attribute.VELOCITY, w.lit((0.0, 1.0, 0.0)).expr()),
            bh.SetAttributeModifier(bh.Attribute.AGE, w.lit(0.0).expr()),
            bh.SetAttributeModifier(bh.Attribute.LIFETIME, w.lit(1.5).expr()), bh.SetAttributeModifier(bh.Attribute.RIBBON_ID, w.lit(bh.Value.u32(0)).expr())]
    asset = bh.EffectAsset(64, bh.SpawnerSettings.rate(10.0), w.finish()).with_name("moving_ribbon")
    for m in mods:
        asset = asset.init(m)
    moving = bh.lower(asset)
    M = Blob(moving)
    assert [_op(i) for i in M.update] == [MACRO_FIRST, OP["HNB_OP_M_EULER"]] and M.h[11] >= 3
    killers = {}
    for name in ("HNB_OP_M_KILL_SPHERE", "HNB_OP_M_KILL_AABB", "HNB_OP_KILL_IF", "HNB_OP_ALIVE_SET", "HNB_OP_ALIVE_AND"):
        killers[name] = _set_ins(moving, W_UPDATE_OFF, 1, x=OP[name] | (U << 16) | (U << 24), y=0)    # operands: parameter word 0
    got = _check(driver, tmp_path, [(base, DEFAULTS), (moving, DEFAULTS)] + [(b, DEFAULTS) for b in list(broken.values()) + list(killers.values())])
    assert got[0]["front_static"] == got[1]["front_static"] == 1 and got[1]["provable"] == 1
    for name, g in zip(list(broken) + list(killers), got[2:]):
        assert g["front_static"] == 0, name
    for name, g in zip(broken, got[2:]):
        assert g["provable"] == 1 and g["update_streams"] == 1, name      # the premise alone fails
    alone = ribbon_alone(driver, tmp_path, list(killers.values()))            # (ribbon_facts itself, for the three that facts() never hands to it)
    assert [(g["provable"], g["front_static"]) for g in alone] == [(1, 0)] * 5
    for name, g in zip(killers, got[2 + len(broken):]):
        assert g["update_streams"] == (1 if "_M_" in name else 0) and g["provable"] == g["update_streams"], name   # (KILL_IF / ALIVE_* are no streaming ops at all)


def test_slot_init_eligible_breaks_with_each_premise(driver, tmp_path):
    base = bh.lower(effects.firework_trails(64))
    B = Blob(base)
    k = _find(B.init, lambda i: _op(i) == OP["HNB_OP_FRAND"])
    ldpc = _set_ins(base, W_INIT_OFF, k, x=(B.init[k][0] & ~0xFF) | OP["HNB_OP_LDPC"])
    # LDPARENT in the init: validate_blob accepts it only with a listed parent attribute, and so only with the parent flag - that premise cannot
    # be broken alone. The flag without any LDPARENT can: every LDPARENT of the child overwritten with an FRAND of the same destination and width.
    child = bh.lower(effects.firework_trails_child())
    C_ = Blob(child)
    assert any(_op(i) == OP["HNB_OP_LDPARENT"] for i in C_.init) and C_.h[W_FLAGS] & READS_PARENT
    flag_alone = child
    for k, i in enumerate(C_.init):
        if _op(i) == OP["HNB_OP_LDPARENT"]:
            flag_alone = _set_ins(flag_alone, W_INIT_OFF, k, x=(i[0] & ~0xFF) | OP["HNB_OP_FRAND"])
    F = Blob(flag_alone)
    assert F.h[W_FLAGS] & READS_PARENT and not any(_op(i) in (OP["HNB_OP_LDPC"], OP["HNB_OP_LDPARENT"]) for i in F.init)
    ribbon = bh.lower(effects.ribbon(64, rate=10.0))
    got = _check(driver, tmp_path, [(base, DEFAULTS), (ldpc, DEFAULTS), (child, DEFAULTS), (flag_alone, DEFAULTS), (ribbon, DEFAULTS)])
    assert [g["slot_init_eligible"] for g in got] == [1, 0, 0, 0, 0]
    assert not any(_op(i) in (OP["HNB_OP_LDPC"], OP["HNB_OP_LDPARENT"]) for i in Blob(ribbon).init)   # the flag alone


def test_age_cohorts_at_the_auto_threshold_under_every_mode(driver, tmp_path):
    base = bh.lower(gold._stream_asset(64, True))
    assert Blob(base).h[W_RENDER_LO] >> ATTR_AGE & 1
    cases, want = [], []
    for cap in (65535, 65536):
        for reads in (0, 1):
            b = _set_header(_set_header(base, W_CAPACITY, cap), W_RENDER_LO, (Blob(base).h[W_RENDER_LO] & ~(1 << ATTR_AGE)) | (reads << ATTR_AGE))
            for mode in (COHORT_OFF, COHORT_LEAN, COHORT_ALL, COHORT_AUTO):
                cases.append((b, (mode, True, True, False)))
                cohort = mode in (COHORT_LEAN, COHORT_ALL) or (mode == COHORT_AUTO and not (reads and cap < 65536))
                want.append((int(cohort), int(cohort and mode == COHORT_AUTO and bool(reads)), 4 if cohort else 6))
    got = _check(driver, tmp_path, cases)
    assert [(g["age_cohort"], g["auto_materialise"], g["stream_waves"]) for g in got] == want
    assert all(g["cull_lifetime"] == 1 and g["lean"] == 1 for g in got)
    # a stack that is not lean keeps its plane under LEAN and AUTO, not under ALL
    ff = _set_header(bh.lower(effects.force_field(64)), W_CAPACITY, 65536)
    got = _check(driver, tmp_path, [(ff, (m, True, True, False)) for m in (COHORT_OFF, COHORT_LEAN, COHORT_ALL, COHORT_AUTO)])
    assert [(g["age_cohort"], g["stream_waves"], g["lean"], g["kills"]) for g in got] == [(0, 5, 0, 1), (0, 5, 0, 1), (1, 4, 0, 1), (0, 5, 0, 1)]


def test_horizon_eligible_needs_each_of_its_six_inputs(driver, tmp_path):
    base = bh.lower(effects.firework_trails(64))
    cases = {
        "all six": (base, DEFAULTS),
        "update_streams": (bh.lower(gold._generic_asset(64)), DEFAULTS),
        "cull_lifetime": (base, (COHORT_AUTO, False, True, False)),
        "no kill modifier": (bh.lower(effects.force_field(64)), DEFAULTS),
        "no ribbons": (bh.lower(effects.ribbon(64, rate=10.0)), DEFAULTS),
        "not slot order": (base, (COHORT_AUTO, True, True, True)),
        "HNB_OPT_HORIZON": (base, (COHORT_AUTO, True, False, False)),
    }
    got = dict(zip(cases, _check(driver, tmp_path, list(cases.values()))))
    assert [g["horizon_eligible"] for g in got.values()] == [1, 0, 0, 0, 0, 0, 0]
    assert got["update_streams"]["update_streams"] == 0 and got["cull_lifetime"]["cull_lifetime"] == 0 and got["no kill modifier"]["kills"] == 1
    assert got["no ribbons"]["has_ribbons"] == 1 and got["no ribbons"]["slot_order"] == 0 and got["not slot order"]["slot_order"] == 1
    for name in ("no kill modifier", "no ribbons", "not slot order", "HNB_OPT_HORIZON"):       # nothing else is missing in these
        assert got[name]["update_streams"] == 1 and got[name]["cull_lifetime"] == 1, name
    assert got["no kill modifier"]["skip_eligible"] == 0 and got["not slot order"]["skip_eligible"] == 1


# ---- 8. where the code lives ------------------------------------------------------------------------------------------------
def test_the_header_is_plain_cpp_and_the_runtime_keeps_no_second_copy():
    hdr = open(os.path.join(CSRC, "hnb_program.h")).read()
    assert "hip" not in hdr and "__global__" not in hdr and "__device__" not in hdr and "g_last_error" not in hdr
    assert set(re.findall(r'#include\s+([<"][^>"]+[>"])', hdr)) == {"<algorithm>", "<cstdarg>", "<cstdint>", "<cstdio>", "<cstring>", '"hnb_dev.h"', '"hnb_plan.h"'}
    assert "reinterpret_cast" not in hdr                 # every word of the blob is read with memcpy
    src = open(os.path.join(CSRC, "hanabi_amd.hip")).read()
    body = src[src.index("int hnb_program_create("):]
    body = body[:body.index("ctx->programs.push_back")]
    assert "HNB_OP_" not in body and "parse_program(" in body and "= f." in body
    everything = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip")))
    for name in ("update_is_streamable", "cull_eligible", "validate_stream", "validate_blob", "slot_init_eligible", "age_cohort_eligible", "slab_layout"):
        assert len(re.findall(r"^inline [\w:<> ]+ " + name + r"\(", everything, flags=re.M)) == 1, name
        assert len(re.findall(r"^(?:static )?(?:bool|int) " + name + r"\(", everything, flags=re.M)) == 0, name
    for name in ("kSortTile", "kSortGroup", "kSceneMaxChunks", "kAutoMaterialiseMinSlots", "kAttrComponents"):
        assert len(re.findall(r"constexpr \w+ " + name + r"\b", everything)) == 1, name
