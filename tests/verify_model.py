"""What hnb_effect_check and hnb_effect_compare report (include/hanabi_amd.h "Verification on the device"), restated in numpy, and the tools that
read an effect's raw state from the device and plant single wrong words into it.

model_check / model_compare are the header's rules over plain arrays: tests/test_verify_model.py pins them on hand-made arrays without a GPU,
tests/test_gpu_verification_faults.py holds the kernels against them.

The raw state is read through Effect.device_view() and hipMemcpy: both list columns and the dead column in full, the HnbDeviceMeta row and the
planes - no call of the library interprets it on the way, so a corrupted state is read as it stands. The alive bytes are not part of the view:
a test derives them from the lists of the healthy state (hnb_effect_check has just said that they agree).

Planting is a hipMemcpy of single words to those same addresses, after Context.synchronize(); `planted` restores them on exit. Whoever plants
keeps to the rules in the docstring of tests/test_gpu_verification_faults.py."""
import contextlib
import ctypes as C

import numpy as np

U32 = np.uint32
META_WORDS = ("alive_count", "particle_counter", "list_column", "max_update", "dead_count", "spawned", "indirect_write_index", "instance_count")   # HnbDeviceMeta
LIST_COLUMN = META_WORDS.index("list_column")             # the word hnb_effect_compare leaves out: where the rows live is not what they are
WRITE_INDEX = META_WORDS.index("indirect_write_index")    # compared by its bit 0
COMPARED_WORDS = tuple(i for i in range(8) if i != LIST_COLUMN)
SECTION_ALIVE, SECTION_DEAD, SECTION_ATTR0 = 0, 1, 2


# ---- the rules ----------------------------------------------------------------------------------------------------------------------------------------
def model_check(alive_col, head, dead_col, alive_count, flags, age, life, reaps):
    """HnbEffectCheck's four counts. alive_col: the list column that holds the alive list, dead_col: the dead column, both of `capacity` words;
    flags: the alive byte per slot; age, life: the planes as float32 per slot (None where the layout has none); reaps: the program reaps by
    lifetime. Row r < alive_count names alive_col[(head + r) % capacity], every other row names dead_col[r]."""
    alive_col, dead_col = np.asarray(alive_col, U32), np.asarray(dead_col, U32)
    cap = len(dead_col)
    assert len(alive_col) == cap and 0 <= alive_count <= cap and 0 <= head < max(cap, 1)
    rows = np.arange(cap, dtype=np.int64)
    is_alive = rows < alive_count
    slot = np.where(is_alive, alive_col[(head + rows) % cap], dead_col).astype(np.int64)
    in_range = slot < cap
    s, a = slot[in_range], is_alive[in_range]
    out = {"bad_slots": int((~in_range).sum()),
           "duplicate_slots": int(len(s) - len(np.unique(s))),               # rows that name a slot an earlier-counted row already named
           "alive_byte_mismatches": int(((np.asarray(flags)[s] == 1) != a).sum()),
           "alive_past_lifetime": 0}
    if reaps and age is not None and life is not None:
        with np.errstate(invalid="ignore"):
            young = np.asarray(age, np.float32)[s] < np.asarray(life, np.float32)[s]
        out["alive_past_lifetime"] = int((a & ~young).sum())                  # !(age < lifetime): a NaN on either side counts
    return out


def _first_diff(x, y):
    d = np.flatnonzero(np.asarray(x, U32) != np.asarray(y, U32))
    return len(d), (int(d[0]) if len(d) else None)


def model_compare(a, b):
    """HnbEffectDiff of two raw states of one layout. A state is a dict: "meta" (the eight words of HnbDeviceMeta), "alive_col" (the column
    list_column & 1 names) and "dead_col" (`capacity` words each), "planes" (a list of (attribute id, the plane's words) in layout order)."""
    ma, mb = [int(x) for x in a["meta"]], [int(x) for x in b["meta"]]
    cap = len(a["dead_col"])
    assert len(b["dead_col"]) == cap and [p[0] for p in a["planes"]] == [p[0] for p in b["planes"]]
    na, nb = ma[0], mb[0]
    counters = 0
    for i in COMPARED_WORDS:
        x, y = (ma[i] & 1, mb[i] & 1) if i == WRITE_INDEX else (ma[i], mb[i])
        counters += int(x != y or (i == 0 and (na > cap or nb > cap)))       # an alive_count above the capacity is a difference, even the same on both sides
    sections = []                                                            # (section id, differing words, first index)
    if na == nb and na <= cap:                                               # else the rows do not correspond
        rows = np.arange(na, dtype=np.int64)
        ha, hb = ma[LIST_COLUMN] >> 1, mb[LIST_COLUMN] >> 1
        sections.append((SECTION_ALIVE,) + _first_diff(np.asarray(a["alive_col"])[(ha + rows) % cap], np.asarray(b["alive_col"])[(hb + rows) % cap]))
        sections.append((SECTION_DEAD,) + _first_diff(np.asarray(a["dead_col"])[na:], np.asarray(b["dead_col"])[na:]))   # index 0 is row alive_count
    else:
        sections += [(SECTION_ALIVE, 0, None), (SECTION_DEAD, 0, None)]
    for (attr, pa), (_, pb) in zip(a["planes"], b["planes"]):
        assert len(pa) == len(pb) and len(pa) % cap == 0
        sections.append((SECTION_ATTR0 + int(attr),) + _first_diff(pa, pb))
    out = {"counter_diffs": counters, "alive_list_diffs": sections[0][1], "dead_list_diffs": sections[1][1], "attr_diffs": sum(s[1] for s in sections[2:]),
           "first_section": -1, "first_index": 0}
    for sec, n, first in sections:
        if n:
            out["first_section"], out["first_index"] = sec, first
            break
    out["equal"] = int(counters == 0 and all(s[1] == 0 for s in sections))
    return out


# ---- the raw state ------------------------------------------------------------------------------------------------------------------------------------
_HIP = None
H2D, D2H = 1, 2


def _hip():
    global _HIP
    if _HIP is None:
        _HIP = C.CDLL("libamdhip64.so")
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.hipDeviceSynchronize.argtypes = []
    return _HIP


def read_words(addr, n):
    """n 32-bit words at the device address addr"""
    out = np.zeros(max(int(n), 1), U32)
    if n:
        assert _hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(int(addr)), int(n) * 4, D2H) == 0
    return out[:n]


def write_words(addr, words):
    w = np.ascontiguousarray(words, U32)
    assert _hip().hipMemcpy(C.c_void_p(int(addr)), C.c_void_p(w.ctypes.data), w.nbytes, H2D) == 0
    assert _hip().hipDeviceSynchronize() == 0


def meta_addr(fx, word):
    """device address of word `word` (an index or a name of META_WORDS) of the effect's HnbDeviceMeta row. The row moves from frame to frame."""
    word = META_WORDS.index(word) if isinstance(word, str) else int(word)
    assert 0 <= word < len(META_WORDS)
    return int(fx.device_view().meta) + 4 * word


def column_addr(fx, column, index):
    """device address of PHYSICAL index `index` of list column `column`"""
    v = fx.device_view()
    assert 0 <= index < v.capacity
    return int(v.alive_list[column]) + 4 * int(index)


def dead_addr(fx, row):
    v = fx.device_view()
    assert 0 <= row < v.capacity
    return int(v.dead_list) + 4 * int(row)


def plane_addr(fx, attr, word):
    """device address of word `word` (slot * ncomp + component) of the attribute's plane"""
    v = fx.device_view()
    p = v.plane(int(attr))
    assert 0 <= word < v.capacity * p.ncomp
    return int(p.plane) + 4 * int(word)


def read_state(ctx, fx, planes=True):
    """The effect's raw state after everything enqueued so far, in model_compare's form, plus "columns" (both list columns), "head" and "alive_count".
    planes: True (every plane), False (none) or a list of attribute ids."""
    ctx.synchronize()
    v = fx.device_view()
    cap = v.capacity
    meta = read_words(v.meta, 8)
    cols = [read_words(v.alive_list[c], cap) for c in (0, 1)]
    want = range(v.n_attrs) if planes is True else [i for i in range(v.n_attrs) if planes and v.attrs[i].attr in [int(a) for a in planes]]
    return {"meta": meta, "columns": cols, "alive_col": cols[int(meta[LIST_COLUMN]) & 1], "dead_col": read_words(v.dead_list, cap),
            "head": int(meta[LIST_COLUMN]) >> 1, "alive_count": int(meta[0]), "capacity": cap,
            "planes": [(int(v.attrs[i].attr), read_words(v.attrs[i].plane, cap * v.attrs[i].ncomp)) for i in want]}


def plane_of(state, attr):
    return next(p for a, p in state["planes"] if a == int(attr))


def alive_row_addr(fx, state, row):
    """device address of LOGICAL row `row` of the alive list: behind the head, round the column's end"""
    return column_addr(fx, int(state["meta"][LIST_COLUMN]) & 1, (state["head"] + int(row)) % state["capacity"])


def healthy_flags(state):
    """the alive byte per slot, from the lists of a state hnb_effect_check has found consistent"""
    cap, n = state["capacity"], state["alive_count"]
    flags = np.zeros(cap, np.uint8)
    flags[state["alive_col"][(state["head"] + np.arange(n, dtype=np.int64)) % cap]] = 1
    return flags


@contextlib.contextmanager
def planted(ctx, words):
    """words: (device address, 32-bit value) pairs, written in order after ctx.synchronize() (ctx: one context or several); the words they
    replaced come back on exit, in reverse order, also when the body raises."""
    for c in ctx if isinstance(ctx, (tuple, list)) else (ctx,):
        c.synchronize()
    old = []
    try:
        for addr, value in words:
            old.append((addr, int(read_words(addr, 1)[0])))
            write_words(addr, [int(value) & 0xFFFFFFFF])
        yield
    finally:
        for addr, value in reversed(old):
            write_words(addr, [value])
