"""tests/verify_model.py pinned on hand-made arrays: one case per rule of HnbEffectCheck / HnbEffectDiff (include/hanabi_amd.h "Verification on
the device"). The GPU tests hold the kernels against this model, so the model itself is held against the header's words here."""
import numpy as np
import pytest

from verify_model import META_WORDS, model_check, model_compare

F32, U32 = np.float32, np.uint32
NAN = F32(np.nan)
ZERO = {"bad_slots": 0, "duplicate_slots": 0, "alive_byte_mismatches": 0, "alive_past_lifetime": 0}


def healthy(cap=8, n=5, head=0):
    """slots 7, 6, ... alive in rows 0 .. n - 1 (behind `head`), the others in the dead rows [n, cap); ages below lifetimes only for the alive"""
    perm = np.arange(cap, dtype=U32)[::-1].copy()
    alive_col = np.full(cap, 0xDEAD, U32)                  # stale rows: out of range, so reading one shows
    alive_col[(head + np.arange(n)) % cap] = perm[:n]
    dead_col = np.full(cap, 0xDEAD, U32)
    dead_col[n:] = perm[n:]
    flags = np.zeros(cap, np.uint8)
    flags[perm[:n]] = 1
    age = np.where(flags == 1, F32(0.5), F32(2.0)).astype(F32)
    life = np.ones(cap, F32)
    return dict(alive_col=alive_col, head=head, dead_col=dead_col, alive_count=n, flags=flags, age=age, life=life, reaps=True)


def check(s, **changes):
    return model_check(**{**s, **changes})


def expect(**counts):
    return {**ZERO, **counts}


@pytest.mark.parametrize("cap,n,head", [(8, 5, 0), (8, 0, 0), (8, 8, 0), (8, 5, 6), (8, 8, 3), (1, 1, 0), (1, 0, 0), (8, 1, 7)])
def test_a_healthy_state_counts_nothing(cap, n, head):
    assert check(healthy(cap, n, head)) == ZERO             # with a head the rows wrap round the column's end; stale rows are not read


def test_rows_behind_a_head_wrap_round_the_end_of_the_column():
    s = healthy(8, 5, head=6)                               # rows 0 .. 4 at indices 6, 7, 0, 1, 2
    assert [int(x) for x in s["alive_col"][[6, 7, 0, 1, 2]]] == [7, 6, 5, 4, 3]
    assert check(s, head=5) == expect(bad_slots=1, alive_byte_mismatches=0)     # the wrong head reads the stale index 5, and not index 2
    assert check(s, head=0) == expect(bad_slots=2)                              # indices 0 .. 4: two stale ones


def test_a_row_naming_a_slot_at_or_beyond_capacity_counts_once_and_in_nothing_else():
    for value in (8, 0xFFFFFFFF):
        s = healthy()
        s["alive_col"][0] = value
        assert check(s) == expect(bad_slots=1)
        s = healthy()
        s["dead_col"][7] = value
        assert check(s) == expect(bad_slots=1)
    s = healthy()
    s["alive_col"][0] = s["dead_col"][6] = 8
    assert check(s) == expect(bad_slots=2)


def test_duplicates_are_rows_minus_distinct_slots():
    s = healthy()
    s["alive_col"][1] = s["alive_col"][0]                   # twice in the alive list: the byte agrees with both rows
    assert check(s) == expect(duplicate_slots=1)
    s["alive_col"][2] = s["alive_col"][0]                   # three times counts 2
    assert check(s) == expect(duplicate_slots=2)
    s = healthy()
    s["dead_col"][6] = s["dead_col"][5]
    s["alive_col"][1] = s["alive_col"][0]                   # two slots named twice each
    assert check(s) == expect(duplicate_slots=2)
    s = healthy()
    s["alive_col"][0] = s["dead_col"][7]                    # across the lists: the alive row names a dead slot, whose age is past its lifetime
    assert check(s) == expect(duplicate_slots=1, alive_byte_mismatches=1, alive_past_lifetime=1)
    assert check(s, reaps=False) == expect(duplicate_slots=1, alive_byte_mismatches=1)


def test_alive_byte_mismatches_count_rows_whose_list_disagrees_with_the_byte():
    s = healthy()
    s["alive_col"][0], s["dead_col"][7] = s["dead_col"][7], s["alive_col"][0]   # an alive row swapped with a dead row
    assert check(s, reaps=False) == expect(alive_byte_mismatches=2)
    s = healthy()
    s["flags"][7] = 0                                       # slot 7 is in the alive list
    assert check(s) == expect(alive_byte_mismatches=1)
    s["flags"][0] = 1                                       # slot 0 is in the dead list
    assert check(s) == expect(alive_byte_mismatches=2)
    s["flags"][7] = 2                                       # only the value 1 says alive
    assert check(s) == expect(alive_byte_mismatches=2)


def test_alive_past_lifetime_is_not_age_below_lifetime_and_only_for_alive_rows_of_a_reaping_program():
    s = healthy()
    s["age"][7] = s["life"][7]                              # age == lifetime
    assert check(s) == expect(alive_past_lifetime=1)
    s["age"][7] = np.nextafter(s["life"][7], F32(-np.inf))
    assert check(s) == ZERO
    s["age"][7] = NAN
    assert check(s) == expect(alive_past_lifetime=1)
    s["age"][7], s["life"][7] = F32(0.5), NAN
    assert check(s) == expect(alive_past_lifetime=1)
    assert check(s, reaps=False) == ZERO
    assert check(s, age=None) == ZERO and check(s, life=None) == ZERO      # a layout without one of the two
    s = healthy()
    s["age"][0] = s["life"][0] = NAN                        # slot 0 is dead
    assert check(s) == ZERO


def test_the_alive_count_decides_which_column_a_row_is_read_from():
    s = healthy(8, 5)
    assert check(s, alive_count=4) == expect(bad_slots=1)   # row 4 is now read from the dead column: stale
    assert check(s, alive_count=6) == expect(bad_slots=1)   # row 5 from the alive column: stale
    s["alive_col"][5] = s["dead_col"][5]                    # ... unless it still names the slot: then the byte and the age object
    assert check(s, alive_count=6) == expect(alive_byte_mismatches=1, alive_past_lifetime=1)


# ---- model_compare ------------------------------------------------------------------------------------------------------------------------------------
def state(cap=8, n=5, head=0, column=0):
    s = healthy(cap, n, head)
    meta = np.array([n, 40, (head << 1) | column, n, cap - n, 3, 1, n], U32)
    rng = np.random.default_rng(1)
    planes = [(2, rng.integers(0, 2 ** 32, cap * 3, dtype=np.uint64).astype(U32)), (5, rng.integers(0, 2 ** 32, cap, dtype=np.uint64).astype(U32)),
              (9, rng.integers(0, 2 ** 32, cap * 4, dtype=np.uint64).astype(U32))]
    return {"meta": meta, "alive_col": s["alive_col"], "dead_col": s["dead_col"], "planes": planes}


EQUAL = {"equal": 1, "counter_diffs": 0, "alive_list_diffs": 0, "dead_list_diffs": 0, "attr_diffs": 0, "first_section": -1, "first_index": 0}


def diff(**fields):
    return {**EQUAL, "equal": 0, **fields}


def test_equal_states_are_equal_wherever_their_rows_live():
    assert model_compare(state(), state()) == EQUAL
    assert model_compare(state(head=6, column=1), state()) == EQUAL          # another head, another column: the same rows
    assert model_compare(state(n=0), state(n=0, head=3)) == EQUAL
    assert model_compare(state(n=8, head=3), state(n=8)) == EQUAL
    a, b = state(), state()
    b["alive_col"][6], b["dead_col"][2] = 1, 2                               # stale rows of either column are not compared
    assert model_compare(a, b) == EQUAL


@pytest.mark.parametrize("word", [w for w in META_WORDS if w != "list_column"])
def test_each_of_the_seven_counter_words_counts(word):
    a, b = state(), state()
    b["meta"][META_WORDS.index(word)] += 1
    d = model_compare(a, b)
    assert d["counter_diffs"] == 1 and d["equal"] == 0
    if word == "indirect_write_index":
        b["meta"][META_WORDS.index(word)] += 1                               # compared by its bit 0
        assert model_compare(a, b) == EQUAL


def test_lists_are_compared_by_logical_row_and_only_under_equal_counts():
    a, b = state(head=6), state()
    b["alive_col"][3] = 99                                                   # logical row 3 of b; in a it lives at index 1
    assert model_compare(a, b) == diff(alive_list_diffs=1, first_section=0, first_index=3)
    a["alive_col"][6] = 98                                                   # a's logical row 0
    assert model_compare(a, b) == diff(alive_list_diffs=2, first_section=0, first_index=0)
    a, b = state(), state()
    b["dead_col"][7] = 99
    assert model_compare(a, b) == diff(dead_list_diffs=1, first_section=1, first_index=2)   # relative to row alive_count
    b["dead_col"][5] = 98
    assert model_compare(a, b) == diff(dead_list_diffs=2, first_section=1, first_index=0)
    b["meta"][0] = 4                                                         # the counts differ: the rows do not correspond
    assert model_compare(a, b) == diff(counter_diffs=1)


def test_an_alive_count_above_the_capacity_is_a_difference_and_skips_the_lists():
    a, b = state(), state()
    a["meta"][0] = b["meta"][0] = 9
    b["alive_col"][0] = 99
    assert model_compare(a, b) == diff(counter_diffs=1)
    b["meta"][0] = 8
    assert model_compare(a, b) == diff(counter_diffs=1)


def test_planes_are_compared_over_capacity_times_ncomp_words_and_reported_by_attribute_id():
    a, b = state(), state()
    b["planes"][2][1][31] ^= 1                                               # the last word of the vec4 plane
    assert model_compare(a, b) == diff(attr_diffs=1, first_section=2 + 9, first_index=31)
    b["planes"][0][1][23] ^= 0x80000000
    b["planes"][0][1][4] ^= 1
    assert model_compare(a, b) == diff(attr_diffs=3, first_section=2 + 2, first_index=4)    # the first section in layout order, its smallest index
    b["dead_col"][6] = 99
    assert model_compare(a, b) == diff(attr_diffs=3, dead_list_diffs=1, first_section=1, first_index=1)
    b["alive_col"][4] = 99
    assert model_compare(a, b) == diff(attr_diffs=3, dead_list_diffs=1, alive_list_diffs=1, first_section=0, first_index=4)
    assert model_compare(b, a) == model_compare(a, b)


def test_words_are_compared_as_bits():
    a, b = state(), state()
    a["planes"][1][1][0], b["planes"][1][1][0] = 0, 0x80000000               # +0 and -0
    assert model_compare(a, b) == diff(attr_diffs=1, first_section=2 + 5, first_index=0)
    a["planes"][1][1][0], b["planes"][1][1][0] = 0x7FC00000, 0x7FC00001      # two NaNs
    assert model_compare(a, b) == diff(attr_diffs=1, first_section=2 + 5, first_index=0)
    b["planes"][1][1][0] = 0x7FC00000                                        # the same NaN
    assert model_compare(a, b) == EQUAL
