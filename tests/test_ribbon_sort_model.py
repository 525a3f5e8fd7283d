"""The key patterns of tests/ribbon_keys.py against the oracle, without a GPU.

tests/test_gpu_ribbon_sort.py drives the product's sort kernels with these keys and checks the result against two things:
the oracle's list and ribbon_keys.expected_list (numpy's stable argsort on the 64-bit key). This file ties the second to the
first - the oracle's stable (RIBBON_ID, AGE bits) sort IS that argsort, on every pattern - and checks that each generator
produces what its name says (which key bytes vary, ties, descending order, ages that cross zero, NaNs that die).
"""
import numpy as np
import pytest

import ribbon_keys as rk
from helpers import A, Frame, OracleRunner

N, CAP = 5000, 6000


def _burst(runner, n):
    runner.step(Frame(0.0, n, 0x5EED, props={"a0": np.float32(0.5), "k": np.array([1], np.uint32)}))


@pytest.fixture(scope="module")
def asset():
    return rk.sort_asset(CAP)


@pytest.mark.parametrize("name", list(rk.PATTERNS))
def test_oracle_sort_equals_the_numpy_model(asset, name):
    gen, dt = rk.PATTERNS[name]
    o = OracleRunner(asset)
    _burst(o, N)
    before = o.fx.alive_list()
    assert len(before) == N
    rid, age = gen(N, 1234)
    assert rid.dtype == np.uint32 and age.dtype == np.uint32 and len(rid) == len(age) == N
    rp, ap, lp = rk.planes(CAP, before, rid, age)
    o.fx.write_attr(A.RIBBON_ID.id, rp)
    o.fx.write_attr(A.AGE.id, ap.view(np.float32))
    o.fx.write_attr(A.LIFETIME.id, lp.view(np.float32))
    assert rk.in_key_order(before, rp, ap) == (name == "all_equal")      # a sort that did nothing would not pass
    o.step(Frame(dt, 0, 0x5EED + 1))
    rid_after = o.fx.read_attr(A.RIBBON_ID.id)
    age_after = o.fx.read_attr(A.AGE.id).view(np.uint32)
    np.testing.assert_array_equal(rid_after, rp)
    alive = rk.survivors(before, age_after, lp)
    want = rk.expected_list(alive, rid_after, age_after)
    np.testing.assert_array_equal(o.fx.alive_list(), want)
    if name == "nan_ages":
        assert len(alive) == N - N // 10                                 # NaN < lifetime is false: the NaNs die, the rest is compacted and sorted
    else:
        assert len(alive) == N
    if dt == 0.0 and name != "nan_ages":
        # a tick of +0 passes every bit pattern through, denormals included; only -0 becomes +0 (x + +0 in round-to-nearest)
        np.testing.assert_array_equal(age_after, np.where(ap == 0x80000000, 0, ap))
    if name == "all_equal":
        np.testing.assert_array_equal(want, before)


def test_generators_make_the_keys_their_names_promise():
    n = 5000
    for b in range(8):
        assert rk.varying_bytes(*rk.PATTERNS[f"one_byte{b}"][0](n, 7)) == [b]
        rid, age = rk.PATTERNS[f"one_byte{b}"][0](n, 7)
        assert len(np.unique(rk.key64(rid, age))) == 256
    assert rk.varying_bytes(*rk.all_equal(n, 7)) == []
    assert rk.varying_bytes(*rk.bytes_0_7(n, 7)) == [0, 7]
    assert rk.varying_bytes(*rk.bytes_1_2_4(n, 7)) == [1, 2, 4]
    assert rk.varying_bytes(*rk.all_bytes(n, 7)) == list(range(8))
    rid, _ = rk.bytes_0_7(n, 7)
    assert {0, 0x80000000, 0xFF000000} <= set(rid.tolist())
    rid, age = rk.all_bytes(n, 7)
    assert {0, 0x80000000, 0xFFFFFFFF} <= set(rid.tolist()) and (age >> 31).any() and not (age >> 31).all()
    assert len(np.unique(rk.key64(*rk.few_distinct(n, 7)))) == 3
    for m in (2, 64, 65, 4097, 266240):
        k = rk.key64(*rk.reversed_keys(m, 7)).astype(np.int64)
        assert (np.diff(k) < 0).all()
    rid, age = rk.age_bit_edges(n, 7)
    assert set(rk.AGE_EDGES.tolist()) <= set(age.tolist()) and age.max() <= 0x7EFFFFFF
    rid, age = rk.signed_ages(n, 7)
    a = age.view(np.float32)
    after = a + np.float32(1 / 60)
    assert (age == 0x80000000).any() and (age == 0).any() and ((a < 0) & (after > 0)).sum() > n // 10 and (after < 0).sum() > n // 10
    rid, age = rk.nan_ages(n, 7)
    nan = np.isnan(age.view(np.float32))
    assert nan.sum() == n // 10 and ((age[nan] & 0x7FC00000) == 0x7FC00000).all() and (age[nan] >> 31).any() and not (age[nan] >> 31).all()
    for name, (gen, _) in rk.PATTERNS.items():          # no generator but nan_ages makes an age that dies, whatever the size
        for m in (0, 1, 64, 65, 257):
            rid, age = gen(m, 3)
            assert len(rid) == len(age) == m
            if name != "nan_ages":
                assert (age.view(np.float32) < rk.LIFETIME).all()
