"""The reference of the device-sort tests (tests/order_ref.py) checked on its own, so that test_device_sort_gpu.py
never compares the kernel with a reference that is itself wrong: ``stable_order`` against Python's stable ``sorted`` on
every generator, and every float32 generator against the value constraints it promises, at every tested length."""
import math

import numpy as np
import pytest

import order_ref

N_SMALL = 257


def _python_order(keys, descending):
    """the same order from Python's sort: NaN below every number, ties by position (sorted is stable, also reversed)"""
    vals = [float(v) for v in keys]

    def key(i):
        v = vals[i]
        return (0, 0.0) if math.isnan(v) else (1, v)  # (-0.0 == 0.0 in Python's comparison too)

    return sorted(range(len(vals)), key=key, reverse=descending)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("desc", [True, False])
def test_stable_order_matches_pythons_sorted_on_every_generator(dtype, desc):
    for j, (name, fn) in enumerate(order_ref.patterns(dtype)):
        keys = fn(N_SMALL, 7 + j)
        assert keys.shape == (N_SMALL,) and keys.dtype == (np.float32 if dtype == "f32" else np.float64), name
        got = order_ref.stable_order(keys, desc)
        assert got.dtype == np.int64 and list(got) == _python_order(keys, desc), (dtype, name, desc)
    for name, keys in order_ref.small_int_patterns(N_SMALL, 3):
        sq = keys * keys
        assert list(order_ref.stable_order(sq, desc)) == _python_order(sq, desc), name


def test_stable_order_tie_rules_by_hand():
    nan = float("nan")
    keys = np.asarray([0.0, nan, -0.0, 1.0, -np.inf, nan, 1.0, 0.0, np.inf, 5e-324])
    #                  0    1     2    3     4       5    6    7     8      9
    assert list(order_ref.stable_order(keys, True)) == [8, 3, 6, 9, 0, 2, 7, 4, 1, 5]
    assert list(order_ref.stable_order(keys, False)) == [1, 5, 4, 0, 2, 7, 9, 3, 6, 8]
    assert list(order_ref.stable_order(np.zeros(0), True)) == []


def test_generators_are_deterministic_and_hold_what_they_promise():
    n = 4097
    for dtype in ("f32", "f64"):
        names, m = order_ref.pattern_matrix(dtype, n, seed=5)
        names2, m2 = order_ref.pattern_matrix(dtype, n, seed=5)
        assert names == names2 and m.tobytes() == m2.tobytes()
        nbytes = 4 if dtype == "f32" else 8
        assert len(names) == len(set(names)) == 10 + nbytes and m.shape == (n, len(names))
        col = dict(zip(names, m.T))
        assert len(np.unique(col["all_equal"])) == 1
        for p in (1, 3, 64, 256):
            c = col[f"two_values_p{p}"]
            assert len(np.unique(c)) == 2
            flips = np.nonzero(c[1:] != c[:-1])[0] + 1
            assert np.array_equal(flips, np.arange(p, n, p))  # the value changes every p elements
        assert len(np.unique(col["few_distinct"])) == 16
        assert np.all(np.diff(col["ascending"]) > 0) and np.all(np.diff(col["descending"]) < 0)
        sm = col["sign_mix"]
        assert np.any(sm > 0) and np.any(sm < 0)
        assert np.any((sm == 0) & np.signbit(sm)) and np.any((sm == 0) & ~np.signbit(sm))  # both zeros
        ut = np.uint32 if dtype == "f32" else np.uint64
        triples = np.ascontiguousarray(sm[:n - n % 3]).view(ut).reshape(-1, 3)
        assert np.all(triples == triples[:, :1])                        # every value repeated
        for j in range(nbytes):
            bits = np.ascontiguousarray(col[f"one_byte_varies_b{j}"]).view(ut)
            diff = bits ^ bits[0]
            assert np.all(diff & ~(ut(0xFF) << ut(8 * j)) == 0)        # only byte j differs
            distinct = len(np.unique(bits))
            assert distinct >= (4 if (dtype, j) == ("f32", 3) else 200)
            if j == nbytes - 1:
                assert np.any(np.signbit(col[f"one_byte_varies_b{j}"])) and not np.all(np.signbit(col[f"one_byte_varies_b{j}"]))
        rb = np.ascontiguousarray(col["random_bits"]).view(ut)
        for j in range(nbytes):                                        # every byte of the image varies
            assert len(np.unique((rb >> ut(8 * j)) & ut(0xFF))) > 40
    rb = order_ref.random_bits("f64", n, 1)
    sm = order_ref.sign_mix("f64", n, 1)
    tiny = np.finfo(np.float64).tiny
    for a in (rb, sm):
        assert np.any(np.isnan(a)) and np.any(a == np.inf) and np.any(a == -np.inf)
        assert np.any((a != 0) & (np.abs(a) < tiny))                   # denormals


@pytest.mark.parametrize("n", order_ref.LENGTHS)
def test_f32_generators_stay_finite_normal_and_below_6e4(n):
    names, m = order_ref.pattern_matrix("f32", n, seed=n)
    assert m.dtype == np.float32 and m.shape[0] == n
    for name, c in zip(names, m.T):
        assert order_ref.f32_in_range(np.ascontiguousarray(c)), (name, n)
    for name, keys in order_ref.small_int_patterns(n, n):
        assert keys.dtype == np.float32 and np.all(keys == np.rint(keys)) and np.all(np.abs(keys) <= 2048), name
    # the check itself refuses what it must
    for bad in (np.inf, np.nan, 6.0e4, -7.0e4, 1e-39):
        assert not order_ref.f32_in_range(np.asarray([1.0, bad], dtype=np.float32))
