"""Plain reference for the tests of the device radix sort (csrc/radix_sort.hip): the permutation a stable sort produces,
and the key patterns at which a radix sort goes wrong.  numpy and Python only — nothing here imports the library.

``stable_order(keys, descending)`` is the expected output order: ties keep their input position, ``-0.0 == +0.0`` and a
NaN ranks below every number, stably among NaNs (the rule fusion_rrf_long.hip documents for its float64 scores).

The generators are deterministic from ``(n, seed)``.  ``patterns("f32")`` / ``patterns("f64")`` list them by name:
  all_equal, two_values_p{1,3,64,256}, few_distinct (16 values), ascending, descending, sign_mix (both signs, both zeros,
  every value repeated), one_byte_varies_b{j} (all keys equal except byte j of the bit image: every other pass of an
  8-bit LSD sort sees a single digit and pass j carries the whole order), random_bits (uniformly random bit images).
The float32 generators stay inside ``f32_in_range``: finite, zero or normal, |x| < 6e4 (the values are stored in an index
that also keeps an f16 image), so byte 3 of a float32 (sign and the upper exponent bits) takes a restricted set of values
and ``random_bits`` folds its exponent field into the allowed range.  The float64 generators are unconstrained:
``sign_mix`` and ``random_bits`` hold denormals, both infinities and NaNs of several bit images.
"""
from __future__ import annotations

import numpy as np

# the sizes at which each structure of the sort has an edge: a wave (64), a round (256), a tile (4096), a full second
# tile (8192), a digit histogram of exactly one scan chunk (16384 = 4 tiles x 256 digits = 1024 entries), one entry past
# it (16385: the scan carry) and a ragged sixth tile (20481)
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 16384, 16385, 20481)

F32_LIMIT = 6.0e4
F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)


def stable_order(keys, descending: bool) -> np.ndarray:
    """positions of ``keys`` in stable sorted order (int64): ties by input position, -0.0 == +0.0, NaN below every number"""
    a = np.asarray(keys).astype(np.float64)  # (float32 -> float64 is exact)
    nan = np.isnan(a)
    is_number = (~nan).astype(np.int64)       # 0 for a NaN: below every number
    value = np.where(nan, 0.0, a)
    if descending:                            # a stable descending sort is the stable ascending sort of the negated keys
        is_number, value = -is_number, -value
    # lexsort: last key is the primary one; a stable merge sort comparing with `<`, so -0.0 and +0.0 tie
    return np.lexsort((value, is_number)).astype(np.int64)


def f32_in_range(x) -> bool:
    """the constraint on every float32 pattern: finite, zero or normal, |x| < 6e4"""
    x = np.asarray(x)
    if x.dtype != np.float32 or not np.all(np.isfinite(x)):
        return False
    m = np.abs(x.astype(np.float64))
    return bool(np.all((m == 0.0) | ((m >= F32_MIN_NORMAL) & (m < F32_LIMIT))))


def _types(dtype):
    if dtype == "f32":
        return np.float32, np.uint32, 4
    if dtype == "f64":
        return np.float64, np.uint64, 8
    raise ValueError(dtype)


def all_equal(dtype, n, seed):
    ft, _, _ = _types(dtype)
    return np.full(n, -1.75 + (seed % 5), dtype=ft)


def two_values(dtype, n, seed, period):
    ft, _, _ = _types(dtype)
    lo, hi = ft(-2.5 - (seed % 3)), ft(7.0)
    return np.where((np.arange(n) // period) % 2 == 0, hi, lo).astype(ft)


def few_distinct(dtype, n, seed):
    ft, _, _ = _types(dtype)
    rng = np.random.default_rng(seed)
    vals = (np.arange(16, dtype=np.float64) - 7.5) * 3.25  # 16 values, eight of each sign
    return vals[rng.integers(0, 16, size=n)].astype(ft)


def ascending(dtype, n, seed):
    ft, _, _ = _types(dtype)
    return ((np.arange(n, dtype=np.float64) - n // 2) * 0.5 + (seed % 2) * 0.25).astype(ft)  # strictly increasing


def descending(dtype, n, seed):
    return ascending(dtype, n, seed)[::-1].copy()


def sign_mix(dtype, n, seed):
    """positive and negative values and both zeros, every drawn value repeated three times in a row"""
    ft, _, _ = _types(dtype)
    rng = np.random.default_rng(seed)
    pool = [-0.0, 0.0, -0.0, 0.0, -1.5, 1.5, -3.0, 3.0, -1024.25, 1024.25, -2.0 ** -20, 2.0 ** -20]
    if dtype == "f64":
        pool += [np.inf, -np.inf, np.nan, -np.nan, 5e-324, -5e-324, 2.0 ** -1040, -(2.0 ** -1040), 1e300, -1e300]
    pool = np.asarray(pool, dtype=ft)
    draws = rng.integers(0, len(pool), size=n // 3 + 1)
    return np.repeat(pool[draws], 3)[:n].copy()


# byte 3 of a float32 is the sign and the upper seven exponent bits: with bit 23 of the base image set, 0x30..0x46 are the
# exponent fields 97..141, i.e. magnitudes 2^-30 .. < 2^15 — normal and below 6e4 — under either sign (46 distinct values)
_F32_BASE = 0x3FA55A3C
_F32_BYTE3 = np.asarray([s | e for s in (0x00, 0x80) for e in range(0x30, 0x47)], dtype=np.uint32)
_F64_BASE = 0x3FF5A53CC35A96E1


def one_byte_varies(dtype, n, seed, j):
    """all keys equal except byte ``j`` of the bit image"""
    ft, ut, nbytes = _types(dtype)
    assert 0 <= j < nbytes
    rng = np.random.default_rng(seed + 101 * j)
    if dtype == "f32" and j == 3:
        byte = _F32_BYTE3[rng.integers(0, len(_F32_BYTE3), size=n)]
    else:
        byte = rng.integers(0, 256, size=n).astype(ut)
    base = ut(_F32_BASE if dtype == "f32" else _F64_BASE)
    shift = ut(8 * j)
    bits = (base & ~(ut(0xFF) << shift)) | (byte.astype(ut) << shift)
    return bits.astype(ut).view(ft).copy()


def random_bits(dtype, n, seed):
    """uniformly random bit images; float32: the exponent field folded into 1..141 (normal, below 6e4), float64: raw
    bits with NaNs, infinities, denormals and zeros written over a sixteenth of the positions (raw bits alone hold one
    such key in a thousand)"""
    ft, ut, _ = _types(dtype)
    rng = np.random.default_rng(seed)
    if dtype == "f32":
        bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        exp = (bits >> np.uint32(23)) & np.uint32(0xFF)
        exp = np.uint32(1) + exp % np.uint32(141)
        bits = (bits & np.uint32(0x807FFFFF)) | (exp << np.uint32(23))
        return bits.view(np.float32).copy()
    bits = rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)
    special = np.asarray([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,  # NaNs
                          0x7FF0000000000000, 0xFFF0000000000000,                                          # +-inf
                          0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,  # denormals
                          0x0000000000000000, 0x8000000000000000], dtype=np.uint64)                        # +-0
    hit = rng.random(n) < 1.0 / 16.0
    bits[hit] = special[rng.integers(0, len(special), size=int(hit.sum()))]
    return bits.view(np.float64).copy()


def patterns(dtype):
    """[(name, fn(n, seed) -> keys)] — every pattern of the given key type ('f32' or 'f64')"""
    _, _, nbytes = _types(dtype)
    out = [("all_equal", lambda n, seed: all_equal(dtype, n, seed))]
    for p in (1, 3, 64, 256):
        out.append((f"two_values_p{p}", lambda n, seed, p=p: two_values(dtype, n, seed, p)))
    out += [("few_distinct", lambda n, seed: few_distinct(dtype, n, seed)),
            ("ascending", lambda n, seed: ascending(dtype, n, seed)),
            ("descending", lambda n, seed: descending(dtype, n, seed)),
            ("sign_mix", lambda n, seed: sign_mix(dtype, n, seed))]
    for j in range(nbytes):
        out.append((f"one_byte_varies_b{j}", lambda n, seed, j=j: one_byte_varies(dtype, n, seed, j)))
    out.append(("random_bits", lambda n, seed: random_bits(dtype, n, seed)))
    return out


def pattern_matrix(dtype, n, seed=0):
    """(names, [n, P] array): column j is pattern j at length n (seed + j)"""
    ps = patterns(dtype)
    cols = [fn(n, seed + j) for j, (_, fn) in enumerate(ps)]
    return [name for name, _ in ps], np.stack(cols, axis=1)


def small_int_patterns(n, seed=0):
    """[(name, float32 keys)]: integer-valued rows with |x| <= 2048, whose squares are exact in float32 however they are
    formed — the keys of the ascending (L2) sort"""
    rng = np.random.default_rng(seed)
    span = np.arange(n, dtype=np.int64)
    asc = (span * 2048 // max(n, 1) + 1) * np.where(span % 2 == 0, 1, -1)  # |x| = 1 .. 2048 non-decreasing, signs alternate
    out = [("all_equal", np.full(n, -37, dtype=np.int64))]
    for p in (1, 3, 64, 256):
        out.append((f"two_values_p{p}", np.where((span // p) % 2 == 0, 2048, -3)))
    out += [("few_distinct", (np.arange(16) * 131 - 1000)[rng.integers(0, 16, size=n)]),
            ("ascending", asc), ("descending", asc[::-1].copy())]
    for _, v in out:
        assert np.all(np.abs(v) <= 2048)
    return [(name, v.astype(np.float32)) for name, v in out]
