"""Test helper (no GPU import): the magnitude sweep of the exact flat index — named, seeded corpora and queries away from
unit-scale Gaussian data — and the scale-free exactness check the sweep's results are held to.

``case(name)`` returns ``(x, q, metric, normalize, k)`` with metric 'ip' or 'l2'.  ``check_exact`` compares a result with
``oracle.flat_index``: ids position by position, scores to one float32 spacing.  ``near_tie_queries`` counts, from the
oracle alone, the queries in which ``check_exact`` could ever have to excuse a difference; ``EXCUSE_CAP`` bounds that
count per case (a condition on the inputs, checked on the CPU before any device runs).
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import flat_index as orc

N, NQ, K = 100_000, 64, 10
F16_MAX = 65504.0


def _gauss(seed, n, d, nq=NQ):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, d), dtype=np.float32), rng.standard_normal((nq, d), dtype=np.float32)


def _unit(v):
    return (v / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)


def _scaled(seed, s, n=N, d=64):
    x, q = _gauss(seed, n, d)
    return x * np.float32(s), q * np.float32(s)


def _one_row_out_of_range(seed=7):
    x, q = _gauss(seed, N, 64)
    x[31_337, 3:7] = 70000.0                     # four components beyond +-65504
    q[5] = x[31_337] / np.float32(1000.0)        # one query aimed at that row
    return x, q


def _query_out_of_range(seed, exact_rows):
    """two queries (3 and 40) with one component 1e5: their f16 image holds an infinity"""
    x, q = _gauss(seed, N, 64)
    if exact_rows:
        x = x.astype(np.float16).astype(np.float32)     # rows the f16 image holds exactly: xerr = 0, eps = 0 * inf
    q[3, 11] = 1.0e5
    q[40, 50] = -1.0e5
    return x, q


OUT_OF_RANGE_QUERIES = (3, 40)


def _integers(seed=7, n=N, d=128):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, d)).astype(np.float32), rng.integers(0, 256, (NQ, d)).astype(np.float32))


def _dyadic(seed=7, n=N, d=100):
    rng = np.random.default_rng(seed)
    return ((rng.integers(-64, 65, (n, d)) / 64.0).astype(np.float32), (rng.integers(-64, 65, (NQ, d)) / 64.0).astype(np.float32))


def _far(seed, rows_far):
    """L2 with norms a factor 1000 apart, f16-exact on both sides (the certificate's bound is then the accumulation term
    alone): unit-norm rows under queries of norm 1024, or rows of norm ~1000 (N(0,1) * 125) under unit-norm queries"""
    x, q = _gauss(seed, N, 64)
    if rows_far:
        x, q = x * np.float32(125.0), _unit(q)
    else:
        x, q = _unit(x), _unit(q)
    x, q = x.astype(np.float16).astype(np.float32), q.astype(np.float16).astype(np.float32)
    return (x, q) if rows_far else (x, q * np.float32(1024.0))


def _row_norms(seed=7, n=N, d=64):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=np.float32)
    x *= (10.0 ** rng.uniform(-3.0, 3.0, (n, 1))).astype(np.float32)
    q = rng.standard_normal((NQ, d), dtype=np.float32)
    return x, q


def _tight_band(seed, s, n=N, d=128):
    """the construction of test_tight_clusters_second_pass_is_exact (300 centroids, noise 0.02), scaled"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((300, d)).astype(np.float32)
    x = (cent[rng.integers(0, 300, n)] + 0.02 * rng.standard_normal((n, d))).astype(np.float32)
    q = (cent[rng.integers(0, 300, NQ)] + 0.02 * rng.standard_normal((NQ, d))).astype(np.float32)
    return x * np.float32(s), q * np.float32(s)


def _adversarial(seed, which, n=N, d=64):
    """The Cauchy-Schwarz terms of the bound, met with equality.  Rows are f16-exact values in +-(1, 2) (f16 spacing 2^-10).
    'rows': f16-exact queries (||q16 - q|| = 0), and row i < 64 displaced by a vector parallel to query i, small enough that
    the f16 image still holds the undisplaced row: (image - row) . q16 = -||image - row|| ||q16||.  'queries': every row
    f16-exact (xerr = 0), Gaussian queries, and row i < 64 the longest of the corpus and parallel to query i's own f16
    rounding error: row . (q16 - q) = ||row|| ||q16 - q||."""
    rng = np.random.default_rng(seed)
    x = ((1.0 + rng.integers(1, 1023, (n, d)) / 1024.0) * rng.choice([-1.0, 1.0], (n, d))).astype(np.float32)
    q = rng.standard_normal((NQ, d), dtype=np.float32)
    if which == "rows":
        q = q.astype(np.float16).astype(np.float32)
        delta = 4.0e-4 * q.astype(np.float64) / np.abs(q).max(axis=1, keepdims=True)
        x[:NQ] = (x[:NQ].astype(np.float64) + delta).astype(np.float32)
    else:
        e = q.astype(np.float16).astype(np.float64) - q.astype(np.float64)
        x[:NQ] = (16.0 * e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float16).astype(np.float32)
    return x, q


# name -> (builder, metric, normalize); seeds are part of the case (changed only when a seed breaks EXCUSE_CAP)
# (tight_band_scaled: seed 12, not the 11 of the test it follows, whose inner products hold two near-ties)
_TABLE = {
    "scale_2^-20-ip": (lambda: _scaled(7, 2.0 ** -20), "ip", False),
    "scale_2^-20-l2": (lambda: _scaled(7, 2.0 ** -20), "l2", False),
    "scale_2^-10-ip": (lambda: _scaled(7, 2.0 ** -10, n=262_144), "ip", False),   # >= 262 144 rows: the 12-bit image by default
    "scale_2^-10-l2": (lambda: _scaled(7, 2.0 ** -10), "l2", False),
    "scale_2^8-ip": (lambda: _scaled(7, 2.0 ** 8), "ip", False),
    "scale_2^8-l2": (lambda: _scaled(7, 2.0 ** 8), "l2", False),
    "scale_2^14-ip": (lambda: _scaled(7, 2.0 ** 14), "ip", False),                # some |x| > 65504
    "scale_2^14-l2": (lambda: _scaled(7, 2.0 ** 14), "l2", False),
    "one_row_out_of_range-ip": (_one_row_out_of_range, "ip", False),
    "one_row_out_of_range-l2": (_one_row_out_of_range, "l2", False),
    "query_out_of_range-ip": (lambda: _query_out_of_range(7, False), "ip", False),
    "query_out_of_range-l2": (lambda: _query_out_of_range(8, False), "l2", False),   # (seed 7: one near-tie)
    "query_out_of_range_exact_rows-ip": (lambda: _query_out_of_range(8, True), "ip", False),
    "query_out_of_range_exact_rows-l2": (lambda: _query_out_of_range(8, True), "l2", False),
    "integers_0_255_d128-ip": (_integers, "ip", False),
    "integers_0_255_d128-l2": (_integers, "l2", False),
    "dyadic_unit-ip": (_dyadic, "ip", False),                                       # d = 100: a padded k-block
    "dyadic_unit-l2": (_dyadic, "l2", False),
    "dyadic_unit-cosine": (_dyadic, "ip", True),
    "far_queries-l2": (lambda: _far(7, False), "l2", False),
    "far_rows-l2": (lambda: _far(7, True), "l2", False),
    "row_norms_1e-3_to_1e3-ip": (_row_norms, "ip", False),
    "row_norms_1e-3_to_1e3-l2": (_row_norms, "l2", False),
    "cosine_of_huge_and_tiny_rows-cosine": (_row_norms, "ip", True),
    "tight_band_scaled_2^8-ip": (lambda: _tight_band(12, 2.0 ** 8), "ip", False),
    "tight_band_scaled_2^8-l2": (lambda: _tight_band(12, 2.0 ** 8), "l2", False),
    "tight_band_scaled_2^-10-ip": (lambda: _tight_band(12, 2.0 ** -10), "ip", False),
    "tight_band_scaled_2^-10-l2": (lambda: _tight_band(12, 2.0 ** -10), "l2", False),
    "adversarial_row_rounding-ip": (lambda: _adversarial(7, "rows"), "ip", False),
    "adversarial_row_rounding-l2": (lambda: _adversarial(7, "rows"), "l2", False),
    "adversarial_query_rounding-ip": (lambda: _adversarial(7, "queries"), "ip", False),
    "adversarial_query_rounding-l2": (lambda: _adversarial(7, "queries"), "l2", False),
}
NAMES = tuple(_TABLE)
ROWS_OUT_OF_RANGE = tuple(n for n in NAMES if n.startswith(("scale_2^14", "one_row_out_of_range")))
QUERIES_OUT_OF_RANGE = tuple(n for n in NAMES if n.startswith("query_out_of_range"))
# queries with two neighbours among the first k + 1 exact scores closer than two float32 spacings: float32 ties are
# inherent only where the distances are huge against their spread (ulp32 of a squared distance near 1e6 is 0.0625)
EXCUSE_CAP = {n: 0 for n in NAMES}
EXCUSE_CAP["far_queries-l2"] = 10


def case(name):
    build, metric, normalize = _TABLE[name]
    x, q = build()
    return np.ascontiguousarray(x), np.ascontiguousarray(q), metric, normalize, K


def _two_spacings(a, b):
    return 2.0 * float(np.spacing(np.float32(max(abs(a), abs(b)))))


@functools.lru_cache(maxsize=2)
def _oracle_cached(name, n_rows):
    x, q, metric, normalize, k = case(name)
    return oracle(x[:n_rows] if n_rows else x, q, k, metric, normalize)


def preprocess(v, normalize):
    """what the index stores / searches with: float32 rows, for cosine divided (in float32) by the correctly rounded float32
    norm, zero norms left alone — k_add and k_prepq accumulate the norm in float64.  oracle.preprocess_vectors follows the
    reference's numpy float32 norm, whose last bits depend on numpy's summation order: rows a spacing apart from the stored
    ones would cost the one-spacing score bar several spacings (the GPU tests pin reconstruct_n to this function's rows)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if not normalize:
        return v
    norm = np.sqrt((v.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    return v / np.where(norm == 0, np.float32(1.0), norm)


def oracle(x, q, k, metric, normalize):
    """(Dr, Ir, s64): flat_search's answer and the float64 scores (inner products / squared distances) it ranks"""
    xm, qm = preprocess(x, normalize), preprocess(q, normalize)
    s64 = orc.exact_scores(qm, xm, metric)
    Dr, Ir = orc.flat_search(qm, xm, k, metric, scores=s64)
    return Dr, Ir, s64


def near_tie_queries(s64, k, metric):
    """(queries with two distinct neighbouring scores among the best k + 1 within two float32 spacings, those of them whose
    close pair is the k-th / (k + 1)-th).  Exactly equal float64 scores do not count: both sides break them by id."""
    anywhere, boundary = 0, 0
    for i in range(s64.shape[0]):
        row = -s64[i] if metric == "ip" else s64[i]
        kk = min(k + 1, row.shape[0])
        best = np.sort(row[np.argpartition(row, kk - 1)[:kk]])
        close = [a != b and abs(a - b) <= _two_spacings(a, b) for a, b in zip(best, best[1:])]
        anywhere += any(close)
        boundary += bool(len(close) >= k and close[k - 1])
    return anywhere, boundary


def check_exact(D, I, x, q, k, metric, normalize, ref=None):
    """Assert that (D, I) is the exact top-k of the float32 rows; returns the number of queries that used the excuse.

    ids equal flat_search's position by position.  A difference is excused only between rows whose float64 scores lie
    within two float32 spacings of each other (a swap inside the list) or of the k-th score (a swap across the boundary):
    device and oracle both report float32(float64 sum) and rank by (float32 value, ascending id); the two sums differ only
    in summation order (relative error <= d * 2^-53), so their float32 roundings differ by at most one spacing and only
    next to a rounding midpoint.  Scores: |D - Dr| <= one float32 spacing of |Dr|, elementwise.  Padding (-1 and
    -+FLT_MAX) and best-first order as the unit-scale tests check them."""
    Dr, Ir, s64 = ref if ref is not None else oracle(x, q, k, metric, normalize)
    assert D.shape == Dr.shape and I.shape == Ir.shape and D.dtype == np.float32 and I.dtype == np.int64
    valid = Ir >= 0
    assert np.array_equal(I >= 0, valid), "padding differs"
    assert np.array_equal(D[~valid], Dr[~valid]), "padding scores differ"
    d = np.diff(D.astype(np.float64), axis=1)[valid[:, 1:]]
    assert np.all(d <= 0) if metric == "ip" else np.all(d >= 0), "not best-first"
    err = np.abs(D.astype(np.float64) - Dr.astype(np.float64))[valid]
    tol = np.spacing(np.abs(Dr[valid])).astype(np.float64)
    worst = float(np.max(err / tol, initial=0.0))
    assert worst <= 1.0, f"a score is {worst:.2f} float32 spacings from float32(float64 sum)"
    excused = 0
    for i in np.nonzero((I != Ir).any(axis=1))[0]:
        kk = int(valid[i].sum())
        kth = s64[i, Ir[i, kk - 1]]
        for p in np.nonzero(I[i] != Ir[i])[0]:
            a, b = s64[i, I[i, p]], s64[i, Ir[i, p]]
            inside = I[i, p] in Ir[i] and Ir[i, p] in I[i]
            other = b if inside else kth
            ok = abs(a - other) <= _two_spacings(a, other) and abs(b - other) <= _two_spacings(b, other) and a != b
            assert ok, (f"query {i} position {p}: row {I[i, p]} (exact {a!r}) where the oracle has row {Ir[i, p]} "
                        f"(exact {b!r}); k-th exact score {kth!r}")
        excused += 1
    return excused


def check_case(name, D, I, n_rows=0, queries=None, k=None):
    """check_exact for case `name` (optionally its first n_rows rows, a subset of its queries, another k); asserts that
    no more queries were excused than the case's cap"""
    x, q, metric, normalize, k0 = case(name)
    if k is None and n_rows == 0:
        Dr, Ir, s64 = _oracle_cached(name, 0)
    else:
        Dr, Ir, s64 = oracle(x[:n_rows] if n_rows else x, q, k or k0, metric, normalize)
    if queries is not None:
        Dr, Ir, s64 = Dr[queries], Ir[queries], s64[queries]
    excused = check_exact(D, I, None, None, k or k0, metric, normalize, ref=(Dr, Ir, s64))
    assert excused <= EXCUSE_CAP[name], (name, excused)
    return excused
