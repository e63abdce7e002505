"""The device radix sort (csrc/radix_sort.hip) on its own terms: the WHOLE output permutation, compared exactly with
the stable order of tests/order_ref.py, at every key pattern and at every length where a structure of the sort has an
edge (a wave, a round of 256, a tile of 4096, a digit histogram of exactly one 1024-entry scan chunk, one past it).
No tolerance anywhere in this file.

Two public entry points return the sort's full output:
  * float32 keys, ``radix_sort_pairs_f32``: ``FlatIndex.search`` with k > 1024 on an inner-product index without
    normalisation whose COLUMNS are the key patterns, queried with the unit vectors.  The dense exact kernel accumulates
    in float64 and rounds once, so the score of row i for query j is x[i, j] * 1 plus exact zeros: the array handed to the
    sort is the pattern itself (a zero of either sign arrives as +0.0), and k = max(n, 1025) returns every position.
    Squared-L2 on one-dimensional integer rows drives the ascending sort the same way (x * x is exact).
  * 64-bit keys, ``radix_sort_pairs_u64``: ``anr_fuse_rrf_long`` with one list in the dense slot, weights (1, 0, 0, 0)
    and pool = n.  The final of the id at rank r is 1 / (60 + r), strictly decreasing, so the two closing sorts (ascending
    on tie keys whose upper bytes are zero, descending on the finals) keep the rank order and ``out_ids`` is the list's
    ids in the stable descending order of its float64 scores — keys that use all eight bytes, NaN, infinities and
    denormals included.  Two lists in opposite orders make every final occur twice and leave the order to the tie key.

What this file cannot see: ``-0.0`` never reaches the float32 sort.  The dense exact kernel starts its float64 sum at +0.0
and +0.0 + -0.0 is +0.0, so a zero score is always +0.0 and ``rs_f2ord``'s canonicalisation of ``-0.0`` has no input
that exercises it through ``search`` (removing it changes no result here).  Its float64 twin in fusion_rrf_long.hip
(``ra_d2ord``) is exercised: ``sign_mix`` and ``random_bits`` interleave both zeros, and their order is by position.

Asserted: 14 lengths x 14 float32 patterns (descending) + 4 lengths x 8 integer patterns (ascending) + 14 lengths x 18
float64 patterns = 480 (length, pattern, route) cases, plus the id offset, scratch reuse, pool padding and cross-list
cases; none skipped.  The whole file runs in about 3 s on an MI355X, no test above 0.3 s.
"""
import ctypes as C

import numpy as np
import pytest

import order_ref
from order_ref import LENGTHS, stable_order

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.402823466e+38)
L2_LENGTHS = (257, 4096, 4097, 16385)
CROSS_LENGTHS = (4097, 16385)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------------------------------------------------------
# float32 keys, descending: FlatIndex.search beyond the select window
# ---------------------------------------------------------------------------------------------------------------
def _ip_index(x):
    from anorag_hip import FlatIndex, METRIC_IP
    idx = FlatIndex(x.shape[1], METRIC_IP, normalize=False)
    idx.add(x)
    return idx


def _check_columns(D, I, x, names, n, k, id_offset=0, tag=""):
    """row j of (D, I) is the complete descending sort of column j of x"""
    assert D.shape == I.shape == (x.shape[1], k) and k >= n
    for j, name in enumerate(names):
        keys = np.ascontiguousarray(x[:, j])
        order = stable_order(keys, descending=True)
        where = (tag, name, n)
        assert np.array_equal(I[j, :n], order + id_offset), where
        assert np.array_equal(D[j, :n], keys[order]), where          # (value equality: the sort returns -0.0 as +0.0)
        assert np.all(I[j, n:] == -1) and np.all(D[j, n:] == -FLT_MAX), where


@pytest.mark.parametrize("n", LENGTHS)
def test_f32_descending_whole_permutation_at_every_pattern(n):
    """I[j, :n] == stable_order(pattern j, descending) and D[j, :n] the keys in that order, for all 14 float32 patterns
    at once (one index per length, the patterns are its columns); -1 / -FLT_MAX beyond n; every query counted as
    answered by the dense exact path, i.e. by the sort"""
    names, x = order_ref.pattern_matrix("f32", n, seed=1000 + n)
    P = len(names)
    assert P == 14 and all(order_ref.f32_in_range(np.ascontiguousarray(c)) for c in x.T)
    k = max(n, 1025)
    idx = _ip_index(x)
    try:
        D, I = idx.search(np.eye(P, dtype=np.float32), k)
        st = idx.last_stats()
        assert st["n_dense_exact"] == P and st["n_queries"] == P, st
        _check_columns(D, I, x, names, n, k)
    finally:
        idx.close()


def test_f32_id_offset_shifts_ids_and_not_the_padding():
    """ANR_OPT_ID_OFFSET: the ids of the sorted rows shift, the -1 padding beyond n does not"""
    from anorag_hip._lib import OPT_ID_OFFSET
    n, k = 257, 1025
    names, x = order_ref.pattern_matrix("f32", n, seed=77)
    idx = _ip_index(x)
    try:
        idx.set_option(OPT_ID_OFFSET, 5000)
        D, I = idx.search(np.eye(len(names), dtype=np.float32), k)
        assert idx.last_stats()["n_dense_exact"] == len(names)
        _check_columns(D, I, x, names, n, k, id_offset=5000, tag="offset")
    finally:
        idx.close()


def test_f32_sort_scratch_reused_by_a_smaller_corpus():
    """16385 rows first, then reset() and 4097 rows on the SAME index: the second search reuses the larger sort scratch
    and its row numbers (largek.hip) — same results as a fresh index, and as the reference"""
    names, big = order_ref.pattern_matrix("f32", 16385, seed=31)
    _, small = order_ref.pattern_matrix("f32", 4097, seed=32)
    q = np.eye(len(names), dtype=np.float32)
    idx = _ip_index(big)
    fresh = _ip_index(small)
    try:
        D0, I0 = idx.search(q, 16385)
        _check_columns(D0, I0, big, names, 16385, 16385, tag="first")
        idx.reset()
        assert idx.ntotal == 0
        idx.add(small)
        D1, I1 = idx.search(q, 4097)
        assert idx.last_stats()["n_dense_exact"] == len(names)
        D2, I2 = fresh.search(q, 4097)
        assert np.array_equal(I1, I2) and np.array_equal(_bits(D1), _bits(D2))
        _check_columns(D1, I1, small, names, 4097, 4097, tag="reused")
        # ... and k > n on the reused scratch: padding after the 4097 sorted rows, nothing of the 16385 earlier ones
        D3, I3 = idx.search(q, 5000)
        _check_columns(D3, I3, small, names, 4097, 5000, tag="reused-padded")
    finally:
        idx.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------
# float32 keys, ascending: squared L2 on one-dimensional integer rows
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", L2_LENGTHS)
def test_f32_ascending_whole_permutation_l2(n):
    """dimension 1, query 0, integer rows with |x| <= 2048: the distance is x * x, exact in float32 however it is formed;
    expected order stable_order(x * x, ascending), +FLT_MAX / -1 beyond n"""
    from anorag_hip import FlatIndex, METRIC_L2
    k = max(n, 1025)
    pats = order_ref.small_int_patterns(n, seed=2000 + n)
    assert [name for name, _ in pats] == ["all_equal", "two_values_p1", "two_values_p3", "two_values_p64",
                                          "two_values_p256", "few_distinct", "ascending", "descending"]
    idx = FlatIndex(1, METRIC_L2, normalize=False)
    try:
        for name, rows in pats:
            idx.reset()
            idx.add(rows.reshape(n, 1))
            D, I = idx.search(np.zeros((1, 1), dtype=np.float32), k)
            assert idx.last_stats()["n_dense_exact"] == 1
            keys = rows * rows
            assert np.array_equal(keys.astype(np.float64), rows.astype(np.float64) ** 2)  # exact
            order = stable_order(keys, descending=False)
            assert np.array_equal(I[0, :n], order), (name, n)
            assert np.array_equal(D[0, :n], keys[order]), (name, n)
            assert np.all(I[0, n:] == -1) and np.all(D[0, n:] == FLT_MAX), (name, n)
    finally:
        idx.close()


# ---------------------------------------------------------------------------------------------------------------
# 64-bit keys: anr_fuse_rrf_long, the whole pool returned
# ---------------------------------------------------------------------------------------------------------------
def _rrf_long(lists, n, weights, pool, rrf_k=60.0):
    """one query through the C entry point, as retrieval/hybrid_search.py calls it; lists = 4 x ((ids, scores) | None)"""
    from anorag_hip import _lib
    offs = np.zeros((1, 5), dtype=np.int64)
    all_ids, all_sc = [], []
    pos = 0
    for s, l in enumerate(lists):
        offs[0, s] = pos
        if l is not None:
            all_ids.append(np.asarray(l[0], dtype=np.int64))
            all_sc.append(np.asarray(l[1], dtype=np.float64))
            pos += len(l[0])
    offs[0, 4] = pos
    ids = np.ascontiguousarray(np.concatenate(all_ids))
    sc = np.ascontiguousarray(np.concatenate(all_sc))
    w = np.asarray(weights, dtype=np.float64)
    o_ids = np.full((1, pool), -7, dtype=np.int64)
    o_fin = np.full((1, pool), -7.0, dtype=np.float64)
    o_src = np.full((1, pool, 4), -7.0, dtype=np.float64)
    o_cnt = np.full((1,), -7, dtype=np.int32)
    _lib.check(_lib.load().anr_fuse_rrf_long(0, 1, ids.ctypes.data, sc.ctypes.data, offs.ctypes.data, n, w.ctypes.data,
                                             C.c_double(rrf_k), pool, o_ids.ctypes.data, o_fin.ctypes.data,
                                             o_src.ctypes.data, o_cnt.ctypes.data), "anr_fuse_rrf_long")
    return o_ids[0], o_fin[0], o_src[0], int(o_cnt[0])


def _check_single_list(ids, scores, n, pool, where):
    o_ids, o_fin, o_src, cnt = _rrf_long([(ids, scores), None, None, None], n, (1.0, 0.0, 0.0, 0.0), pool)
    order = stable_order(scores, descending=True)
    assert cnt == n, where
    assert np.array_equal(o_ids[:n], ids[order]), where
    finals = 1.0 / (60.0 + np.arange(1, n + 1, dtype=np.float64))
    assert np.array_equal(_bits(o_fin[:n]), _bits(finals)), where                       # bit for bit
    assert np.array_equal(o_src[:n, 0], scores[order], equal_nan=True), where
    assert np.all(np.isnan(o_src[:n, 1:])), where                                       # no other source
    assert np.all(o_ids[n:] == -1) and np.array_equal(_bits(o_fin[n:]), np.zeros(pool - n, dtype=np.uint64)), where


@pytest.mark.parametrize("n", LENGTHS)
def test_u64_descending_whole_permutation_at_every_pattern(n):
    """out_ids == ids[stable_order(scores, descending)] for all 18 float64 patterns (NaN below every number, -0.0 == +0.0,
    infinities, denormals), the ids a fixed random permutation so that a key / value mix-up cannot hide; the finals
    1 / (60 + r) bit for bit; the raw scores back in that order"""
    ids = np.random.default_rng(4000 + n).permutation(n).astype(np.int64)
    pats = order_ref.patterns("f64")
    assert len(pats) == 18
    for j, (name, fn) in enumerate(pats):
        _check_single_list(ids, fn(n, 3000 + n + j), n, n, (name, n))


def test_u64_pool_beyond_the_list_pads_and_keeps_the_count():
    """pool = n + 7: the seven entries after the sorted list are -1 / 0.0 and the count is still n"""
    n = 4097
    ids = np.random.default_rng(5).permutation(n).astype(np.int64)
    for j, (name, fn) in enumerate(order_ref.patterns("f64")):
        _check_single_list(ids, fn(n, 600 + j), n, n + 7, (name, "pool n + 7"))


@pytest.mark.parametrize("n", CROSS_LENGTHS)
def test_u64_cross_list_ties_over_the_whole_pool(n):
    """two full lists, dense and bm25, weights (1, 1, 0, 0), the bm25 order the reverse of the dense order: every final
    1/(60+r) + 1/(60+n+1-r) occurs twice and the tie key (first source holding the id, its rank there) decides.  Ids and
    finals of the WHOLE pool against oracle.fusion.fuse on the same lists"""
    from oracle.fusion import fuse
    rng = np.random.default_rng(9000 + n)
    ids_d = rng.permutation(n).astype(np.int64)
    sc_d = order_ref.few_distinct("f64", n, 17)                 # ties inside the dense list too
    rank_d = np.empty(n, dtype=np.int64)                        # dense rank of every id, from 1
    rank_d[ids_d[stable_order(sc_d, descending=True)]] = np.arange(1, n + 1)
    ids_b = rng.permutation(n).astype(np.int64)                 # the bm25 list in an order of its own
    sc_b = rank_d[ids_b].astype(np.float64) * 0.37              # the worse the dense rank, the better the bm25 score
    ref = fuse(dense=list(zip(ids_d.tolist(), sc_d.tolist())), bm25=list(zip(ids_b.tolist(), sc_b.tolist())),
               candidate_pool=n, fusion_method="rrf", weights={"dense": 1.0, "bm25": 1.0}, rrf_k=60.0)
    assert len(ref) == n
    ref_ids = np.asarray([r["note_id"] for r in ref], dtype=np.int64)
    ref_fin = np.asarray([r["final_similarity"] for r in ref], dtype=np.float64)
    assert len(np.unique(ref_fin)) <= (n + 1) // 2              # every final is shared: the tie key orders each pair
    o_ids, o_fin, o_src, cnt = _rrf_long([(ids_d, sc_d), (ids_b, sc_b), None, None], n, (1.0, 1.0, 0.0, 0.0), n)
    assert cnt == n
    assert np.array_equal(o_ids, ref_ids), n
    assert np.array_equal(_bits(o_fin), _bits(ref_fin)), n
    by_id_d = np.empty(n)
    by_id_d[ids_d] = sc_d
    by_id_b = np.empty(n)
    by_id_b[ids_b] = sc_b
    assert np.array_equal(o_src[:, 0], by_id_d[o_ids]) and np.array_equal(o_src[:, 1], by_id_b[o_ids])
    assert np.all(np.isnan(o_src[:, 2:]))
