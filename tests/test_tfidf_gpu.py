"""GPU tests of the TF-IDF join (anr_tfidf_*, anorag_hip.note_dedup): the device equals the numpy restatement
(tests/tfidf_ref.py) and the reference's own output (tests/golden/dedup_cases.npz) exactly — pairs as integers, values by
their bits — at the smallest shapes where the kernels can go wrong."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import tfidf_ref as ref
from test_tfidf_cpu import BAD_CREATE, _create

pytestmark = pytest.mark.gpu
FILE = ref.load_file()
CASES = FILE["cases"]
WITH_CSR = [c for c in CASES if c["csr"] is not None]
ANR_EINVAL, ANR_ESTATE = -1, -3


class Raw:
    """the C ABI as it is, from a CSR of labels and values"""

    def __init__(self, indptr, terms, values, n_terms):
        from anorag_hip import _lib as L
        self.L, self.lib = L, L.load()
        self.indptr = np.ascontiguousarray(indptr, np.int64)
        self.terms = np.ascontiguousarray(terms, np.int32)
        self.values = np.ascontiguousarray(values, np.float64)
        self.n_rows, self.n_terms = len(self.indptr) - 1, n_terms
        self.h = C.c_void_p()
        rc = self.lib.anr_tfidf_create(0, self.n_rows, n_terms, self.indptr.ctypes.data, self.terms.ctypes.data,
                                       self.values.ctypes.data, C.byref(self.h))
        assert rc == 0, L.last_error()

    def slots(self, s):
        assert self.lib.anr_tfidf_set_option(self.h, 1, s) == 0, self.L.last_error()

    def join_raw(self, threshold):
        npairs = C.c_int64(-7)
        stats = np.full(8, -7, np.int64)
        rc = self.lib.anr_tfidf_self_join(self.h, threshold, C.byref(npairs), stats.ctypes.data)
        return rc, npairs.value, stats

    def join(self, threshold):
        rc, npairs, stats = self.join_raw(threshold)
        assert rc == 0, self.L.last_error()
        out = (np.full(npairs, -7, np.int32), np.full(npairs, -7, np.int32), np.full(npairs, -7.0, np.float64))
        assert self.lib.anr_tfidf_self_join_fetch(self.h, *[a.ctypes.data for a in out]) == 0, self.L.last_error()
        assert stats[3] == npairs and stats[2] >= npairs and stats[5] in (64, 4096)
        return out, stats

    def scores_raw(self, q_indptr, q_terms, q_weights):
        q_indptr = np.ascontiguousarray(q_indptr, np.int64)
        q_terms = np.ascontiguousarray(q_terms, np.int32)
        q_weights = np.ascontiguousarray(q_weights, np.float64)
        out = np.full((len(q_indptr) - 1, self.n_rows), -7.0, np.float64)
        rc = self.lib.anr_tfidf_scores(self.h, len(q_indptr) - 1, q_indptr.ctypes.data, q_terms.ctypes.data,
                                       q_weights.ctypes.data, out.ctypes.data)
        return rc, out

    def close(self):
        if self.h.value:
            assert self.lib.anr_tfidf_destroy(self.h) == 0
            self.h = C.c_void_p()


def same_arrays(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (k, np.flatnonzero(g != w)[:8])


def check_against_ref(indptr, terms, values, n_terms, thresholds):
    s = ref.pair_matrix(indptr, terms, values, n_terms)
    raw = Raw(indptr, terms, values, n_terms)
    try:
        for t in thresholds:
            got, stats = raw.join(t)
            same_arrays(got, ref.duplicates(s, t))
        return s, stats
    finally:
        raw.close()


# ---- goldens
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_detect_duplicate_notes_equals_the_reference(case):
    from anorag_hip import detect_duplicate_notes
    notes = copy.deepcopy(case["notes"])
    got = detect_duplicate_notes(notes)
    want = ref.load_expected(case)
    ref.same_result(got, want)
    assert all(type(v) is np.float64 for _, _, v in got["semantic_duplicates"]) or case["csr"] is None
    assert [np.float64(v).tobytes() for _, _, v in got["semantic_duplicates"]] == \
        [np.float64(v).tobytes() for _, _, v in want["semantic_duplicates"]]


@pytest.mark.parametrize("case", WITH_CSR, ids=[c["name"] for c in WITH_CSR])
def test_join_of_the_recorded_matrix_is_bit_equal_to_sklearn(case):
    from anorag_hip import TfidfJoin
    ids = [n.get("note_id", "") for n in case["notes"]]
    with TfidfJoin(ref.Csr(case["csr"])) as join:
        I, J, sim, stats = join.duplicates(0.85, return_stats=True)
    want = ref.tuples(case["expected"]["semantic_duplicates"])
    assert [(ids[i], ids[j]) for i, j in zip(I.tolist(), J.tolist())] == [(a, b) for a, b, _ in want]
    assert sim.tobytes() == np.array([v for _, _, v in want], np.float64).tobytes()
    assert stats["pairs_kept"] == len(want) and stats["pairs_nominated"] >= len(want)


def test_semantic_duplicates_early_return_and_fallback():
    from anorag_hip import lexical_duplicates, semantic_duplicates
    assert semantic_duplicates([]) == [] and semantic_duplicates([{"note_id": "a", "content": "one note"}]) == []
    case = next(c for c in CASES if c["name"] == "empty_vocabulary_lexical_fallback")
    got = semantic_duplicates(copy.deepcopy(case["notes"]))
    assert got == ref.tuples(case["lexical"]["0.85"]) == lexical_duplicates(case["notes"])
    assert all(type(v) is float for _, _, v in got)


# ---- against the restatement
LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 300]


@pytest.mark.parametrize("n_rows", [0, 1, 2, 3, 65, 300])
def test_random_unit_rows_equal_the_restatement(n_rows):
    rng = np.random.default_rng(1000 + n_rows)
    lengths = [LENGTHS[k % len(LENGTHS)] for k in rng.permutation(max(n_rows, len(LENGTHS)))[:n_rows]]
    indptr, terms, values = ref.random_unit_rows(rng, lengths, 400)
    s, stats = check_against_ref(indptr, terms, values, 400, [0.05, 0.3, 0.6, 1.5])
    if n_rows >= 65:
        kept = np.count_nonzero(np.triu(s >= 0.3, 1))
        assert 0 < kept < n_rows * (n_rows - 1) // 2, "the threshold must separate the pairs of this input"


def two_rows_sharing(n_shared, rng, extra_rows=3):
    """rows 0 and 1 hold the same n_shared labels with slightly different weights; the others are unrelated"""
    n_terms = n_shared + 40
    base = rng.random(n_shared) + 0.5
    rows_t = [np.arange(n_shared), np.arange(n_shared)]
    rows_v = [base / np.sqrt(np.sum(base * base))]
    other = base * (1.0 + 0.01 * rng.random(n_shared))
    rows_v.append(other / np.sqrt(np.sum(other * other)) * (1.0 - 2.0 ** -30))
    for _ in range(extra_rows):
        t = np.sort(rng.choice(n_terms, 9, replace=False))
        v = rng.random(9) + 0.1
        rows_t.append(t)
        rows_v.append(v / np.sqrt(np.sum(v * v)))
    indptr = np.concatenate([[0], np.cumsum([len(t) for t in rows_t])]).astype(np.int64)
    return indptr, np.concatenate(rows_t).astype(np.int32), np.concatenate(rows_v), n_terms


def test_two_rows_sharing_2000_terms_of_tiny_weight():
    indptr, terms, values, n_terms = two_rows_sharing(2000, np.random.default_rng(7))
    s, _ = check_against_ref(indptr, terms, values, n_terms, [0.2, 0.9, 0.999])
    assert s[0, 1] > 0.999


def test_products_that_underflow():
    # rows 0..2 share label 0 with a large weight and labels 1..6 with 1e-160: those products are subnormal (1e-320) and 1
    # each in the integer bound; 1e-170 * 1e-300 is 0.0 and adds nothing to either.  Rows 3 and 4 share tiny weights only
    tiny = [1e-160] * 6
    rows = [([0, 1, 2, 3, 4, 5, 6], [0.9] + tiny), ([0, 1, 2, 3, 4, 5, 6], [0.8] + tiny), ([0, 2, 4, 6], [1.0, 1e-160, 1e-160, 1e-200]),
            ([1, 2, 3, 7], [1e-160, 1e-160, 1e-170, 0.5]), ([1, 2, 3, 8], [1e-160, 1e-160, 1e-300, 0.7])]
    indptr = np.concatenate([[0], np.cumsum([len(t) for t, _ in rows])]).astype(np.int64)
    terms = np.concatenate([t for t, _ in rows]).astype(np.int32)
    values = np.concatenate([v for _, v in rows]).astype(np.float64)
    s, stats = check_against_ref(indptr, terms, values, 9, [1e-300, 0.75, 0.5])
    assert 0.0 < s[3, 4] < 1e-300 and s[0, 1] == 0.9 * 0.8
    assert stats[2] == 3   # at 0.5 the bound nominates exactly the three pairs over label 0 (floor(0.5 * 2^30) > 6)


@pytest.mark.parametrize("n_shared", [1, 300])
def test_threshold_is_inclusive_and_the_bound_is_tight_enough(n_shared):
    indptr, terms, values, n_terms = two_rows_sharing(n_shared, np.random.default_rng(40 + n_shared), extra_rows=20)
    s = ref.pair_matrix(indptr, terms, values, n_terms)
    v = float(s[0, 1])
    assert 0.9 < v < 1.0
    raw = Raw(indptr, terms, values, n_terms)
    try:
        at, _ = raw.join(v)
        above, _ = raw.join(float(np.nextafter(v, 2.0)))
    finally:
        raw.close()
    same_arrays(at, ref.duplicates(s, v))
    assert (at[0][0], at[1][0]) == (0, 1) and at[2][0].tobytes() == np.float64(v).tobytes()
    same_arrays(above, tuple(a[1:] for a in at))     # the pair is gone, every other pair is unchanged
    # a low threshold lists the unrelated rows too: the same values again
    check_against_ref(indptr, terms, values, n_terms, [0.01])


@functools.lru_cache(maxsize=None)
def overflow_input():
    """300 rows that all hold label 0, with near-duplicate groups of 4 among them"""
    rng = np.random.default_rng(11)
    rows_t, rows_v = [], []
    for r in range(300):
        if r % 10 < 4 and r >= 10 and r % 10 > 0:      # rows 11-13, 21-23, ...: copies of the group's first row, perturbed
            t = rows_t[r - r % 10]
            v = rows_v[r - r % 10] * (1.0 + 0.05 * rng.random(len(t)))
        else:
            t = np.concatenate([[0], 1 + np.sort(rng.choice(500, 12, replace=False))])
            v = rng.random(13) + 0.2
            v[0] = 1.0   # label 0 alone gives every pair at least 1 / 18.3 > 0.05
        rows_t.append(t)
        rows_v.append(v / np.sqrt(np.sum(v * v)))
    indptr = np.concatenate([[0], np.cumsum([len(t) for t in rows_t])]).astype(np.int64)
    return indptr, np.concatenate(rows_t).astype(np.int32), np.concatenate(rows_v), 501


def test_overflow_passes_do_not_change_the_result():
    indptr, terms, values, n_terms = overflow_input()
    s = ref.pair_matrix(indptr, terms, values, n_terms)
    raw = Raw(indptr, terms, values, n_terms)
    try:
        for t in (0.9, 0.05):
            raw.slots(0)
            big, st_big = raw.join(t)
            raw.slots(64)
            small, st_small = raw.join(t)
            same_arrays(small, big)
            same_arrays(big, ref.duplicates(s, t))
            assert st_big[4] == 0 and st_big[5] == 4096 and st_small[4] > 0 and st_small[5] == 64
            assert st_small[1] == st_big[1] >= 300 * 299 // 2     # every pair shares label 0: each is walked once
        assert len(big[0]) == 300 * 299 // 2 and len(ref.duplicates(s, 0.9)[0]) == 29 * 6
    finally:
        raw.close()


def test_two_calls_are_byte_equal_and_bad_arguments_leave_the_handle_usable():
    indptr, terms, values, n_terms = overflow_input()
    raw = Raw(indptr, terms, values, n_terms)
    try:
        none = [np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float64)]
        assert raw.lib.anr_tfidf_self_join_fetch(raw.h, *[a.ctypes.data for a in none]) == ANR_ESTATE
        first, _ = raw.join(0.5)
        for bad in (0.0, -0.5, float("nan"), 2.0000001, float("inf")):
            rc, npairs, stats = raw.join_raw(bad)
            assert rc == ANR_EINVAL and npairs == -7 and np.all(stats == -7), bad
        for bad in (63, 96, 8192, -64):
            assert raw.lib.anr_tfidf_set_option(raw.h, 1, bad) == ANR_EINVAL
        assert raw.lib.anr_tfidf_set_option(raw.h, 2, 64) == ANR_EINVAL
        for name, args in BAD_CREATE.items():        # create's own refusals, with a device present
            rc, h = _create(raw.lib, *args)
            assert rc == ANR_EINVAL and not h.value, name
        rc, _ = raw.scores_raw([0, 1], [n_terms], [1.0])
        assert rc == ANR_EINVAL
        rc, _ = raw.scores_raw([0, 1], [0], [float("nan")])
        assert rc == ANR_EINVAL
        rc, _ = raw.scores_raw([0, 2, 1], [0, 1], [1.0, 1.0])
        assert rc == ANR_EINVAL
        second, _ = raw.join(0.5)
        same_arrays(second, first)
        assert len(first[0]) > 0
        rc, npairs, _ = raw.join_raw(2.0)            # legal, and nothing reaches it
        assert rc == 0 and npairs == 0
    finally:
        raw.close()


# ---- scores
@functools.lru_cache(maxsize=None)
def scores_input():
    """1000 documents; label k of 0..4 is held by the first (1, 63, 64, 65, 1000)[k] documents, so document 0 is in every
    posting; labels 5..64 are filler, label 65 is held by nobody"""
    rng = np.random.default_rng(5)
    reach = [1, 63, 64, 65, 1000]
    rows_t, rows_v = [], []
    for d in range(1000):
        t = [k for k in range(5) if d < reach[k]] + sorted((5 + rng.choice(60, 3, replace=False)).tolist())
        v = rng.random(len(t)) + 0.1
        rows_t.append(np.array(t))
        rows_v.append(v / np.sqrt(np.sum(v * v)))
    indptr = np.concatenate([[0], np.cumsum([len(t) for t in rows_t])]).astype(np.int64)
    return indptr, np.concatenate(rows_t).astype(np.int32), np.concatenate(rows_v), 66


@pytest.mark.parametrize("nq", [0, 1, 5])
def test_scores_equal_the_restatement(nq):
    indptr, terms, values, n_terms = scores_input()
    queries = [[0, 1, 2, 3, 4], [], [4, 7, 2, 30, 0, 3, 1], [65], [9, 4]][:nq]   # in the order given, also unsorted; 65: an empty posting
    rng = np.random.default_rng(50 + nq)
    q_indptr = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int64)
    q_terms = np.array([t for q in queries for t in q], np.int32)
    q_w = rng.random(len(q_terms)) + 0.1
    raw = Raw(indptr, terms, values, n_terms)
    try:
        rc, got = raw.scores_raw(q_indptr, q_terms, q_w)
        assert rc == 0, raw.L.last_error()
        rc, again = raw.scores_raw(q_indptr, q_terms, q_w)
        assert rc == 0
    finally:
        raw.close()
    want = ref.scores(indptr, terms, values, n_terms, q_indptr, q_terms, q_w)
    assert got.shape == (nq, 1000) and got.tobytes() == want.tobytes() and again.tobytes() == got.tobytes()
    if nq == 5:
        assert np.count_nonzero(got[0]) == 1000 and not got[1].any() and np.count_nonzero(got[3]) == 0


def test_scores_of_the_recorded_retriever_matrix_are_sklearns():
    from anorag_hip import TfidfJoin
    r = FILE["retriever"]
    with TfidfJoin(ref.Csr(r["csr"])) as join:
        got = join.scores(ref.Csr(r["query_csr"]))
        with pytest.raises(ValueError):
            join.scores(ref.Csr(dict(r["query_csr"], shape=[5, 3])))
    assert got.tobytes() == r["sims"].tobytes()


def test_bm25_search_is_the_same_with_the_device_key_on():
    from anorag_hip.compat import config
    from vector_store.retriever import VectorRetriever
    r = FILE["retriever"]

    def retriever():
        vr = object.__new__(VectorRetriever)   # the TF-IDF fallback alone: no encoder, no index
        vr.bm25_enabled, vr.tfidf_vectorizer, vr.tfidf_matrix, vr.tfidf_join = True, None, None, None
        vr.atomic_notes = copy.deepcopy(r["notes"])
        vr._build_bm25_index(vr.atomic_notes)
        assert vr.bm25_enabled
        return vr

    host = retriever()
    assert host.tfidf_join is None
    assert not config.get("anorag_hip.tfidf_device", False)   # off unless set
    config.set("anorag_hip.tfidf_device", True)
    try:
        dev = retriever()
    finally:
        config.set("anorag_hip.tfidf_device", False)
    assert dev.tfidf_join is not None
    assert dev.tfidf_matrix.shape == tuple(r["csr"]["shape"])
    for q in r["queries"]:
        a, b = host._bm25_search(q, r["top_k"]), dev._bm25_search(q, r["top_k"])
        assert a == b
        assert len(a) == (0 if q.startswith("zzz") else r["top_k"])
    dev._close_tfidf_join()
    assert dev.tfidf_join is None and dev._bm25_search(r["queries"][0], r["top_k"]) == host._bm25_search(r["queries"][0], r["top_k"])


# ---- the set loops
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_entity_and_lexical_duplicates_equal_the_reference(case):
    from anorag_hip import entity_duplicates, lexical_duplicates
    for t, rows in case["lexical"].items():
        got = lexical_duplicates(case["notes"], float(t))
        assert got == ref.tuples(rows) and all(type(v) is float for _, _, v in got)
    for t, rows in case["entity"].items():
        got = entity_duplicates(case["notes"], float(t))
        assert got == ref.tuples(rows) and all(type(v) is float for _, _, v in got)


def test_non_positive_jaccard_threshold_keeps_the_host_loop():
    from anorag_hip import entity_duplicates
    case = next(c for c in CASES if c["name"] == "notes_without_entities")
    got = entity_duplicates(case["notes"], 0.0)
    assert got == ref.entity_duplicates(case["notes"], 0.0)
    with_entities = sum(1 for n in case["notes"] if n.get("entities"))
    assert len(got) == with_entities * (with_entities - 1) // 2   # notes with empty sets are skipped, every other pair passes
