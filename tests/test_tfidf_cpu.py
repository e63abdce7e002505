"""CPU tests (no GPU needed) of the TF-IDF join's host half: the restatement (tests/tfidf_ref.py) against what the
reference returned (tests/golden/dedup_cases.npz) bit for bit, anorag_hip.note_dedup's normalisation, relabelling and
host-side merge of the three duplicate lists, and the argument checks of the C ABI, which come before any device work."""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import tfidf_ref as ref

FILE = ref.load_file()
CASES = FILE["cases"]
WITH_CSR = [c for c in CASES if c["csr"] is not None]
ANR_EINVAL, ANR_EHIP = -1, -2


def ids(cases):
    return [c["name"] for c in cases]


@pytest.mark.parametrize("case", WITH_CSR, ids=ids(WITH_CSR))
def test_restatement_equals_sklearn_values(case):
    want = ref.tuples(case["expected"]["semantic_duplicates"])
    got = ref.semantic_from_csr(case)
    assert got == want
    assert [np.float64(v).tobytes() for _, _, v in got] == [np.float64(v).tobytes() for _, _, v in want]


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_restated_set_loops_equal_the_reference(case):
    for t, rows in case["lexical"].items():
        assert ref.lexical_duplicates(case["notes"], float(t)) == ref.tuples(rows)
    for t, rows in case["entity"].items():
        assert ref.entity_duplicates(case["notes"], float(t)) == ref.tuples(rows)
    assert ref.tuples(case["expected"]["entity_duplicates"]) == ref.tuples(case["entity"]["0.8"])


@pytest.mark.parametrize("case", WITH_CSR + [FILE["retriever"]], ids=ids(WITH_CSR) + ["retriever"])
def test_host_half_on_recorded_matrices(case):
    from anorag_hip import note_dedup as nd
    m = ref.Csr(case["csr"])
    # sklearn stores the rows unsorted by column id: a sorted matrix here would mean the recording lost the stored order
    assert any(np.any(np.diff(m.indices[a:b]) < 0) for a, b in zip(m.indptr[:-1], m.indptr[1:]))
    terms, label = nd.relabel_terms(m)
    want_terms, want_label = ref.relabel(m.indptr, m.indices, m.shape[1])
    assert terms.dtype == np.int32 and np.array_equal(terms, want_terms) and np.array_equal(label, want_label)
    assert sorted(label.tolist()) == list(range(m.shape[1]))
    for a, b in zip(m.indptr[:-1], m.indptr[1:]):
        assert np.all(np.diff(terms[a:b].astype(np.int64)) > 0)
    assert nd.normalize_rows(m.indptr, m.data).tobytes() == ref.normalize(m.indptr, m.data).tobytes()


def test_relabel_refuses_rows_without_a_global_order():
    from anorag_hip import note_dedup as nd
    ok = SimpleNamespace(format="csr", shape=(3, 4), indptr=np.array([0, 2, 4, 5]), indices=np.array([3, 1, 3, 0, 1]),
                         data=np.ones(5))
    terms, label = nd.relabel_terms(ok)          # first seen: 3, 1, then 0; column 2 is never seen
    assert label.tolist() == [2, 1, 3, 0] and terms.tolist() == [0, 1, 0, 2, 1]
    bad = SimpleNamespace(format="csr", shape=(2, 4), indptr=np.array([0, 2, 4]), indices=np.array([3, 1, 1, 3]),
                          data=np.ones(4))       # row 0 holds 3 before 1, row 1 holds 1 before 3
    with pytest.raises(ValueError, match="row 1"):
        nd.relabel_terms(bad)
    twice = SimpleNamespace(format="csr", shape=(1, 4), indptr=np.array([0, 2]), indices=np.array([2, 2]), data=np.ones(2))
    with pytest.raises(ValueError):
        nd.relabel_terms(twice)
    with pytest.raises(ValueError):
        nd.relabel_terms(SimpleNamespace(format="csr", shape=(1, 2), indptr=np.array([0, 1]), indices=np.array([2]),
                                         data=np.ones(1)))
    with pytest.raises(ValueError, match="float64"):
        nd.relabel_terms(SimpleNamespace(format="csr", shape=(1, 2), indptr=np.array([0, 1]), indices=np.array([1]),
                                         data=np.ones(1, np.float32)))


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_host_merge_of_recorded_lists_gives_the_reference_dict(case):
    """exact_duplicates, merge_duplicate_results and deduplicate_notes are host code: fed the recorded semantic and entity
    lists they must rebuild every other field of the reference's dict"""
    from anorag_hip import note_dedup as nd
    want = ref.load_expected(case)
    notes = copy.deepcopy(case["notes"])
    exact = nd.exact_duplicates(notes)
    assert exact == want["exact_duplicates"] and list(exact) == list(want["exact_duplicates"])
    merged = nd.merge_duplicate_results(exact, ref.tuples(want["semantic_duplicates"]), ref.tuples(want["entity_duplicates"]))
    kept = nd.deduplicate_notes(notes, merged)
    removed = sum(len(v) for v in merged.values())
    assert removed == want["removed_count"] and len(kept) == want["remaining_count"]
    assert removed / max(len(notes), 1) == want["duplicate_rate"]
    got = dict(want, deduplicated_notes=kept)
    ref.same_result(got, want)


def test_restated_scores_equal_sklearn():
    r = FILE["retriever"]
    m, q = ref.Csr(r["csr"]), ref.Csr(r["query_csr"])
    terms, label = ref.relabel(m.indptr, m.indices, m.shape[1])
    got = ref.scores(m.indptr, terms, ref.normalize(m.indptr, m.data), m.shape[1], q.indptr, label[q.indices],
                     ref.normalize(q.indptr, q.data))
    assert got.tobytes() == r["sims"].tobytes()


def _create(lib, n_rows, n_terms, indptr, terms, values):
    h = C.c_void_p()
    indptr = np.ascontiguousarray(indptr, np.int64)
    terms = np.ascontiguousarray(terms, np.int32)
    values = np.ascontiguousarray(values, np.float64)
    rc = lib.anr_tfidf_create(0, n_rows, n_terms, indptr.ctypes.data, terms.ctypes.data, values.ctypes.data, C.byref(h))
    return rc, h


BAD_CREATE = {
    "descending labels": (2, 4, [0, 2, 3], [2, 1, 0], [0.6, 0.8, 1.0]),
    "repeated label": (1, 4, [0, 2], [1, 1], [0.6, 0.8]),
    "label too large": (1, 4, [0, 1], [4], [1.0]),
    "negative label": (1, 4, [0, 1], [-1], [1.0]),
    "nan value": (1, 4, [0, 1], [0], [np.nan]),
    "infinite value": (1, 4, [0, 1], [0], [np.inf]),
    "negative value": (1, 4, [0, 2], [0, 1], [-0.6, 0.8]),
    "row longer than a unit": (1, 4, [0, 2], [0, 1], [0.8, 0.7]),
    "row a little longer than a unit": (1, 4, [0, 1], [0], [1.0 + 2.0 ** -20]),
    "indptr descends": (2, 4, [0, 1, 0], [0], [1.0]),
    "indptr not from 0": (1, 4, [1, 2], [0, 1], [1.0, 1.0]),
    "too many rows": (2 ** 31 - 1, 4, [0], [], []),
    "too many terms": (0, 2 ** 31 - 1, [0], [], []),
}


@pytest.mark.parametrize("name", list(BAD_CREATE))
def test_create_checks_its_arguments_before_any_device_work(name):
    from anorag_hip import _lib
    lib = _lib.load()
    rc, h = _create(lib, *BAD_CREATE[name])
    assert rc == ANR_EINVAL and not h.value, (name, rc, _lib.last_error())
    assert _lib.last_error()


def test_create_accepts_what_is_legal_and_null_handles_are_refused():
    from anorag_hip import _lib
    lib = _lib.load()
    # a unit row, a row just inside the slack (sum of squares 1 + 2^-21 + 2^-44), an all-zero row and an empty row
    rc, h = _create(lib, 4, 4, [0, 2, 3, 4, 4], [0, 1, 3, 2], [0.6, 0.8, 1.0 + 2.0 ** -22, 0.0])
    if _lib.device_count() > 0:
        assert rc == 0, _lib.last_error()
        assert lib.anr_tfidf_destroy(h) == 0
    else:
        assert rc == ANR_EHIP and "no HIP device" in _lib.last_error()
        from anorag_hip import AnoragError, TfidfJoin
        with pytest.raises(AnoragError, match="no HIP device"):   # no quiet host path
            TfidfJoin(ref.Csr(WITH_CSR[0]["csr"]))
    assert lib.anr_tfidf_create(0, 0, 0, None, None, None, None) == ANR_EINVAL
    assert lib.anr_tfidf_self_join(None, 0.85, None, None) == ANR_EINVAL
    assert lib.anr_tfidf_self_join_fetch(None, None, None, None) == ANR_EINVAL
    assert lib.anr_tfidf_scores(None, 0, None, None, None, None) == ANR_EINVAL
    assert lib.anr_tfidf_set_option(None, 1, 64) == ANR_EINVAL
    assert lib.anr_tfidf_destroy(None) == 0
