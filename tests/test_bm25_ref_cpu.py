"""CPU tests (no GPU needed): the exact-order BM25 reference of tests/bm25_ref.py is checked against oracle/bm25.py before
tests/test_bm25_paths_gpu.py lets it judge the device; the synthetic query batch reaches what it is meant to reach; and
anr_bm25_create refuses malformed postings before it opens a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bm25_ref as br
from oracle import bm25 as obm


def test_reference_equals_the_oracle_on_a_random_corpus():
    rng = np.random.default_rng(11)
    vocab = [f"w{i}" for i in range(120)]
    probs = 1.0 / np.arange(1, 121)
    probs /= probs.sum()
    notes = [{"title": "", "content": " ".join(rng.choice(vocab, size=rng.integers(0, 40), p=probs))} for _ in range(300)]
    text = lambda n: f"{n.get('title', '')} {n.get('content', '')}"
    orc = obm.build_bm25_corpus(notes, text)
    voc, post = br.corpus_postings([obm.tokenize_text(text(n)) if text(n) else [] for n in notes])
    assert post.n_docs == 300 and post.n_terms == len(voc) > 50
    queries = [" ".join(rng.choice(vocab, size=rng.integers(1, 9), p=probs)) for _ in range(30)]
    queries += ["w0 w0 w1 w0", "zzz", "w3 zzz w3", "w119 w118 w117 w0 w1 w2 w3 w4 w5 w6 w7 w8"]
    for q in queries:
        toks = obm.tokenize_text(q)
        ids = br.encode_query(voc, toks)
        raw, raw_max = post.scores(ids, 0)
        assert raw.tolist() == orc.get_scores(toks)                       # bit for bit
        assert raw_max == max(raw.tolist())
        norm, norm_max = post.scores(ids, 1)
        assert norm.tolist() == obm.bm25_scores(orc, notes, q)
        assert norm_max == (1.0 if raw_max > 0 else raw_max) and norm_max == max(norm.tolist())
        for normalize in (0, 1):                                           # the sparse form of the same reference
            t, v, m = post.sparse_scores(ids, normalize)
            row, mx = post.scores(ids, normalize)
            assert t.tolist() == post.touched(ids).tolist() and v.tolist() == row[t].tolist() and m == mx
            assert np.count_nonzero(row) == np.count_nonzero(v)


def test_reference_adds_in_query_order():
    """a document under three terms with weights 1e16, 1.0, -1e16: 0.0 in that order (1e16 + 1.0 rounds back to 1e16),
    1.0 in the order 1e16, -1e16, 1.0"""
    post = br.Postings(3, [0, 1, 2, 3], [1, 1, 1], [1e16, 1.0, -1e16])
    assert post.scores([0, 1, 2], 0)[0].tolist() == [0.0, 0.0, 0.0]
    assert post.scores([0, 1, 2], 0)[1] == 0.0
    assert post.scores([0, 2, 1], 0)[0].tolist() == [0.0, 1.0, 0.0]
    two = br.Postings(3, [0, 1, 2, 3, 4], [1, 1, 1, 2], [1e16, 1.0, -1e16, 4.0])
    assert two.scores([0, 2, 1, 3], 1)[0].tolist() == [0.0, 0.25, 1.0] and two.scores([0, 2, 1, 3], 1)[1] == 1.0
    assert two.scores([0, 2, 1, 3], 0)[1] == 4.0
    assert post.sparse_scores([0, 1, 2], 0)[1].tolist() == [0.0] and post.sparse_scores([0, 2, 1], 0)[1].tolist() == [1.0]
    assert post.touched([0, 1, 2]).tolist() == [1]                        # touched, although its sum is exactly 0.0
    # the maximum: 0.0 when a document stayed untouched and every touched one is negative; no division then
    neg = br.Postings(3, [0, 2], [0, 2], [-2.0, -4.0])
    assert neg.scores([0], 1)[0].tolist() == [-2.0, 0.0, -4.0] and neg.scores([0], 1)[1] == 0.0
    allneg = br.Postings(2, [0, 2], [0, 1], [-2.0, -4.0])
    assert allneg.scores([0], 1)[0].tolist() == [-2.0, -4.0] and allneg.scores([0], 1)[1] == -2.0
    assert allneg.sparse_scores([0], 1)[2] == -2.0 and neg.sparse_scores([0], 1)[2] == 0.0
    # combine: t = 0.0; t += w_f * row_f in field order
    rows = [np.array([1e16, 1.0]), np.array([1.0, 1.0]), np.array([1e16, -1.0])]
    assert br.combine(rows, [1.0, 1.0, -1.0], 0)[0].tolist() == [0.0, 3.0]
    swapped = [rows[0], rows[2], rows[1]]
    assert br.combine(swapped, [1.0, -1.0, 1.0], 0)[0].tolist() == [1.0, 3.0] and br.combine(swapped, [1.0, -1.0, 1.0], 0)[1] == 3.0
    assert br.combine(swapped, [1.0, -1.0, 1.0], 1)[0].tolist() == [1.0 / 3.0, 1.0] and br.combine(swapped, [1.0, -1.0, 1.0], 1)[1] == 1.0
    assert br.combine([np.array([-1.0, -3.0])], [2.0], 1)[0].tolist() == [-2.0, -6.0]
    assert br.combine([np.array([-1.0, -3.0])], [2.0], 1)[1] == -2.0


@pytest.mark.parametrize("name", list(br.HANDLES))
def test_synthetic_batch_reaches_what_it_is_meant_to(name):
    """preconditions of tests/test_bm25_paths_gpu.py, checked where no device is needed"""
    pos, neg = br.handle_postings(name, "pos"), br.handle_postings(name, "neg")
    n = pos.n_docs
    assert pos.docs.tobytes() == neg.docs.tobytes() and np.array_equal(np.abs(pos.weights), np.abs(neg.weights))
    mags = np.abs(pos.weights[np.abs(pos.weights) < 1e15])
    assert mags.min() < 2.0 ** -28 and mags.max() > 2.0 ** 28 and np.all(pos.weights[np.abs(pos.weights) != 1e16] > 0)
    for t in range(pos.n_terms):                                           # what anr_bm25_create demands
        d = pos.docs[pos.indptr[t]:pos.indptr[t + 1]]
        assert np.all(np.diff(d) > 0) and (len(d) == 0 or (d[0] >= 0 and d[-1] < n))
    for tn in br.NEGATIVE_TERMS:
        assert np.all(neg.weights[neg.indptr[neg.term[tn]]:neg.indptr[neg.term[tn] + 1]] < 0)
    lens = np.diff(pos.indptr)[pos.short]
    assert lens.min() == 1 and lens.max() == 64 and len(lens) == 1200
    batch = dict(br.query_batch(pos))
    names = [k for k, _ in br.query_batch(pos)]
    assert names[0] == "empty_first" and names[-1] == "empty_last" and "empty_middle" in names[5:-5]
    assert [dict(br.query_batch(neg))[k] for k in names] == [batch[k] for k in names]
    assert len(batch["short513"]) == 513 and len(batch["short1100"]) == 1100 and len(batch["short600_L1025"]) == 601
    assert len(set(batch["short1100"])) <= 150
    # the touched-documents division across token blocks: fewer postings than documents, on every handle
    assert pos.posting_sum(batch["short600_L1025"]) < n
    assert len(pos.touched(batch["short513"])) < pos.posting_sum(batch["short513"])     # overlaps: first occurrences matter
    # LOW twice: as many postings as documents, half the corpus untouched -> maximum 0.0 on the negative handle
    assert pos.posting_sum(batch["LOW_LOW"]) >= n and len(pos.touched(batch["LOW_LOW"])) == n // 2
    for k in ("ALL", "LOW_LOW", "EVEN_ODD"):
        row, m = neg.scores(batch[k], 1)
        assert m == (0.0 if k == "LOW_LOW" else row.max()) and m <= 0.0 and row.min() < 0.0
        assert row.tobytes() == neg.scores(batch[k], 0)[0].tobytes()      # no division
    assert pos.scores(batch["ORD_abc"], 0)[0].tobytes() != pos.scores(batch["ORD_acb"], 0)[0].tobytes()
    # sparse rows: which are refused, and why
    for post in (pos, neg):
        for cap in (6144, 7168, 65536):
            why = [post.sparse_refusal(q, cap) for q in batch.values()]
            assert sum(w is None for w in why) * 4 >= 3 * len(why)
            if cap > 6144:
                held = {k for k, w in zip(batch, why) if w is None}
                assert {"short513", "short1100", "short600_L1025"} <= held
            if name == "C" and cap == 7168:
                assert {"sum", "slice", "count"} <= set(why)
                assert post.sparse_refusal(batch["RUN4500"], cap) == "slice" and post.sparse_refusal(batch["L9000"], cap) == "count"
            if name == "B" and cap <= 7168:
                assert "count" in why


def _code(name):
    """an error code of include/anorag.h (anorag_hip._lib names only ANR_OK)"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "anorag.h")) as f:
        return int(re.search(r"#define\s+%s\s+\((-?\d+)\)" % name, f.read()).group(1))


_EINVAL, _EHIP = _code("ANR_EINVAL"), _code("ANR_EHIP")


def _create(n_docs, indptr, docs, weights=None, out=True):
    from anorag_hip import _lib
    lib = _lib.load()
    indptr = np.asarray(indptr, dtype=np.int64)
    docs = np.asarray(docs, dtype=np.int32)
    weights = np.ones(max(len(docs), 1), dtype=np.float64) if weights is None else weights
    h = C.c_void_p(0xdead0)     # must come back NULL
    rc = lib.anr_bm25_create(0, n_docs, len(indptr) - 1, indptr.ctypes.data, docs.ctypes.data if len(docs) else None,
                             weights.ctypes.data, C.byref(h) if out else None)
    return rc, h.value, lib.anr_last_error()


@pytest.mark.parametrize("what,says,n_docs,indptr,docs", [
    ("indptr[0] != 0", b"CSR", 10, [1, 2, 3], [0, 1, 2]),
    ("decreasing indptr", b"non-decreasing", 10, [0, 3, 2, 4], [0, 1, 2, 3]),
    ("document id below 0", b"out of range", 10, [0, 2, 3], [-1, 4, 5]),
    ("document id == n_docs", b"out of range", 10, [0, 2, 3], [3, 10, 5]),
    ("document id above n_docs", b"out of range", 10, [0, 2, 3], [3, 4, 11]),
    ("equal ids inside a list", b"ascending", 10, [0, 1, 4], [9, 2, 5, 5]),
    ("descending ids inside a list", b"ascending", 10, [0, 1, 4], [9, 2, 7, 6]),
    ("n_docs > 2^31 - 1", b"2^31", 2 ** 31, [0, 2, 3], [0, 1, 2]),
])
def test_bm25_create_refuses_malformed_postings_before_any_device_work(what, says, n_docs, indptr, docs):
    rc, h, msg = _create(n_docs, indptr, docs)
    assert rc == _EINVAL and h is None and says in msg, (what, msg)   # refused, and by the intended branch


def test_bm25_create_refuses_a_null_out_pointer():
    rc, _, msg = _create(10, [0, 2, 3], [0, 1, 2], out=False)
    assert rc == _EINVAL and b"out" in msg


def test_bm25_create_validation_does_not_refuse_well_formed_postings():
    """the same shapes, well formed, pass the validation: the call goes on to look for a device (ANR_EHIP without one,
    a handle with one) — so the refusals above are about the malformation, not about the call"""
    from anorag_hip import _lib
    rc, h, _ = _create(10, [0, 2, 3, 3], [3, 9, 0])   # ascending inside each list only; an empty list; id n_docs - 1
    if _lib.device_count() > 0:
        assert rc == _lib.ANR_OK and h
        assert _lib.load().anr_bm25_destroy(C.c_void_p(h)) == 0
    else:
        assert rc == _EHIP and h is None
