"""Exact-order reference of the device BM25 (csrc/bm25.hip) on raw CSR postings, and the synthetic postings and query
batch tests/test_bm25_paths_gpu.py uses.  Plain Python + numpy, no device: test infrastructure only.

The device's contract is "bit-identical float64": every document receives the posting weights of the query's tokens in
query-token order, one addition at a time.  ``Postings.scores`` does exactly that and nothing cleverer, so that a kernel
which adds in another order, divides twice or takes the maximum over the wrong set disagrees with it in the last bit.
tests/test_bm25_ref_cpu.py checks this file against oracle/bm25.py before it judges the device; the device tests
in turn hold sparse_refusal against what anr_bm25_sparse_dev refuses.
"""
from __future__ import annotations

import math
from collections import Counter
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# limits of anr_bm25_sparse_dev (include/anorag.h; kSpMaxCap, kSrSlice, kSrWidth, kSrTarget, kSrMaxSlices of csrc/bm25.hip)
HASH_CAP = 6144        # rows up to this many documents live in one LDS hash table
SLICE_DOCS = 4096      # touched documents one slice holds
SLICE_WIDTH = 131072   # ids one slice may span
SLICE_TARGET = 2048    # postings per slice the host aims at
MAX_SLICES = 1024      # slices per query


class Postings:
    """CSR postings (n_docs, indptr, docs, weights) with the reference scoring on them."""

    def __init__(self, n_docs: int, indptr, docs, weights, term: Optional[Dict[str, int]] = None):
        self.n_docs = int(n_docs)
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        self.docs = np.ascontiguousarray(docs, dtype=np.int32)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.n_terms = len(self.indptr) - 1
        self.term = dict(term or {})   # name -> term id (the synthetic postings)
        self.short: List[int] = []     # term ids of SHORT_0 .. (the synthetic postings)
        self.short_lengths = np.zeros(0, dtype=np.int64)   # their list lengths (the synthetic postings)
        self.edge_bounds: Tuple[int, ...] = ()             # range bounds b with a term EDGE_b = {b - 1, b}

    def _list(self, t: int):
        lo, hi = int(self.indptr[t]), int(self.indptr[t + 1])
        return self.docs[lo:hi], self.weights[lo:hi]

    def posting_sum(self, query: Sequence[int]) -> int:
        return int(sum(int(self.indptr[t + 1] - self.indptr[t]) for t in query))

    @staticmethod
    def _normalise(row: np.ndarray, n_docs: int, normalize) -> Tuple[np.ndarray, float]:
        """bm25_scores' rule: divide by the maximum over ALL n_docs scores when it is > 0.  Second value: what the device
        reports as the maximum of its OUTPUT row — 1.0 when it divided (m / m), the maximum itself otherwise."""
        m = float(row.max()) if n_docs > 0 and len(row) else 0.0
        if normalize and m > 0.0:
            return row / m, 1.0
        return row, m

    def scores(self, query: Sequence[int], normalize) -> Tuple[np.ndarray, float]:
        row = np.zeros(self.n_docs, dtype=np.float64)
        for t in query:                      # query order, with repetition
            d, w = self._list(t)
            np.add.at(row, d, w)             # one addition per posting; a list holds a document once
        return self._normalise(row, self.n_docs, normalize)

    def touched(self, query: Sequence[int]) -> np.ndarray:
        """sorted ids of the documents in any of the query's lists: the ids of a sparse row (sums of exactly 0.0 included)"""
        if not len(query):
            return np.zeros(0, dtype=np.int64)
        return np.unique(np.concatenate([self._list(t)[0] for t in query])).astype(np.int64)

    def sparse_scores(self, query: Sequence[int], normalize) -> Tuple[np.ndarray, np.ndarray, float]:
        """(touched ids, their scores, reported maximum) without forming the n_docs-vector: the same additions in the same
        order on a vector indexed by the rank of the document among the touched ones"""
        ids = self.touched(query)
        vals = np.zeros(len(ids), dtype=np.float64)
        for t in query:
            d, w = self._list(t)
            np.add.at(vals, np.searchsorted(ids, d), w)
        m = float(vals.max()) if len(ids) else 0.0
        if len(ids) < self.n_docs:
            m = max(m, 0.0)                  # an untouched document kept its 0.0
        if normalize and m > 0.0:
            return ids, vals / m, 1.0
        return ids, vals, m

    def sparse_refusal(self, query: Sequence[int], cap: int) -> Optional[str]:
        """why anr_bm25_sparse_dev cannot hold the row at this cap (count -1), or None.  cap <= 6144: more than cap touched
        documents.  Beyond (sparse_sliced): a posting sum above 4 cap; else, with the row cut into
        R = min(1024, max(ceil(n_docs / 131072), ceil(sum / 2048))) document ranges [n_docs r / R, n_docs (r + 1) / R), a
        range with more than 4096 touched documents; else more than cap touched documents."""
        ids = self.touched(query)
        if cap <= HASH_CAP:
            return "count" if len(ids) > cap else None
        s = self.posting_sum(query)
        if s > 4 * cap:
            return "sum"
        R = min(MAX_SLICES, max(max(1, -(-self.n_docs // SLICE_WIDTH)), -(-s // SLICE_TARGET)))
        bounds = np.array([self.n_docs * r // R for r in range(R + 1)], dtype=np.int64)
        if np.diff(np.searchsorted(ids, bounds)).max(initial=0) > SLICE_DOCS:
            return "slice"
        return "count" if len(ids) > cap else None


def combine(field_rows: Sequence[np.ndarray], weights: Sequence[float], normalize) -> Tuple[np.ndarray, float]:
    """FieldWeightedBM25.get_scores: t = 0.0; t += w_f * row_f in field order; then bm25_scores' normalisation"""
    t = np.zeros(len(field_rows[0]), dtype=np.float64)
    for w, row in zip(weights, field_rows):
        t = t + float(w) * np.asarray(row, dtype=np.float64)
    return Postings._normalise(t, len(t), normalize)


def corpus_postings(corpus: List[List[str]], k1: float = 1.5, b: float = 0.75):
    """(vocab, Postings) of a tokenised corpus, computed as anorag_hip.bm25_search.DeviceBM25.__init__ computes them:
    terms numbered by first appearance, documents ascending inside a list, the weight of a posting by the reference's
    expression operation by operation in float64"""
    doc_len = [len(d) for d in corpus]
    doc_count = len(corpus)
    avgdl = sum(doc_len) / len(doc_len) if doc_len else 0
    vocab: Dict[str, int] = {}
    post_doc: List[List[int]] = []
    post_tf: List[List[int]] = []
    for di, doc in enumerate(corpus):
        for term, tf in Counter(doc).items():
            ti = vocab.get(term)
            if ti is None:
                ti = len(post_doc)
                vocab[term] = ti
                post_doc.append([])
                post_tf.append([])
            post_doc[ti].append(di)
            post_tf[ti].append(tf)
    n_terms = len(post_doc)
    idf = np.empty(n_terms, dtype=np.float64)
    indptr = np.zeros(n_terms + 1, dtype=np.int64)
    for ti in range(n_terms):
        n = len(post_doc[ti])
        idf[ti] = math.log((doc_count - n + 0.5) / (n + 0.5) + 1.0)
        indptr[ti + 1] = indptr[ti] + n
    docs = np.fromiter((d for lst in post_doc for d in lst), dtype=np.int32, count=int(indptr[-1]))
    tf = np.fromiter((t for lst in post_tf for t in lst), dtype=np.float64, count=int(indptr[-1]))
    if len(docs):
        dl = np.asarray(doc_len, dtype=np.float64)[docs]
        term_of = np.repeat(np.arange(n_terms), np.diff(indptr))
        numerator = tf * (k1 + 1)
        denominator = tf + k1 * (1 - b + b * (dl / avgdl))
        weights = idf[term_of] * (numerator / denominator)
    else:
        weights = np.zeros(0, dtype=np.float64)
    return vocab, Postings(doc_count, indptr, docs, weights)


def encode_query(vocab: Dict[str, int], tokens: Sequence[str]) -> List[int]:
    """DeviceBM25._encode_queries: a token no document holds is omitted"""
    return [vocab[t] for t in tokens if t in vocab]


# ---- synthetic postings ---------------------------------------------------------------------------------------------
N_SHORT = 1200
ORD_WEIGHTS = {"ORD_a": 1e16, "ORD_b": 1.0, "ORD_c": -1e16}
NEGATIVE_TERMS = ("LOW", "ALL", "EVEN", "ODD")


def synthetic_postings(n_docs: int, variant: str, edge_bounds: Sequence[int] = (), seed: int = 20240607) -> Postings:
    """The postings of tests/test_bm25_paths_gpu.py, deterministic in (n_docs, variant, edge_bounds, seed).

    Weights: +-2^k with k uniform in [-30, 30] times a mantissa in [1, 2) — sums whose last bits depend on the order of
    the additions.  variant "pos": the same magnitudes, every weight positive.  variant "neg": every weight of LOW, ALL,
    EVEN and ODD negative, random signs elsewhere.  ORD_a / ORD_b / ORD_c carry 1e16 / 1.0 / -1e16 in both.

    Terms: ALL, EVEN, ODD, LOW (the first n_docs // 2 documents), ONE_0, ONE_LAST, EDGE_<b> = {b - 1, b} for every b of
    edge_bounds, L1025 / L2047 / ORD_* (1500) random documents, EMPTY, RUN4500 (documents 0 .. 4499: more than one slice of
    a sparse row holds when the slices are wide), L9000 (n_docs >= 12000 only: more than a cap-7168 row holds), and 1200
    SHORT_i of 1 to 64 documents drawn from 4000 "hot" documents so that they overlap."""
    assert variant in ("pos", "neg") and n_docs >= 4600
    rng = np.random.default_rng(seed)
    lists: List[Tuple[str, np.ndarray]] = []

    def rand(k):
        return np.sort(rng.choice(n_docs, size=k, replace=False))

    lists.append(("ALL", np.arange(n_docs)))
    lists.append(("ONE_0", np.array([0])))
    lists.append(("EVEN", np.arange(0, n_docs, 2)))
    lists.append(("EMPTY", np.zeros(0, dtype=np.int64)))
    lists.append(("ODD", np.arange(1, n_docs, 2)))
    lists.append(("L1025", rand(1025)))
    lists.append(("LOW", np.arange(n_docs // 2)))
    lists.append(("ONE_LAST", np.array([n_docs - 1])))
    lists.append(("L2047", rand(2047)))
    ord_docs = rand(1500)
    for name in ORD_WEIGHTS:
        lists.append((name, ord_docs))
    for b in edge_bounds:
        assert 0 < b < n_docs
        lists.append((f"EDGE_{b}", np.array([b - 1, b])))
    lists.append(("RUN4500", np.arange(4500)))
    if n_docs >= 12000:
        lists.append(("L9000", rand(9000)))
    # the SHORT terms: lengths independent of n_docs (skewed to short lists), documents from a hot set
    lrng = np.random.default_rng(seed + 1)
    lengths = np.minimum(64, 1 + np.floor(64.0 * lrng.random(N_SHORT) ** 3).astype(np.int64))
    hot = rand(min(n_docs, 4000))
    for i in range(N_SHORT):
        lists.append((f"SHORT_{i}", np.sort(rng.choice(hot, size=int(lengths[i]), replace=False))))

    term = {name: i for i, (name, _) in enumerate(lists)}
    indptr = np.zeros(len(lists) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(d) for _, d in lists])
    docs = np.concatenate([d for _, d in lists]).astype(np.int32)
    nnz = int(indptr[-1])
    mag = np.ldexp(1.0 + rng.random(nnz), rng.integers(-30, 31, size=nnz))
    sign = np.where(rng.random(nnz) < 0.5, -1.0, 1.0)
    weights = mag.copy() if variant == "pos" else sign * mag
    for name, w in ORD_WEIGHTS.items():
        weights[indptr[term[name]]:indptr[term[name] + 1]] = w
    if variant == "neg":
        for name in NEGATIVE_TERMS:
            sl = slice(int(indptr[term[name]]), int(indptr[term[name] + 1]))
            weights[sl] = -mag[sl]
    post = Postings(n_docs, indptr, docs, weights, term)
    post.short = [term[f"SHORT_{i}"] for i in range(N_SHORT)]
    post.short_lengths = lengths
    post.edge_bounds = tuple(edge_bounds)
    return post


def query_batch(post: Postings, seed: int = 977) -> List[Tuple[str, List[int]]]:
    """(name, term ids) of the batch every handle is asked: the same content whatever the handle (the EDGE queries follow
    the handle's bounds), the empty query first, in the middle and last"""
    t = post.term
    rng = np.random.default_rng(seed)
    sh = np.asarray(post.short)
    q513 = sh[rng.choice(N_SHORT, size=513, replace=False)].tolist()
    pool = rng.choice(N_SHORT, size=150, replace=False)
    q1100 = sh[pool[rng.integers(0, 150, size=1100)]].tolist()
    shortest = np.argsort(post.short_lengths, kind="stable")[:600]
    q600 = sh[rng.permutation(shortest)].tolist() + [t["L1025"]]
    out: List[Tuple[str, List[int]]] = [("empty_first", []), ("EMPTY", [t["EMPTY"]]), ("ONE_0", [t["ONE_0"]]),
                                        ("ONE_LAST", [t["ONE_LAST"]])]
    out += [(f"EDGE_{b}", [t[f"EDGE_{b}"]]) for b in post.edge_bounds]
    out += [("ONE_LAST_ONE_0", [t["ONE_LAST"], t["ONE_0"]]), ("L2047", [t["L2047"]])]
    out += [("L1025", [t["L1025"]]), ("L2047_L1025", [t["L2047"], t["L1025"]]), ("EVENx3", [t["EVEN"]] * 3),
            ("ALL", [t["ALL"]]), ("empty_middle", []), ("EVEN_ODD", [t["EVEN"], t["ODD"]]), ("LOW_LOW", [t["LOW"]] * 2),
            ("ORD_abc", [t["ORD_a"], t["ORD_b"], t["ORD_c"]]), ("ORD_acb", [t["ORD_a"], t["ORD_c"], t["ORD_b"]]),
            ("ALL_L2047_ALL", [t["ALL"], t["L2047"], t["ALL"]]), ("short513", q513), ("short1100", q1100),
            ("short600_L1025", q600), ("RUN4500", [t["RUN4500"]])]
    if "L9000" in t:
        out.append(("L9000", [t["L9000"]]))
    out.append(("empty_last", []))
    return out


def csr_queries(queries: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """(q_indptr int64 [nq + 1], q_terms int32) of the C ABI"""
    indptr = np.zeros(len(queries) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(q) for q in queries])
    terms = np.asarray([x for q in queries for x in q], dtype=np.int32)
    if terms.size == 0:
        terms = np.zeros(1, dtype=np.int32)   # (a valid pointer; no entry is read)
    return indptr, terms


# the handles of tests/test_bm25_paths_gpu.py.  With n_cu = 256 compute units score_chunk picks
#   R = min(32, max(1, ceil(1024 / nq))), then R = max(1, n_docs // 4096) when n_docs < 4096 R;  R <= 1: k_bm25.
HANDLES = {
    # 5000 < 2 * 4096 -> R = 5000 // 4096 = 1 for every nq: the single-workgroup kernel
    "A": dict(n_docs=5000, edge_bounds=()),
    # nq <= 341: ceil(1024 / nq) >= 4 and 12290 < 4 * 4096 -> R = 12290 // 4096 = 3, bounds 12290 r // 3 = 4096, 8193;
    # nq = 400: ceil(1024 / 400) = 3 and 12290 >= 3 * 4096 -> R = 3;  nq = 512: ceil(1024 / 512) = 2 -> R = 2, bound 6145
    "B": dict(n_docs=12290, edge_bounds=(4096, 8193, 6145)),
    # nq <= 33: ceil(1024 / nq) >= 32 and 131072 >= 32 * 4096 -> R = 32, bounds 4096 r
    "C": dict(n_docs=131072, edge_bounds=tuple(4096 * r for r in range(1, 32))),
}


def handle_postings(name: str, variant: str) -> Postings:
    return synthetic_postings(HANDLES[name]["n_docs"], variant, HANDLES[name]["edge_bounds"])
