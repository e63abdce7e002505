"""GPU tests of anr_index_diversify, anorag_hip.diversity and the retrieval.diversity_scheduler drop-in: the goldens
recorded from the reference, the cosine kernel against the float64 restatement under its derived bound, the decision
kernel on hand-made matrices (equal to the restatement exactly), the workload's shape, and the refusals."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import diversity_ref as dr
from anorag_hip import METRIC_IP, FlatIndex, _lib
from anorag_hip.diversity import DiversityShapeError, diversify
from retrieval import diversity_scheduler as ds
from vector_store.retriever import VectorRetriever

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diversity_cases.npz")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN, allow_pickle=False)


def _retriever(ids, emb):
    """a VectorRetriever over the case's embeddings, rows stored as given (an inner-product index without normalisation),
    built without the constructor: that one loads an embedding model"""
    vr = object.__new__(VectorRetriever)
    index = FlatIndex(emb.shape[1], METRIC_IP, normalize=False, device=0)
    index.add(emb)
    vr.vector_index = types.SimpleNamespace(index=index)
    vr.note_id_to_index = {str(n): j for j, n in enumerate(ids)}
    return vr


def _check_case(z, i, vector_retriever, strip_embeddings):
    cfg, plain = dr.case_config(z, i)
    cands = dr.case_candidates(z, i)
    if strip_embeddings:
        for c in cands:
            c.pop("embedding", None)
    sch = ds.DiversityScheduler(cfg, vector_retriever=vector_retriever)
    if plain:
        sch.diversity_config.enable_evidence_quota = False
    kept = sch.deduplication_processor.deduplicate(sch._convert_to_candidate_items(cands))[0]
    assert [it.id for it in kept] == [str(s) for s in z[f"c{i}_kept_ids"]], i
    res = sch.schedule_candidates(cands, "q")
    assert [it.id for it in res.selected_candidates] == [str(s) for s in z[f"c{i}_selected_ids"]], i
    assert abs(res.diversity_score - float(z["diversity_score"][i])) <= 1e-12, (i, res.diversity_score)
    assert [res.deduplication_stats[k] for k in ("total", "removed", "kept")] == [int(v) for v in z["dedup_stats"][i]]


def test_goldens_through_the_dropin_with_stored_rows(z, monkeypatch):
    def no_host_loop(*a, **k):
        raise AssertionError("the host loop must not run for lists the library accepts")
    monkeypatch.setattr(ds, "_host_decide", no_host_loop)
    ran = 0
    for i in range(int(z["n_cases"])):
        if not z[f"c{i}_has_emb"].all():
            continue   # a candidate without an embedding follows the word rule: the sim= test below
        vr = _retriever(z[f"c{i}_ids"], z[f"c{i}_emb"])
        try:
            _check_case(z, i, vr, strip_embeddings=True)   # candidates need not carry embeddings
        finally:
            vr.vector_index.index.close()
        ran += 1
    assert ran >= 30


def test_goldens_through_the_sim_path(z, monkeypatch):
    def no_host_loop(*a, **k):
        raise AssertionError("the host loop must not run for lists the library accepts")
    monkeypatch.setattr(ds, "_host_decide", no_host_loop)
    names = [str(k) for k in z["kind_names"]]
    want = (1 << names.index("no_embedding")) | (1 << names.index("topical"))
    ran = 0
    for i in range(int(z["n_cases"])):
        if int(z["kinds"][i]) & want or i % 5 == 0:
            _check_case(z, i, None, strip_embeddings=False)
            ran += 1
    assert ran >= 6


def _full_matrices(index, row_lists):
    """Kernel A's whole matrices: no dedup and max_candidates >= C return every candidate and its similarities"""
    out = diversify(index, row_lists, [np.zeros(len(r)) for r in row_lists], max_candidates=1024, dedup=False,
                    similarity_threshold=2.0)
    for (kept, sel, _), r in zip(out, row_lists):
        assert list(kept) == list(range(len(r))) and list(sel) == list(range(len(r)))
    return [o[2] for o in out]


def _rows(rng, n, d):
    x = (rng.standard_normal((n, d)) * np.exp(rng.uniform(-3, 3, (n, 1)))).astype(np.float32)
    return x


def _check_cosine(sim, x, d):
    ref = dr.cosine_matrix_fast(x)
    assert sim.shape == ref.shape
    err = float(np.max(np.abs(sim - ref))) if sim.size else 0.0
    assert err <= 2 * (d + 8) * U, (err, 2 * (d + 8) * U)
    assert np.array_equal(sim, sim.T)


@pytest.mark.parametrize("d", [1, 3, 4, 5, 384, 770])
def test_cosine_kernel_against_the_restatement(d):
    """|sim_dev - sim_ref| <= 2 (d + 8) 2^-53: products of float32 values are exact in float64, so device and restatement
    each lie within gamma_(d-1) of the true dot product and norms, plus a square root, a multiply and a divide; |cos| <= 1"""
    rng = np.random.default_rng(100 + d)
    sizes = [1, 2, 15, 16, 17, 63, 64, 65, 257]
    n = sum(sizes) + 4
    x = _rows(rng, n, d)
    x[5] = 0.0                                   # a zero-norm row
    x[n - 3] = x[7]                              # duplicates of rows used below
    index = FlatIndex(d, METRIC_IP, normalize=False, device=0)
    try:
        index.add(x)
        lists, at = [], 0
        for c in sizes:
            lists.append(np.arange(at, at + c))
            at += c
        lists[5] = np.concatenate([[5, 7, n - 3], lists[5][3:]])        # C = 63 with the zero row and a duplicate pair
        lists[8] = np.concatenate([lists[8][:-2], [7, n - 3]])          # a duplicate pair across the last tile edge
        sims = _full_matrices(index, lists)                             # one ragged call
        for r, s in zip(lists, sims):
            _check_cosine(s, x[r], d)
        s = sims[5]
        assert not s[0].any() and not s[:, 0].any()                     # zero norm: similarity 0, the diagonal included
        assert np.array_equal(s[:, 1], s[:, 2]) and s[1, 2] == s[1, 1]  # equal rows: equal columns, bit for bit
        s = sims[8]
        assert np.array_equal(s[:, -1], s[:, -2])
        a, b = _full_matrices(index, [lists[4], lists[7][::-1]])        # other slot, other order: same values
        assert np.array_equal(a, sims[4]) and np.array_equal(b, sims[7][::-1, ::-1])
    finally:
        index.close()


def test_cosine_kernel_ragged_with_an_empty_query_and_the_largest_list():
    rng = np.random.default_rng(7)
    d = 24
    x = _rows(rng, 1100, d)
    index = FlatIndex(d, METRIC_IP, normalize=False, device=0)
    try:
        index.add(x)
        lists = [np.arange(3), np.zeros(0, dtype=np.int64), rng.permutation(1100)[:1024], np.array([9])]
        sims = _full_matrices(index, lists)
        assert sims[1].shape == (0, 0)
        for r, s in zip(lists, sims):
            _check_cosine(s, x[r], d)
    finally:
        index.close()


def _equal_to_restatement(sim, scores, masks=None, **kw):
    quotas = kw.get("quotas") or ()
    kept, sel, ks, _, info = dr.schedule(sim, scores, masks, max_candidates=kw["max_candidates"],
                                         similarity_threshold=kw["similarity_threshold"], dedup_on=kw.get("dedup", True),
                                         quota=kw.get("quota", False), quotas=quotas, balance_factor=kw.get("balance_factor", 0.8))
    got = diversify(None, None, [scores], None if masks is None else [masks], sim=[sim], **kw)[0]
    assert list(got[0]) == kept and list(got[1]) == sel, (kept, sel, got[0], got[1])
    assert np.array_equal(got[2], ks)
    return kept, sel, info


def _sym(rng, n, values):
    m = rng.choice(values, (n, n))
    m = np.triu(m, 1)
    m = m + m.T
    np.fill_diagonal(m, 1.0)
    return m


def test_decision_kernel_on_hand_made_matrices():
    rng = np.random.default_rng(11)
    thr = 0.85
    # dedup: several kept entries reach the threshold (the first in list order counts), sim exactly at the threshold,
    # equal scores (no replacement), a replacement that moves an entry to the end
    for n in (9, 40, 300):
        sim = _sym(rng, n, [0.1, 0.5, 0.85, np.nextafter(0.85, 0), 0.9])
        scores = rng.choice([0.2, 0.5, 0.5, 0.9, 1.1], n)
        for maxc in (1, n - 1, n, n + 1):
            k, s, info = _equal_to_restatement(sim, scores, max_candidates=maxc, similarity_threshold=thr)
    assert info["replaced"] > 0 and info["dropped"] > 0
    # sort and greedy ties: few distinct scores and similarities, so equal scores meet in the sort and equal gains in the
    # greedy; both forms; max_candidates at and around the list length
    n = 37
    sim = _sym(rng, n, [0.0, 0.25, 0.5])
    scores = rng.choice([0.25, 0.5, 0.75], n)
    masks = rng.choice([1, 2, 3, 4, 32], n).astype(np.uint32)
    quotas = [3, 2, 1, 0, 0, 0]
    for maxc in (1, 5, n - 1, n, n + 1):
        for quota in (False, True):
            _equal_to_restatement(sim, scores, masks, max_candidates=maxc, similarity_threshold=thr, dedup=False, quota=quota,
                                  quotas=quotas, balance_factor=0.8)
    # every quota exhausted in round one, then round two fills; no type at all: round one takes nothing (gain 1.0)
    _, s, info = _equal_to_restatement(sim, scores, masks, max_candidates=20, similarity_threshold=thr, dedup=False, quota=True,
                                       quotas=[1, 1, 1, 0, 0, 0])
    assert info["round_one"] == 3 and info["round_two_picks"] == 17
    _, s, info = _equal_to_restatement(sim, scores, np.zeros(n, np.uint32), max_candidates=4, similarity_threshold=thr,
                                       dedup=False, quota=True, quotas=quotas)
    assert info["round_one"] == 0 and len(s) == 4
    # a query that stops short: nothing left exceeds the -1.0 start
    low = np.full(n, -9.0)
    low[[3, 8]] = 0.6
    for quota in (False, True):
        _, s, info = _equal_to_restatement(sim, low, masks, max_candidates=10, similarity_threshold=thr, dedup=False, quota=quota,
                                           quotas=quotas)
        assert info["stopped_short"] and len(s) < 10
    # a batch: each query decided on its own matrix
    sims = [_sym(rng, c, [0.1, 0.6, 0.9]) for c in (5, 0, 70)]
    scs = [rng.random(c) for c in (5, 0, 70)]
    out = diversify(None, None, scs, sim=sims, max_candidates=6, similarity_threshold=thr)
    for m, sc, o in zip(sims, scs, out):
        k, s, ks, _, _ = dr.schedule(m, sc, max_candidates=6, similarity_threshold=thr)
        assert list(o[0]) == k and list(o[1]) == s and np.array_equal(o[2], ks)


def test_full_size_decision_matches_the_restatement():
    """the workload's shape: 8 queries, 200 candidates of 768 dimensions, 50 selected, both forms"""
    rng = np.random.default_rng(2024)
    B, Cq, d, K = 8, 200, 768, 50
    centres = rng.standard_normal((40, d))
    common = rng.standard_normal(d)      # a shared component: every cosine is positive, none clamps to 0
    x = (common + centres[rng.integers(0, 40, B * Cq)] + 0.9 * rng.standard_normal((B * Cq, d))).astype(np.float32)
    x[10] = x[3]
    for b in range(B):                    # near-duplicates on either side of the threshold
        for j in (20, 21, 22, 23):
            x[b * Cq + j] = x[b * Cq + j - 15] + np.float32(0.1 * (j - 19)) * rng.standard_normal(d).astype(np.float32)
    scores = [np.round(rng.uniform(0.0, 0.98, Cq), 6) for _ in range(B)]
    masks = [rng.choice([1, 2, 5, 8, 9, 16, 32], Cq).astype(np.uint32) for _ in range(B)]
    rows = [np.arange(b * Cq, (b + 1) * Cq) for b in range(B)]
    index = FlatIndex(d, METRIC_IP, normalize=False, device=0)
    try:
        index.add(x)
        for quota in (False, True):
            kw = dict(max_candidates=K, similarity_threshold=0.85, quota=quota, quotas=dr.QUOTAS, balance_factor=0.8)
            out = index.diversify(rows, scores, masks, **kw)
            for b in range(B):
                k, s, ks, margin, _ = dr.schedule(dr.cosine_matrix_fast(x[rows[b]]), scores[b], masks[b], max_candidates=K,
                                                  similarity_threshold=0.85, quota=quota, quotas=dr.QUOTAS)
                assert margin > dr.MARGIN, margin
                assert list(out[b][0]) == k and list(out[b][1]) == s
                assert len(s) == K and float(np.max(np.abs(out[b][2] - ks))) <= 2 * (d + 8) * U
    finally:
        index.close()


def test_refusals_and_the_dropin_fallback(caplog):
    lib = _lib.load()
    rng = np.random.default_rng(5)
    d = 8
    x = _rows(rng, 1030, d)
    index = FlatIndex(d, METRIC_IP, normalize=False, device=0)
    try:
        index.add(x)
        kw = dict(max_candidates=5, similarity_threshold=0.85)
        for bad in (-1, 1030):
            with pytest.raises(DiversityShapeError):
                diversify(index, [[0, bad, 2]], [[0.1, 0.2, 0.3]], **kw)
        with pytest.raises(DiversityShapeError):
            diversify(index, [np.arange(1025)], [np.zeros(1025)], **kw)
        with pytest.raises(DiversityShapeError):
            diversify(None, None, [np.zeros(1025)], sim=[np.zeros((1025, 1025))], **kw)
        assert diversify(index, [], [], **kw) == []
        e = diversify(index, [[], []], [[], []], **kw)
        assert [len(v[0]) + len(v[1]) for v in e] == [0, 0]
        assert lib.anr_index_diversify(None, 0, 1, None, None, None, None, None, None, None, None, None, None, None) == -1
        # the drop-in: 1030 candidates are refused with rows and with sim=, logged, and decided by the host loop
        vr = object.__new__(VectorRetriever)
        vr.vector_index = types.SimpleNamespace(index=index)
        vr.note_id_to_index = {f"n{j}": j for j in range(1030)}
        cands = [{"id": f"n{j}", "content": f"w{j}", "score": float(s), "embedding": [float(v) for v in x[j]],
                  "topics": [], "entities": []}
                 for j, s in enumerate(np.round(rng.uniform(0, 1, 1030), 6))]
        sch = ds.DiversityScheduler({"diversity_scheduler": {"max_candidates": 12, "deduplication": {"method": "hash"}}},
                                    vector_retriever=vr)
        with caplog.at_level("WARNING"):
            res = sch.schedule_candidates(cands)
        assert "deciding it on the host" in caplog.text
        want = dr.restate_case(cands, "hybrid", 12, "hash", 0.85, True)
        assert [it.id for it in res.selected_candidates] == want["selected_ids"]
    finally:
        index.close()
