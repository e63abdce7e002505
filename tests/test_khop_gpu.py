"""GPU tests of anr_index_khop_rerank, anr_index_cluster_suppress, anorag_hip.khop_rerank and
VectorRetriever.rerank_second_hop: the goldens recorded from the reference through the C ABI (bit-equal scores, equal
orders and kept lists), the stored-rows path against the float64 restatement (tests/khop_ref.py) at every tile edge, the
agreement of the two paths, determinism, ragged batches, the refusals and the retriever extension."""
import ctypes as C
import math
import operator
import types

import numpy as np
import pytest

import khop_ref as kr
from anorag_hip import METRIC_IP, FlatIndex, _lib
from anorag_hip.khop_rerank import KhopShapeError, cluster_suppression, rerank_khop
from vector_store.retriever import VectorRetriever

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
SIZES = [0, 1, 2, 31, 32, 33, 64, 65, 257, 1024]   # the 32-row tile edges, and the list limit
DIMS = [8, 40, 96]                                 # below and across the 64-wide k-chunk
THR = 0.9


def _bound(d):
    """the bound tests/test_diversity_gpu.py uses for this Gram tile: device and restatement each lie within gamma_d of the
    true dot product and norms (products of float32 values are exact in float64), plus a square root, a multiply, a divide"""
    return 2 * (d + 8) * U


@pytest.fixture(scope="module")
def golden():
    return kr.load_cases()


def _weights(w):
    return dict(hop_decay=w["hop_decay"], dense_weight=w["dense_weight"], bm25_weight=w["bm25_weight"],
                focused_weight_hop2=w["focused_weight_hop2"], cov_weight=w["cov_weight"], cons_weight=w["cons_weight"],
                rrf_lambda=w["rrf_lambda"])


def test_goldens_through_the_c_abi(golden):
    """dense / focused / sim_host given: final is bit-equal, order and kept are equal, for every case"""
    rer = [c for c in golden["cases"] if c["kind"] == "rerank"]
    assert len(rer) >= 15
    for case in rer:                                     # every case on its own
        a = kr.case_inputs(case)
        n = len(a["dense"])
        exp = case["expected"]
        _, _, final, order = rerank_khop(None, None, [a["bm25"]], [a["is_prf"]], [a["prf_sim"]], [a["cov"]], [a["cons"]],
                                         [a["hop_no"]], dense=[a["dense"]], focused=[a["focused"]],
                                         note_ids=[[c["note_id"] for c in case["candidates"]]], **_weights(a["w"]))[0]
        assert [kr.bits(f) for f in final] == exp["final_bits"], case["name"]
        assert list(order) == exp["order"], case["name"]
        if not a["enabled"]:
            continue
        sim = kr.cosine_eps_matrix(np.asarray(case["vectors"], dtype=np.float32).reshape(n, -1))
        o = np.asarray(order)
        kept = cluster_suppression(None, None, [final[o]], sim=[sim[np.ix_(o, o)]], cos_threshold=a["thr"],
                                   keep_per_cluster=a["keep_m"])[0]
        assert [int(o[k]) for k in kept] == exp["kept"], case["name"]
    sup = [c for c in golden["cases"] if c["kind"] == "suppress"]
    assert len(sup) >= 3
    # the suppression cases as one ragged batch per setting
    for case in sup:
        _, enabled, thr, keep_m = kr.parse_config(case["config"])
        n = len(case["scores"])
        sim = kr.cosine_eps_matrix(np.asarray(case["vectors"], dtype=np.float32).reshape(n, -1))
        kept = cluster_suppression(None, None, [case["scores"]], sim=[sim], cos_threshold=thr, keep_per_cluster=keep_m)[0]
        assert list(kept) == case["expected"]["kept"], case["name"]


def test_goldens_with_stored_rows(golden):
    """the same cases with the vectors as index rows: the device's own cosines decide the suppression (the margin of the
    fixture is far above the device's error)"""
    for case in golden["cases"]:
        n, d = len(case["candidates"]), case["dim"]
        x = np.asarray(case["vectors"], dtype=np.float32).reshape(n, d)
        index = FlatIndex(d, METRIC_IP, normalize=False, device=0)
        try:
            index.add(x)
            if case["kind"] == "suppress":
                _, _, thr, keep_m = kr.parse_config(case["config"])
                kept = cluster_suppression(index, [np.arange(n)], [case["scores"]], cos_threshold=thr, keep_per_cluster=keep_m)[0]
                assert list(kept) == case["expected"]["kept"], case["name"]
            else:
                a = kr.case_inputs(case)
                if not a["enabled"]:
                    continue
                exp = case["expected"]
                final = np.array([np.frombuffer(bytes.fromhex(b), dtype="<f8")[0] for b in exp["final_bits"]])
                o = np.asarray(exp["order"])
                kept = cluster_suppression(index, [o], [final[o]], cos_threshold=a["thr"], keep_per_cluster=a["keep_m"])[0]
                assert [int(o[k]) for k in kept] == exp["kept"], case["name"]
        finally:
            index.close()


# ---- the stored-rows path ----------------------------------------------------------------------------------------------
class _Work:
    """seeded float32 rows of one dimension, one candidate list per size in SIZES, and everything the two calls read"""

    def __init__(self, d):
        rng = np.random.default_rng(500 + d)
        n = 1500
        centres = rng.standard_normal((60, d))
        x = centres[rng.integers(0, 60, n)] + rng.choice([0.05, 0.3, 0.7, 2.0], (n, 1)) * rng.standard_normal((n, d))
        x = (x * np.exp(rng.uniform(-2, 2, (n, 1)))).astype(np.float32)
        x[7] = 0.0                       # a zero row
        x[11] = x[3]                     # identical rows
        self.d, self.x = d, x
        self.q = rng.standard_normal((len(SIZES), d)).astype(np.float32)
        self.f = rng.standard_normal((len(SIZES), d)).astype(np.float32)
        self.has_focus = [i % 3 != 1 for i in range(len(SIZES))]
        self.rows, self.arrs = [], []
        for c in SIZES:
            r = rng.permutation(n)[:c]
            if c >= 31:                  # positions 0, 1, 2: a row, the zero row, the row's duplicate
                rest = np.setdiff1d(np.arange(n), [3, 7, 11])
                r = np.concatenate([[3, 7, 11], rng.permutation(rest)[:c - 3]])
            self.rows.append(r.astype(np.int64))
            self.arrs.append({
                "bm25": np.round(rng.uniform(0, 1, c), 1), "is_prf": rng.random(c) < 0.4, "prf_sim": np.round(rng.uniform(0, 1, c), 2),
                "cov": rng.choice([0.0, 1 / 3, 0.5, 1.0], c), "cons": rng.integers(0, 2, c), "hop_no": rng.choice([1, 2, 3, 5], c)})
        self.index = FlatIndex(d, METRIC_IP, normalize=False, device=0)
        self.index.add(x)

    def rerank(self, which, **kw):
        a = [self.arrs[i] for i in which]
        return rerank_khop(self.index, [self.rows[i] for i in which], [v["bm25"] for v in a], [v["is_prf"] for v in a],
                           [v["prf_sim"] for v in a], [v["cov"] for v in a], [v["cons"] for v in a], [v["hop_no"] for v in a],
                           query_vecs=self.q[which], focus_vecs=self.f[which], has_focus=[self.has_focus[i] for i in which], **kw)


@pytest.fixture(scope="module", params=DIMS)
def work(request):
    w = _Work(request.param)
    yield w
    w.index.close()


def _cos_fsum(q, xs):
    ql = [float(v) for v in q]
    qq = math.fsum(map(operator.mul, ql, ql))
    out = []
    for x in xs:
        xl = [float(v) for v in x]
        xx, qx = math.fsum(map(operator.mul, xl, xl)), math.fsum(map(operator.mul, ql, xl))
        nq, nx = math.sqrt(qq), math.sqrt(xx)
        out.append(0.0 if nq == 0.0 or nx == 0.0 else max(0.0, qx / (nq * nx)))
    return out


def test_rerank_from_stored_rows(work):
    which = list(range(len(SIZES)))
    out = work.rerank(which)                                # one ragged call, the empty list included
    again = work.rerank(which)
    w = dict(kr.FUSION_DEFAULTS, **kr.FEATURE_DEFAULTS)
    for i, (dense, focused, final, order) in enumerate(out):
        c, a = SIZES[i], work.arrs[i]
        assert len(dense) == len(focused) == len(final) == len(order) == c
        ref_d = _cos_fsum(work.q[i], work.x[work.rows[i]])
        ref_f = _cos_fsum(work.f[i], work.x[work.rows[i]]) if work.has_focus[i] else [0.0] * c
        err = max([abs(p - r) for p, r in zip(dense, ref_d)] + [abs(p - r) for p, r in zip(focused, ref_f)] + [0.0])
        assert err <= _bound(work.d), (c, err, _bound(work.d))
        if not work.has_focus[i]:
            assert not focused.any()
        if c >= 31:
            assert dense[1] == 0.0 and focused[1] == 0.0         # the zero row
            assert dense[0] == dense[2] and focused[0] == focused[2]   # identical rows: identical bits
        # the returned values through the restatement: the rest is exact
        hop = [int(h) for h in a["hop_no"]]
        f_ref, o_ref = kr.rerank([float(v) for v in dense], [float(v) for v in focused], [float(v) for v in a["bm25"]],
                                 [bool(v) for v in a["is_prf"]], [float(v) for v in a["prf_sim"]], [float(v) for v in a["cov"]],
                                 [int(v) for v in a["cons"]], hop, [kr.decay_factor(0.85, h) for h in hop], w)
        assert [kr.bits(v) for v in final] == [kr.bits(v) for v in f_ref], c
        assert list(order) == o_ref, c
        for got, rep in zip(out[i], again[i]):                   # determinism: byte-equal
            assert got.tobytes() == rep.tobytes()
    # a ragged batch with empty queries in the middle equals the queries one at a time
    mix = [3, 0, 8, 0, 5, 1]
    batch = work.rerank(mix)
    for i, got in zip(mix, batch):
        single = work.rerank([i])[0]
        for g, s, o in zip(got, single, out[i]):
            assert g.tobytes() == s.tobytes() == o.tobytes()


def test_suppression_from_stored_rows(work):
    d = work.d
    rng = np.random.default_rng(9)
    scores = [np.round(rng.uniform(0, 1, c), 2) for c in SIZES]       # ties; not sorted
    sims = [kr.cosine_eps_matrix(work.x[r]) for r in work.rows]
    for s in sims:                                                    # on the CPU: no decision within reach of the error
        iu = np.triu_indices(s.shape[0], 1)
        assert not np.any(np.abs(s[iu] - THR) <= 100 * _bound(d))
    n_cut = 0
    for keep_m in (1, 2, 2000):
        got = cluster_suppression(work.index, work.rows, scores, cos_threshold=THR, keep_per_cluster=keep_m)
        given = cluster_suppression(None, None, scores, sim=sims, cos_threshold=THR, keep_per_cluster=keep_m)
        again = cluster_suppression(work.index, work.rows, scores, cos_threshold=THR, keep_per_cluster=keep_m)
        for i, c in enumerate(SIZES):
            ref = kr.suppress(lambda a, b, s=sims[i]: s[a, b], [float(v) for v in scores[i]], THR, keep_m)
            assert list(got[i]) == ref, (c, keep_m)
            assert list(given[i]) == ref, (c, keep_m)                 # the rows path and the sim_host path agree
            assert got[i].tobytes() == again[i].tobytes()
            n_cut += len(ref) < c
            if keep_m == 2000:
                assert sorted(ref) == list(range(c))
    assert n_cut >= 6                                                 # the data holds clusters
    mix = [4, 0, 9, 0, 2]
    batch = cluster_suppression(work.index, [work.rows[i] for i in mix], [scores[i] for i in mix], cos_threshold=THR,
                                keep_per_cluster=1)
    for i, got in zip(mix, batch):
        single = cluster_suppression(work.index, [work.rows[i]], [scores[i]], cos_threshold=THR, keep_per_cluster=1)[0]
        assert list(got) == list(single)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data if a is not None else None


def test_refusals_leave_the_outputs_untouched():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    d, n = 8, 1030
    x = rng.standard_normal((n, d)).astype(np.float32)
    index = FlatIndex(d, METRIC_IP, normalize=False, device=0)
    try:
        index.add(x)
        base = {"offs": np.array([0, 3], dtype=np.int64), "rows": np.array([0, 5, 9], dtype=np.int64),
                "q": x[:1].copy(), "f": None, "hf": None, "dense": None, "foc": None,
                "bm25": np.array([0.1, 0.2, 0.3]), "is_prf": np.array([1, 0, 1], dtype=np.uint8), "psim": np.array([0.5, 0.0, 0.6]),
                "cov": np.zeros(3), "cons": np.zeros(3, dtype=np.int32), "hop": np.full(3, 2, dtype=np.int32), "decay": np.ones(3),
                "prm": (1.0, 0.6, 0.3, 0.1, 0.05, 0.2, 50.0), "h": index._h, "nq": 1}

        def rerank_rc(**over):
            a = dict(base, **over)
            t = max(int(a["offs"][-1]), 3) if len(a["offs"]) else 3
            outs = [np.full(t, -7.0), np.full(t, -7.0), np.full(t, -7.0), np.full(t, -7, dtype=np.int32)]
            prm = _lib.KhopParams(*a["prm"])
            rc = lib.anr_index_khop_rerank(a["h"], 0, a["nq"], _p(a["offs"]), _p(a["rows"]), _p(a["q"]), _p(a["f"]), _p(a["hf"]),
                                           _p(a["dense"]), _p(a["foc"]), _p(a["bm25"]), _p(a["is_prf"]), _p(a["psim"]),
                                           _p(a["cov"]), _p(a["cons"]), _p(a["hop"]), _p(a["decay"]), C.byref(prm),
                                           *[_p(o) for o in outs])
            return rc, all((o == -7).all() for o in outs)

        assert rerank_rc() == (0, False)                                        # the base call is a good one
        nan3 = np.array([0.1, np.nan, 0.3])
        long = np.arange(1026, dtype=np.int64) % n
        z = np.zeros(1025)
        bad = {
            "too long": dict(offs=np.array([0, 1025], dtype=np.int64), rows=long, bm25=z, is_prf=np.zeros(1025, np.uint8), psim=z,
                             cov=z, cons=np.zeros(1025, np.int32), hop=np.zeros(1025, np.int32), decay=z + 1),
            "row below": dict(rows=np.array([0, -1, 9], dtype=np.int64)),
            "row above": dict(rows=np.array([0, n, 9], dtype=np.int64)),
            "nan bm25": dict(bm25=nan3), "nan prf_sim": dict(psim=nan3), "nan cov": dict(cov=nan3), "nan decay": dict(decay=nan3),
            "nan dense": dict(dense=nan3, foc=np.zeros(3)), "nan focused": dict(dense=np.zeros(3), foc=nan3),
            "nan weight": dict(prm=(1.0, 0.6, float("nan"), 0.1, 0.05, 0.2, 50.0)),
            "nan rrf_k": dict(prm=(1.0, 0.6, 0.3, 0.1, 0.05, 0.2, float("nan"))),
            "offs descend": dict(offs=np.array([0, 3, 2], dtype=np.int64), nq=2),
            "offs not from 0": dict(offs=np.array([1, 3], dtype=np.int64)),
            "no handle": dict(h=None),
        }
        for name, over in bad.items():
            assert rerank_rc(**over) == (-1, True), name
        assert rerank_rc(h=None, dense=np.zeros(3))[0] == 0                     # no rows to read: no handle needed
        assert lib.anr_index_khop_rerank(*([None, 0, 0] + [None] * 19)) == -1   # null handle, nothing given
        assert rerank_rc(nq=0)[0] == 0 and rerank_rc(offs=np.array([0, 0], dtype=np.int64)) == (0, True)

        sbase = {"offs": base["offs"], "rows": base["rows"], "sim": None, "score": np.array([0.3, 0.2, 0.1]), "thr": 0.9,
                 "keep_m": 2, "h": index._h, "nq": 1}

        def suppress_rc(**over):
            a = dict(sbase, **over)
            kept, nk = np.full(1100, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32)
            rc = lib.anr_index_cluster_suppress(a["h"], 0, a["nq"], _p(a["offs"]), _p(a["rows"]), _p(a["sim"]), _p(a["score"]),
                                                a["thr"], a["keep_m"], _p(kept), _p(nk))
            return rc, bool((kept == -7).all() and (nk == -7).all())

        assert suppress_rc() == (0, False)
        sbad = {
            "too long": dict(offs=np.array([0, 1025], dtype=np.int64), rows=long, score=z),
            "too long, sim": dict(offs=np.array([0, 1025], dtype=np.int64), sim=np.zeros(1025 * 1025), score=z, h=None),
            "row below": dict(rows=np.array([0, -1, 9], dtype=np.int64)), "row above": dict(rows=np.array([0, n, 9], dtype=np.int64)),
            "keep_m 0": dict(keep_m=0), "keep_m negative": dict(keep_m=-3), "nan thr": dict(thr=float("nan")),
            "nan score": dict(score=nan3), "offs descend": dict(offs=np.array([0, 3, 2], dtype=np.int64), nq=2),
            "offs not from 0": dict(offs=np.array([2, 3], dtype=np.int64)), "no handle": dict(h=None),
        }
        for name, over in sbad.items():
            assert suppress_rc(**over) == (-1, True), name
        assert suppress_rc(h=None, sim=np.eye(3))[0] == 0
        assert suppress_rc(nq=0) == (0, True)
        rc, untouched = suppress_rc(offs=np.array([0, 0, 0], dtype=np.int64), nq=2)
        assert rc == 0 and not untouched                                        # n_kept is written: two zeros
        # the wrapper turns a refusal into its own exception
        with pytest.raises(KhopShapeError):
            cluster_suppression(index, [[0, n]], [[0.1, 0.2]])
        with pytest.raises(KhopShapeError):
            cluster_suppression(index, [[0, 1]], [[0.1, 0.2]], keep_per_cluster=0)
        one = [[0.0]]
        with pytest.raises(KhopShapeError):
            rerank_khop(index, [[n]], one, one, one, one, one, [[2]], query_vecs=x[:1])
        assert rerank_khop(index, [], [], [], [], [], [], [], query_vecs=np.zeros((0, d))) == []
        assert cluster_suppression(index, [], []) == []
    finally:
        index.close()


# ---- the retriever extension -------------------------------------------------------------------------------------------
def test_retriever_rerank_second_hop():
    rng = np.random.default_rng(77)
    n, d = 40, 32
    centres = rng.standard_normal((6, d))
    x = centres[rng.integers(0, 6, n)] + rng.choice([0.05, 0.4, 1.5], (n, 1)) * rng.standard_normal((n, d))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    texts = {"the query": centres.sum(0) + rng.standard_normal(d), "acme founded": centres[:3].sum(0) + rng.standard_normal(d)}
    texts = {k: (v / np.linalg.norm(v)).astype(np.float32) for k, v in texts.items()}
    encoded = []

    def encode_queries(qs):
        encoded.append(list(qs))
        return np.stack([texts[q] for q in qs])

    vr = object.__new__(VectorRetriever)
    index = FlatIndex(d, METRIC_IP, normalize=False, device=0)
    try:
        index.add(x)
        vr.vector_index = types.SimpleNamespace(index=index)
        vr.embedding_manager = types.SimpleNamespace(encode_queries=encode_queries)
        vr.note_id_to_index = {f"n{j}": j for j in range(n)}
        ents = ["Acme", "Borealis", "Cobalt"]
        pick = rng.permutation(n)[:30]
        cands = [{"note_id": f"n{j}", "title": f"t{j}", "content": ("acme " if j % 4 == 0 else "") + f"text {j}",
                  "entities": [ents[j % 3]] if j % 2 else [], "hop_no": int(rng.choice([1, 2, 3])),
                  "retrieval_method": "prf_bridge" if j % 3 == 0 else "dense", "similarity_score": float(np.round(rng.random(), 3))}
                 for j in pick]
        bm25 = [float(v) for v in np.round(rng.uniform(0, 1, len(cands)), 3)]
        path_entities = ["Acme", "Cobalt"]
        # the restatement, fed with score_candidates' values (float32 cosines of the same stored rows)
        ids = [c["note_id"] for c in cands]
        dense32 = vr.score_candidates(["the query"], [ids])[0]
        foc32 = vr.score_candidates(["acme founded"], [ids])[0]
        w = dict(kr.FUSION_DEFAULTS, **kr.FEATURE_DEFAULTS)
        cc = [kr.cov_cons(c, path_entities) for c in cands]
        hop = [c["hop_no"] for c in cands]
        args = ([c["retrieval_method"] == "prf_bridge" for c in cands], [c["similarity_score"] for c in cands],
                [v[0] for v in cc], [v[1] for v in cc], hop, [kr.decay_factor(0.85, h) for h in hop], w)
        f32, o32 = kr.rerank(dense32, foc32, bm25, *args)
        # a float32 cosine of unit rows lies within (d + 2) 2^-24 of the float64 one; both enter with weights <= 1.0 and 0.4
        tol = 1.4 * (d + 2) * 2.0 ** -24
        # on the CPU: neither a rank nor the order hangs on that difference (cosines clamped to 0.0 tie in both)
        pos = np.sort([v for v in dense32 if v > 0.0])
        assert len(pos) > 10 and pos[0] > 4 * tol and np.diff(pos).min() > 4 * tol and np.diff(np.sort(f32)).min() > 4 * tol
        encoded.clear()
        out = vr.rerank_second_hop("the query", [dict(c) for c in cands], q_focus="acme founded", path_entities=path_entities,
                                   bm25_scores=bm25, suppress=False)
        assert encoded == [["the query", "acme founded"]]              # one forward for both texts
        assert [c["note_id"] for c in out] == [ids[i] for i in o32]
        assert max(abs(c["final_score"] - f32[ids.index(c["note_id"])]) for c in out) <= tol
        # exactly: the device's own cosines through the restatement
        rows = [vr.note_id_to_index[i] for i in ids]
        dev = rerank_khop(index, [rows], [bm25], [args[0]], [args[1]], [args[2]], [args[3]], [hop],
                          query_vecs=texts["the query"][None], focus_vecs=texts["acme founded"][None])[0]
        f64, o64 = kr.rerank([float(v) for v in dev[0]], [float(v) for v in dev[1]], bm25, *args)
        assert [c["final_score"] for c in out] == [f64[i] for i in o64] and o64 == o32
        # with the suppression: the reranked list through the restatement's loop on the float64 cosines
        sim = kr.cosine_eps_matrix(x[[rows[i] for i in o64]])
        iu = np.triu_indices(len(o64), 1)
        assert not np.any(np.abs(sim[iu] - 0.9) <= 100 * _bound(d))
        kept = kr.suppress(lambda a, b: sim[a, b], [f64[i] for i in o64], 0.90, 2)
        assert len(kept) < len(o64)
        full = vr.rerank_second_hop("the query", [dict(c) for c in cands], q_focus="acme founded", path_entities=path_entities,
                                    bm25_scores=bm25)
        assert [c["note_id"] for c in full] == [ids[o64[k]] for k in kept]
        # no focus phrase: focused is 0.0, one text encoded
        encoded.clear()
        nf = vr.rerank_second_hop("the query", [dict(c) for c in cands], path_entities=path_entities, bm25_scores=bm25,
                                  suppress=False)
        assert encoded == [["the query"]]
        f0, o0 = kr.rerank([float(v) for v in dev[0]], [0.0] * len(ids), bm25, *args)
        assert [(c["note_id"], c["final_score"]) for c in nf] == [(ids[i], f0[i]) for i in o0]
        assert vr.rerank_second_hop("the query", []) == []
        with pytest.raises(ValueError):
            vr.rerank_second_hop("the query", [dict(cands[0]), dict(cands[0])])
        with pytest.raises(ValueError):
            vr.rerank_second_hop("the query", [{"note_id": "nowhere"}])
    finally:
        index.close()
