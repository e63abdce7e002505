"""CPU tests of the second-hop rerank and the cluster suppression (no GPU needed): the plain-Python restatement
(tests/khop_ref.py) reproduces every golden recorded from the reference's own method bodies — scores by their bits,
orders and kept lists exactly — and the Python wrapper packs its arguments as the C ABI expects and refuses bad input."""
import ctypes as C
import types

import numpy as np
import pytest

import khop_ref as kr


@pytest.fixture(scope="module")
def golden():
    return kr.load_cases()


def test_the_fixture_holds_every_kind_of_case(golden):
    names = {c["name"] for c in golden["cases"]}
    assert {"ties", "prf_none", "prf_all", "prf_mixed", "hops", "decay_085", "decay_one", "decay_zero", "no_focus",
            "no_path_entities", "keep_1", "keep_2", "keep_all", "disabled", "unsorted", "identical_rows", "zero_row"} <= names
    assert golden["rrf_k"] == kr.RRF_K


def test_restatement_reproduces_every_golden(golden):
    for case in golden["cases"]:
        final, order, kept = kr.restate_case(case)
        exp = case["expected"]
        if case["kind"] == "rerank":
            assert [kr.bits(f) for f in final] == exp["final_bits"], case["name"]
            assert order == exp["order"], case["name"]
        assert kept == exp["kept"], case["name"]


def test_no_golden_cosine_is_within_its_margin_of_the_threshold(golden):
    """the margin is d * 2^-23 (a float32 dot product of normalised rows), stored with the case"""
    for case in golden["cases"]:
        assert case["margin"] == case["dim"] * 2.0 ** -23
        _, _, thr, _ = kr.parse_config(case["config"])
        n = len(case["candidates"])
        cos = kr.cosine_eps_matrix(np.asarray(case["vectors"], dtype=np.float32).reshape(n, -1))
        iu = np.triu_indices(n, 1)
        assert not np.any(np.abs(cos[iu] - thr) <= case["margin"]), case["name"]


def test_the_cases_show_their_properties(golden):
    by = {c["name"]: c for c in golden["cases"]}
    a = kr.case_inputs(by["hops"])
    assert set(a["hop_no"]) == {1, 2, 3, 5} and a["w"]["focused_weight_hop2"] - 0.10 * 3 < 0.0
    assert kr.case_inputs(by["no_focus"])["focused"] == [0.0] * len(by["no_focus"]["candidates"])
    a = kr.case_inputs(by["no_path_entities"])
    assert not any(a["cov"]) and not any(a["cons"])
    assert set(kr.case_inputs(by["decay_one"])["decay"]) == {1.0} and set(kr.case_inputs(by["decay_zero"])["decay"]) == {1.0}
    assert 0.85 ** 4 in kr.case_inputs(by["decay_085"])["decay"]
    assert kr.parse_config(by["unparsable"]["config"])[0]["dense_weight"] == 1.0
    assert kr.parse_config(by["unparsable"]["config"])[0]["rrf_lambda"] == 0.35
    assert kr.parse_config(by["unparsable"]["config"])[1:] == (True, 0.90, 2)
    assert 0 not in by["unsorted"]["expected"]["kept"]
    assert len(by["keep_1"]["expected"]["kept"]) < len(by["keep_2"]["expected"]["kept"]) + 1
    assert by["disabled"]["expected"]["kept"] == by["disabled"]["expected"]["order"]


def test_ranks_and_suppression_on_hand_examples():
    assert kr.ranks_desc([0.5, 0.9, 0.5, 0.1]) == [2, 1, 3, 4]
    assert kr.ranks_desc([0.5, 0.9, 0.5, 0.1], [True, False, True, True]) == [1, 0, 2, 3]
    cos = {(0, 1): 0.95, (0, 2): 0.95, (1, 2): 0.1}
    f = lambda i, j: cos.get((i, j), 0.0)  # noqa: E731
    assert kr.suppress(f, [0.1, 0.9, 0.5], 0.9, 1) == [1]            # the seed loses to a later member
    assert kr.suppress(f, [0.1, 0.9, 0.5], 0.9, 2) == [1, 2]
    assert kr.suppress(lambda i, j: 0.0, [0.1, 0.9, 0.5], 0.9, 1) == [1, 2, 0]
    # similarity is taken to the seed: 1 and 2 are close to each other, not to 0
    assert kr.suppress(lambda i, j: 0.95 if (i, j) == (1, 2) else 0.0, [0.9, 0.5, 0.4], 0.9, 1) == [0, 1]


# ---- the wrapper -----------------------------------------------------------------------------------------------------
def _arr(ptr, dtype, n):
    if ptr is None:
        return None
    dt = np.dtype(dtype)
    return np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(ptr), dtype=dt).copy()


class _FakeLib:
    """records what the wrapper hands to the two entry points and answers with a fixed pattern"""

    def __init__(self):
        self.calls = []

    def anr_index_khop_rerank(self, h, dev, nq, offs, rows, qv, fv, hf, dense, foc, bm25, is_prf, psim, cov, cons, hop, decay,
                              prm, o_dense, o_foc, o_fin, o_ord):
        offs_a = _arr(offs, np.int64, nq + 1)
        t = int(offs_a[-1])
        p = prm._obj
        self.calls.append({
            "h": h, "dev": dev, "nq": nq, "offs": offs_a, "rows": _arr(rows, np.int64, t), "hf": _arr(hf, np.uint8, nq),
            "dense": _arr(dense, np.float64, t), "foc": _arr(foc, np.float64, t), "bm25": _arr(bm25, np.float64, t),
            "is_prf": _arr(is_prf, np.uint8, t), "psim": _arr(psim, np.float64, t), "cov": _arr(cov, np.float64, t),
            "cons": _arr(cons, np.int32, t), "hop": _arr(hop, np.int32, t), "decay": _arr(decay, np.float64, t),
            "qv": qv, "fv": fv,
            "prm": (p.dense_w, p.bm25_w, p.focused_w2, p.cov_w, p.cons_w, p.rrf_lambda, p.rrf_k)})
        out = np.frombuffer((C.c_char * (t * 8)).from_address(o_fin), dtype=np.float64)
        out[:] = np.arange(t)
        order = np.frombuffer((C.c_char * (t * 4)).from_address(o_ord), dtype=np.int32)
        order[:] = np.concatenate([np.arange(b - a)[::-1] for a, b in zip(offs_a[:-1], offs_a[1:])])
        return 0

    def anr_index_cluster_suppress(self, h, dev, nq, offs, rows, sim, score, thr, keep_m, kept, n_kept):
        offs_a = _arr(offs, np.int64, nq + 1)
        t = int(offs_a[-1])
        sizes = np.diff(offs_a)
        self.calls.append({"h": h, "nq": nq, "offs": offs_a, "rows": _arr(rows, np.int64, t),
                           "sim": _arr(sim, np.float64, int((sizes * sizes).sum())), "score": _arr(score, np.float64, t),
                           "thr": thr, "keep_m": keep_m})
        nk = np.frombuffer((C.c_char * (nq * 4)).from_address(n_kept), dtype=np.int32)
        nk[:] = np.minimum(sizes, 1)
        return 0


@pytest.fixture()
def fake(monkeypatch):
    from anorag_hip import _lib
    lib = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    return lib


def test_rerank_wrapper_packs_ragged_queries(fake):
    from anorag_hip.khop_rerank import rerank_khop
    out = rerank_khop(None, None, [[0.5, 0.25], [], [1.0]], [[True, False], [], [0]], [[0.9, 0.0], [], [0.3]],
                      [[0.5, 0.0], [], [1.0]], [[1, 0], [], [1]], [[1, 3], [], [2]], dense=[[0.1, 0.2], [], [0.3]],
                      focused=[[0.4, 0.5], [], [0.6]], hop_decay=0.5, bm25_weight=0.7, device=3,
                      note_ids=[["a", "b"], [], ["a"]])
    c = fake.calls[0]
    assert c["h"] is None and c["dev"] == 3 and c["nq"] == 3 and list(c["offs"]) == [0, 2, 2, 3]
    assert c["rows"] is None and c["qv"] is None and c["fv"] is None and c["hf"] is None
    assert list(c["dense"]) == [0.1, 0.2, 0.3] and list(c["foc"]) == [0.4, 0.5, 0.6] and list(c["bm25"]) == [0.5, 0.25, 1.0]
    assert list(c["is_prf"]) == [1, 0, 0] and list(c["psim"]) == [0.9, 0.0, 0.3] and list(c["cons"]) == [1, 0, 1]
    assert list(c["hop"]) == [1, 3, 2] and list(c["decay"]) == [1.0, 0.5 ** 2, 0.5]
    assert c["prm"] == (1.0, 0.7, 0.30, 0.10, 0.05, 0.2, 50.0)
    assert [list(o[2]) for o in out] == [[0.0, 1.0], [], [2.0]] and [list(o[3]) for o in out] == [[1, 0], [], [0]]


def test_rerank_wrapper_passes_rows_and_vectors(fake):
    from anorag_hip.khop_rerank import rerank_khop
    index = types.SimpleNamespace(_h=1234, device=1, d=4)
    q = np.arange(8, dtype=np.float64).reshape(2, 4)
    one = [[0.0]] * 2
    rerank_khop(index, [[5], [7]], one, one, one, one, one, [[2]] * 2, query_vecs=q, focus_vecs=q, has_focus=[True, False])
    c = fake.calls[0]
    assert c["h"] == 1234 and c["dev"] == 1 and list(c["rows"]) == [5, 7] and list(c["hf"]) == [1, 0]
    assert list(_arr(c["qv"], np.float32, 8)) == list(range(8)) and c["dense"] is None
    rerank_khop(index, [[5], [7]], one, one, one, one, one, [[2]] * 2, query_vecs=q)
    assert fake.calls[1]["fv"] is None and fake.calls[1]["hf"] is None


def test_wrapper_value_errors(fake):
    from anorag_hip.khop_rerank import cluster_suppression, rerank_khop
    one = [[0.0, 0.0]]
    with pytest.raises(ValueError, match="repeat a note_id"):
        rerank_khop(None, None, one, one, one, one, one, one, dense=one, note_ids=[["x", "x"]])
    with pytest.raises(ValueError, match="index or dense"):
        rerank_khop(None, [[0, 1]], one, one, one, one, one, one)
    with pytest.raises(ValueError, match="cov"):
        rerank_khop(None, None, one, one, one, [[0.0]], one, one, dense=one)
    index = types.SimpleNamespace(_h=1, device=0, d=4)
    with pytest.raises(ValueError, match="query_vecs"):
        rerank_khop(index, [[0, 1]], one, one, one, one, one, one, query_vecs=np.zeros((1, 5)))
    with pytest.raises(ValueError, match="sim"):
        cluster_suppression(None, None, [[0.1, 0.2]], sim=[np.zeros((3, 3))])
    with pytest.raises(ValueError, match="index or sim"):
        cluster_suppression(None, [[0, 1]], [[0.1, 0.2]])
    assert not fake.calls


def test_suppression_wrapper_packs_matrices(fake):
    from anorag_hip.khop_rerank import cluster_suppression
    m = np.arange(4.0).reshape(2, 2)
    out = cluster_suppression(None, None, [[0.5, 0.6], [], [0.1]], sim=[m, np.zeros((0, 0)), np.ones((1, 1))],
                              cos_threshold=0.8, keep_per_cluster=3)
    c = fake.calls[0]
    assert c["h"] is None and list(c["offs"]) == [0, 2, 2, 3] and list(c["sim"]) == [0, 1, 2, 3, 1]
    assert list(c["score"]) == [0.5, 0.6, 0.1] and c["thr"] == 0.8 and c["keep_m"] == 3 and c["rows"] is None
    assert [len(o) for o in out] == [1, 0, 1]


def test_decay_factors_are_pythons_own_power():
    from anorag_hip.khop_rerank import decay_factors
    assert decay_factors(0.85, [0, 1, 2, 3, 5]) == [1.0, 1.0, 0.85, 0.85 ** 2, 0.85 ** 4]
    for outside in (0.0, 1.0, 1.5, -0.2):
        assert decay_factors(outside, [1, 2, 5]) == [1.0, 1.0, 1.0]
    assert decay_factors(0.85, [2, 5]) == [kr.decay_factor(0.85, 2), kr.decay_factor(0.85, 5)]


def test_retriever_reads_the_reference_config_keys(monkeypatch):
    from vector_store import retriever as rt
    for cfg in ({}, {"fusion": {"dense_weight": "much", "bm25_weight": None, "rrf_lambda": "0.35"},
                     "features": {"cov_weight": [], "hop_decay": 0.5},
                     "cluster_suppression": {"enabled": " No ", "cos_threshold": "high", "keep_per_cluster": "two"}},
                {"cluster_suppression": {"enabled": 0, "keep_per_cluster": 3.7, "cos_threshold": "0.8"}}):
        monkeypatch.setattr(rt, "config", types.SimpleNamespace(
            get=lambda key, default=None, cfg=cfg: cfg.get(key.split(".", 1)[1], default) if key.startswith("hybrid_search.") else default))
        assert rt._khop_config() == kr.parse_config(cfg)
    note = {"entities": ["Acme", "Gale"], "title": "T", "content": "about acme and more"}
    for pe in (None, [], ["ACME", "Fjord"], ["zeta"]):
        assert rt._cov_cons(note, pe) == kr.cov_cons(note, pe)
    assert rt._cov_cons(note, ["ACME", "Fjord"]) == (0.5, 1)
