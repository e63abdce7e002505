"""CPU tests of the related-notes pass (no GPU needed): the brute-force restatement (tests/related_ref.py) equals the
reference's own output (tests/golden/related_notes_cases.json), every golden case keeps the margins that make the
comparison complete, the host halves of anorag_hip.related_notes, and the C ABI's presence."""
import copy
import os
import re

import numpy as np
import pytest

import related_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ref.load_cases()
IDS = [c["name"] for c in CASES]


def test_golden_file_covers_what_it_is_there_for():
    assert len(CASES) >= 10 and {c["dim"] for c in CASES} == {8, 40, 96}
    assert max(len(c["notes"]) for c in CASES) <= 300
    cfg = [c["config"] for c in CASES]
    assert any(not c for c in cfg) and any(c.get("exclude_same_cluster") is False for c in cfg)
    assert {0, 2} <= {c.get("min_shared_entities", 1) for c in cfg}
    assert {0, 0.6} <= {c.get("entity_similarity_weight", 0.3) for c in cfg}
    assert any(c.get("max_related_notes") == 1 for c in cfg)
    for c in CASES:
        assert c["embeddings"].shape == (len(ref.valid_positions(c["notes"], c["config"])), c["dim"])
        assert 0 < c["base_dev"] < 1e-6


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_the_reference(case):
    ref.same_related(ref.find_related_notes(case["notes"], case["embeddings"], case["config"]), case["expected"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_margin_certificate(case):
    """no decision, order or rounding of a golden case lies within 1e-5 of changing: nothing has to be left out"""
    m = ref.case_margins(case)
    assert min(m.values()) >= 1e-5, m
    for k, v in case["margins"].items():
        assert (v is None and m[k] == float("inf")) or v == m[k]


def test_margins_see_each_kind_of_closeness():
    base = np.array([[1.0, 0.9, 0.5], [0.9, 1.0, 0.2], [0.5, 0.2, 1.0]])
    ents, cl = [[], [], []], [-1, -1, -1]
    p = ref.params(w=0.0, threshold=0.9 - 1e-7)
    assert abs(ref.margins(base, ents, cl, p)["threshold"] - 1e-7) < 1e-12
    p = ref.params(w=0.0, threshold=0.1)
    m = ref.margins(base, ents, cl, p)
    assert abs(m["order"] - 0.3) < 1e-12 and m["bonus"] == float("inf")
    assert abs(m["rounding"] - 0.0005) < 1e-12          # 0.9, 0.5, 0.2 are as far from an x.xxx5 as a value can be
    p = ref.params(w=0.0, threshold=0.6 + 1e-6, exclude_same_cluster=False)
    assert abs(ref.margins(base, ents, [0, 1, 2], p)["bonus"] - 1e-6) < 1e-12
    tie = np.array([[1.0, 0.9, 0.9], [0.9, 1.0, 0.2], [0.9, 0.2, 1.0]])
    p = ref.params(w=0.0, threshold=0.1)
    assert ref.margins(tie, ents, cl, p)["order"] == 0.0 and ref.margins(tie, ents, cl, p, allow_ties=True)["order"] > 0.5
    assert abs(ref.round_margin(0.81249) - 1e-5) < 1e-9 and abs(ref.round_margin(0.8125) - 0.0) < 1e-12


def test_cluster_coding_follows_python_equality():
    from anorag_hip.related_notes import encode_clusters
    vals = [3, -1, None, "a", 3, None, -1.0, "a", 3.0, True, 1, (1, 2), [7], [7], [8]]
    codes = encode_clusters(vals).tolist()
    assert codes.count(-1) == 2 and codes[1] == codes[6] == -1
    for a in range(len(vals)):
        for b in range(len(vals)):
            assert (codes[a] == codes[b]) == (vals[a] == vals[b]), (vals[a], vals[b])
    assert encode_clusters([]).dtype == np.int32 and len(encode_clusters([])) == 0


def test_text_preparation_and_entity_similarity_match_the_restatement():
    from anorag_hip.related_notes import NoteSimilarityCalculator, entity_similarity, note_id
    calc = NoteSimilarityCalculator({})
    notes = [{"content": " a "}, {"content": "  ", "keywords": ["x", "y"]}, {"content": "", "keywords": "kw"}, {"keywords": []},
             {}, {"content": "c", "keywords": ["unused"]}, {"content": None, "keywords": 5}]
    for note in notes:
        assert calc._prepare_text_for_encoding(note) == ref.prepare_text(note)
    assert [calc._prepare_text_for_encoding(n) for n in notes] == ["a", "x y", "kw", "", "", "c", ""]
    assert NoteSimilarityCalculator({"use_content": False})._prepare_text_for_encoding({"content": "a", "keywords": ["k"]}) == "k"
    for inter, uni, la, lb in [(0, 0, 0, 0), (0, 3, 0, 3), (0, 2, 2, 0), (1, 3, 2, 2), (2, 2, 2, 2), (0, 4, 2, 2), (5, 5, 5, 5)]:
        for ms in (0, 1, 2):
            assert entity_similarity(inter, uni, la, lb, ms) == ref.ent_sim(inter, uni, la, lb, ms)
    assert entity_similarity(2, 2, 2, 2, 1) == 1.0 and entity_similarity(0, 4, 2, 2, 0) == 0.1
    assert note_id({"id": 7}) == 7 and note_id({"content": "x"}) == str(hash("x"))
    d = NoteSimilarityCalculator()
    assert (d.similarity_threshold, d.max_related_notes, d.entity_similarity_weight, d.min_shared_entities,
            d.exclude_same_cluster, d.cluster_similarity_bonus, d.model_name, d.batch_size, d.use_content) == \
        (0.75, 5, 0.3, 1, True, 0.1, 'all-MiniLM-L6-v2', 32, True)


@pytest.mark.parametrize("case", CASES[:3], ids=IDS[:3])
def test_result_shaping_from_arrays(case):
    """shape_related builds the reference's dicts from the arrays the device returns (here filled by the restatement)"""
    from anorag_hip.related_notes import shape_related
    notes, config = case["notes"], case["config"]
    p = ref.params_of_config(config)
    valid = ref.valid_positions(notes, config)
    vn = [notes[k] for k in valid]
    ents = [n.get('entities', []) for n in vn]
    rel = ref.related(ref.base_matrix(ref.stored_rows(case["embeddings"])), ents, [n.get('cluster_id', -1) for n in vn], p)
    n, M = len(vn), p["M"]
    res = {"nbr": np.full((n, M), -1, np.int32), "n_nbr": np.zeros(n, np.int32), "combined": np.zeros((n, M)),
           "base": np.zeros((n, M)), "inter": np.zeros((n, M), np.int32), "uni": np.zeros((n, M), np.int32),
           "ent_len": np.array([len(set(e)) for e in ents])}
    for i, row in enumerate(rel):
        res["n_nbr"][i] = len(row)
        for t, (j, c, b, ent, inter, uni) in enumerate(row):
            res["nbr"][i, t], res["combined"][i, t], res["base"][i, t] = j, c, b
            res["inter"][i, t], res["uni"][i, t] = inter, uni
    lists = shape_related(vn, res, p["min_shared"])
    want = [e for k, e in enumerate(case["expected"]) if k in set(valid)]
    got = [dict(note, related_notes=lst) for note, lst in zip(vn, lists)]
    ref.same_related(got, want)


def test_repeated_ids_and_too_few_notes_never_reach_the_device():
    from anorag_hip.related_notes import NoteSimilarityCalculator
    calc = NoteSimilarityCalculator({})
    emb = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="twice"):
        calc.find_related_notes([{"id": "a", "content": "x"}, {"id": "b", "content": "y"}, {"id": "a", "content": "z"}], embeddings=emb)
    with pytest.raises(ValueError, match="twice"):          # the fallback key: equal contents hash alike
        calc.find_related_notes([{"content": "same"}, {"content": "same"}, {"content": "other"}], embeddings=emb)
    notes = [{"id": "a", "content": "x"}, {"id": "b", "content": ""}, {"id": "c"}]
    before = copy.deepcopy(notes)
    assert calc.find_related_notes(notes, embeddings=emb) is notes and notes == before   # one valid note: unchanged
    assert calc.find_related_notes([]) == []
    with pytest.raises(ValueError, match="encoder"):
        NoteSimilarityCalculator({}).find_related_notes([{"id": "a", "content": "x"}, {"id": "b", "content": "y"}])


def test_similarity_statistics_restated():
    from anorag_hip.related_notes import NoteSimilarityCalculator
    notes = CASES[0]["expected"]
    st = NoteSimilarityCalculator({}).compute_similarity_statistics(notes)
    sims = [r["similarity"] for n in notes for r in n["related_notes"]]
    assert st["total_notes"] == len(notes) and st["total_relations"] == len(sims) > 0
    assert st["notes_with_relations"] == sum(1 for n in notes if n["related_notes"])
    assert st["cross_cluster_relations"] + st["same_cluster_relations"] == len(sims)
    assert st["similarity_stats"] == {"mean": np.mean(sims), "std": np.std(sims), "min": np.min(sims), "max": np.max(sims)}
    assert list(st) == ['total_notes', 'notes_with_relations', 'total_relations', 'avg_relations_per_note', 'coverage_rate',
                        'cross_cluster_relations', 'same_cluster_relations', 'similarity_stats']
    empty = NoteSimilarityCalculator({}).compute_similarity_statistics([])
    assert empty["avg_relations_per_note"] == 0 and empty["similarity_stats"]["mean"] == 0


def test_library_exports_the_related_notes_abi():
    """fails without the feature: the header's related-notes symbols are exported and bound, and the class is public"""
    import anorag_hip
    from anorag_hip import _lib
    with open(os.path.join(ROOT, "include", "anorag.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(anr_(?:index_)?related_[a-z0-9_]+)\s*\(", text)))
    assert names == ["anr_index_related_notes", "anr_related_set_option", "anr_related_timing"]
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert "ANR_RELATED_OPT_PAIR_CAP 1" in text and _lib.RELATED_OPT_PAIR_CAP == 1
    assert anorag_hip.NoteSimilarityCalculator is anorag_hip.related_notes.NoteSimilarityCalculator
    assert callable(anorag_hip.related_pairs)
    # argument checks that need no device
    import ctypes as C
    assert lib.anr_related_set_option(99, 0) == -1 and lib.anr_related_set_option(1, -5) == -1
    assert lib.anr_related_set_option(1, 0) == 0
    ms = (C.c_float * 3)()
    assert lib.anr_related_timing(0, ms) == 0
    assert lib.anr_index_related_notes(None, None, None, None, None, None, None, None, None, None, None, None) == -1
