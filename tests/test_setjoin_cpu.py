"""CPU tests of the set-overlap join: the brute-force restatement (tests/setjoin_ref.py) equals what the reference's own
extract_entity_coexistence_relations / extract_topic_relations returned (tests/golden/relation_cases.json), floats by their
bits; the C ABI has the new entry points; anr_setjoin_create refuses malformed rows on the host, with no device present;
the host half of SetJoin numbers and de-duplicates items as documented."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import setjoin_ref as ref

CASES = ref.load_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["anr_setjoin_create", "anr_setjoin_destroy", "anr_setjoin_cooccur", "anr_setjoin_cooccur_fetch",
         "anr_setjoin_pair_counts", "anr_setjoin_set_option"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference(name):
    case = CASES[name]
    got = ref.canonical(ref.entity_coexistence(case["notes"], case["threshold"]), case["notes"])
    ref.same_relations(got, case["coexistence"])
    ref.same_relations(ref.topic(case["notes"]), case["topic"])


def test_goldens_cover_what_they_are_there_for():
    assert len(CASES) >= 10 and {c["threshold"] for c in CASES.values()} >= {0, 1, 2, 3}
    assert len(CASES["nothing_kept"]["coexistence"]) == 0 and len(CASES["grouping"]["topic"]) > 0
    sims = {r["metadata"]["note_similarity"] for r in CASES["grouping"]["topic"]}
    assert {0.5, 0.1} <= sims


def test_restatement_join_matches_the_builder():
    """the integer join and the relation builder of the restatement agree with each other"""
    case = CASES["duplicates"]
    items, rows = ref.encode([n.get("entities", []) for n in case["notes"]])
    I, J, inter, uni, ptr, common = ref.cooccur(rows, 2)
    rel = ref.entity_coexistence(case["notes"], 2)
    assert len(rel) == len(I) > 0 and ptr[-1] == len(common) == inter.sum()
    for p, r in enumerate(rel):
        assert r["metadata"]["common_entities"] == [items[e] for e in common[ptr[p]:ptr[p + 1]]]
        assert r["metadata"]["jaccard_similarity"] == int(inter[p]) / int(uni[p])
    pi, pu = ref.pair_counts(rows, I, J)
    assert np.array_equal(pi, inter) and np.array_equal(pu, uni)


def test_new_symbols_and_signatures():
    from anorag_hip import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "anorag.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\bint %s\(" % name, header)
    assert _lib.SIGNATURES["anr_setjoin_create"][1][:2] == [C.c_int64, C.c_int64]
    assert len(_lib.SIGNATURES["anr_setjoin_cooccur_fetch"][1]) == 7
    assert _lib.SETJOIN_OPT_TABLE_SLOTS == 1 and "#define ANR_SETJOIN_OPT_TABLE_SLOTS 1" in header


@pytest.mark.parametrize("rows,n_items,word", [
    ([[0, 1], [3, 2]], 4, "ascending"),      # a descending row
    ([[0, 1, 1]], 4, "ascending"),           # a repeated id
    ([[0, 4]], 4, "outside"),                # an id out of range
    ([[-1, 2]], 4, "outside"),
])
def test_create_refuses_malformed_rows_on_the_host(rows, n_items, word):
    from anorag_hip import _lib
    lib = _lib.load()
    indptr, items = ref.to_csr(rows)
    h = C.c_void_p()
    rc = lib.anr_setjoin_create(len(rows), n_items, indptr.ctypes.data, items.ctypes.data, 0, C.byref(h))
    assert rc == -1 and not h.value
    assert word in _lib.last_error()


def test_host_id_mapping_and_deduplication():
    from anorag_hip.note_relations import encode_rows
    items, indptr, ids = encode_rows([["b", "a", "b"], [], ("c", "a"), ["c", "c", "c"], [7, "a", 7.5]])
    assert items == ["b", "a", "c", 7, 7.5]
    assert indptr.dtype == np.int64 and indptr.tolist() == [0, 2, 2, 4, 5, 8]
    assert ids.dtype == np.int32 and ids.tolist() == [0, 1, 1, 2, 2, 1, 3, 4]
    items, indptr, ids = encode_rows([])
    assert items == [] and indptr.tolist() == [0] and ids.shape == (0,)
    r_items, r_rows = ref.encode([["b", "a", "b"], [], ("c", "a")])
    assert r_items == ["b", "a", "c"] and r_rows == [[0, 1], [], [1, 2]]


def test_host_rules_need_no_device():
    from anorag_hip import note_relations as nr
    notes = [{"note_id": "a", "entities": ["x"]}, {"note_id": "a", "entities": ["x"]}]
    with pytest.raises(ValueError, match="keep the reference"):
        nr.entity_coexistence_relations(notes, device=10 ** 6)
    with pytest.raises(ValueError, match="keep the reference"):
        nr.entity_coexistence_relations([{"entities": ["x"]}], device=10 ** 6)
    case = CASES["grouping"]
    groups = nr.topic_groups(case["notes"])
    assert 0 not in groups and "" not in groups and list(groups)[:2] == ["alpha", 1]
    assert nr.topic_relations([{"note_id": "a", "cluster_id": 0}, {"note_id": "b", "cluster_id": 0}], device=10 ** 6) == []
    sim = nr.note_similarity([0, 0, 2, 2], [0, 3, 0, 2], [0, 0, 0, 1], [0, 3, 2, 3], [0, 1, 0, 0], [0, 2, 0, 0])
    assert sim.tolist() == [0.5, 0.1, 0.1, min(0.7 * (1 / 3) + 0.3 * 0.0, 1.0)]


def test_module_is_exported():
    import anorag_hip
    assert anorag_hip.SetJoin is anorag_hip.note_relations.SetJoin
    assert anorag_hip.topic_relations is anorag_hip.note_relations.topic_relations
