"""CPU tests of the diversity scheduler: the float64 restatement (tests/diversity_ref.py) against the goldens recorded from
the reference's own DiversityScheduler (tests/golden/make_diversity_golden.py), the margin conditions of the stored file,
and the host-side pieces of the drop-in (conversion, type inference, coverage, hash dedup, the host loop kept for lists
the library refuses)."""
import os

import numpy as np
import pytest

import anorag_hip.diversity as hipdiv
import diversity_ref as dr
from retrieval import diversity_scheduler as ds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diversity_cases.npz")
COVERAGE_KEYS = ("entity_coverage", "topic_coverage", "source_coverage", "temporal_coverage")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN, allow_pickle=False)


def _restate(z, i):
    return dr.restate_case(dr.case_candidates(z, i), dr.STRATEGIES[int(z["strategy"][i])], int(z["max_candidates"][i]),
                           dr.DEDUP_METHODS[int(z["dedup_method"][i])], float(z["dedup_threshold"][i]), bool(z["quota"][i]))


def test_restatement_reproduces_the_reference_and_the_margins_hold(z):
    n = int(z["n_cases"])
    assert n >= 35
    kinds = 0
    for i in range(n):
        r = _restate(z, i)
        assert r["kept_ids"] == [str(s) for s in z[f"c{i}_kept_ids"]], i
        assert r["selected_ids"] == [str(s) for s in z[f"c{i}_selected_ids"]], i
        assert abs(r["diversity_score"] - float(z["diversity_score"][i])) <= 1e-12, i
        assert r["margin"] > dr.MARGIN, (i, r["margin"])
        kinds |= int(z["kinds"][i])
    assert kinds == (1 << len(z["kind_names"])) - 1, "a kind of case is missing from the stored file"


def test_inputs_are_small_and_float32_exact(z):
    for i in range(int(z["n_cases"])):
        emb = z[f"c{i}_emb"]
        assert emb.dtype == np.float32 and emb.shape[0] <= 80 and emb.shape[1] <= 64


def test_dropin_conversion_types_coverage_and_hash_dedup(z):
    for i in range(int(z["n_cases"])):
        cands = dr.case_candidates(z, i)
        cfg, plain = dr.case_config(z, i)
        sch = ds.DiversityScheduler(cfg)
        assert sch.diversity_config.enable_evidence_quota is True       # the constructor never passes the flag on
        items = sch._convert_to_candidate_items(cands)
        masks = [sum(1 << dr.TYPE_NAMES.index(t) for t in it.evidence_types) for it in items]
        assert masks == [int(m) for m in z[f"c{i}_type_mask"]], i
        assert masks == [dr.infer_type_mask(c) for c in cands]
        by_id = {it.id: it for it in items}
        chosen = [by_id[str(s)] for s in z[f"c{i}_selected_ids"]]
        cov = sch._calculate_coverage_metrics(chosen)
        assert [cov[k] for k in COVERAGE_KEYS] == [float(v) for v in z[f"c{i}_coverage"]], i
        if dr.DEDUP_METHODS[int(z["dedup_method"][i])] == "hash":
            kept, stats = sch.deduplication_processor.deduplicate(items)
            assert [it.id for it in kept] == [str(s) for s in z[f"c{i}_kept_ids"]]
            assert [stats["total"], stats["removed"], stats["kept"]] == [int(v) for v in z["dedup_stats"][i]]
    assert ds.DiversityScheduler({})._calculate_coverage_metrics([]) == {}


def test_host_loop_for_refused_lists_reproduces_the_goldens(z, monkeypatch):
    """the only second implementation of the decision procedure: what the drop-in uses when the library refuses a list"""
    def refuse(*a, **k):
        raise hipdiv.DiversityShapeError("refused")
    monkeypatch.setattr(hipdiv, "diversify", refuse)
    for i in range(int(z["n_cases"])):
        cfg, plain = dr.case_config(z, i)
        sch = ds.create_diversity_scheduler(cfg)
        if plain:
            sch.diversity_config.enable_evidence_quota = False
        res = ds.schedule_diverse_candidates(sch, dr.case_candidates(z, i), "q")
        assert [it.id for it in res.selected_candidates] == [str(s) for s in z[f"c{i}_selected_ids"]], i
        assert abs(res.diversity_score - float(z["diversity_score"][i])) <= 1e-12, i
        assert [res.deduplication_stats[k] for k in ("total", "removed", "kept")] == [int(v) for v in z["dedup_stats"][i]]
        assert [res.coverage_metrics[k] for k in COVERAGE_KEYS] == [float(v) for v in z[f"c{i}_coverage"]]
    st = sch.get_stats()
    assert st["total_requests"] == 1 and st["candidates_selected"] == len(res.selected_candidates)
    sch.reset_stats()
    assert sch.get_stats()["total_requests"] == 0


def test_public_surface():
    import retrieval
    for name in ("DiversityScheduler", "DiversityConfig", "CandidateItem", "DiversityResult", "DiversityStrategy",
                 "DeduplicationMethod", "CoverageMetric", "create_diversity_scheduler", "create_diversity_config",
                 "schedule_diverse_candidates"):
        assert hasattr(retrieval, name)
    c = ds.create_diversity_config("topical", max_candidates=7)
    assert c.strategy is ds.DiversityStrategy.TOPICAL and c.max_candidates == 7 and c.enable_evidence_quota
    assert ds.CandidateItem(id="a", content="x y", score=0.1).evidence_types == {"general"}
    empty = ds.DiversityScheduler({}).schedule_candidates([])
    assert empty.selected_candidates == [] and empty.diversity_score == 0.0 and empty.coverage_metrics == {}
