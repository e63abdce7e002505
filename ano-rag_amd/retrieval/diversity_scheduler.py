"""Drop-in for the reference's ``retrieval/diversity_scheduler.py``: candidate diversity and evidence-coverage scheduling,
the step between fused evidence and the answer context (``QueryProcessor._schedule_merged_evidence``,
query/query_processor.py:3367).  Same public surface and behaviour; the arithmetic on embeddings runs in the library.

What stays on the host: conversion of candidate dicts to ``CandidateItem`` (with evidence-type inference), hash / exact /
fuzzy dedup, coverage metrics, the topical evaluator, the statistics and their lock.  What goes to the device
(``anorag_hip.diversity.diversify`` = ``anr_index_diversify``): the semantic dedup and the greedy / quota selection.

* With ``vector_retriever=`` every candidate whose id is in ``note_id_to_index`` is a stored row of the retriever's flat
  index and the device computes the cosine matrix from those rows: candidates need not carry embeddings.
* Without it, or when a candidate has no row, the matrix is built here by the reference's per-pair rule (cosine of the
  ``embedding`` lists in float64, word Jaccard where an embedding is missing, topic Jaccard for the selection under
  ``strategy: topical``) and handed over as ``sim=``; the decision procedure still runs in the library.
* A list the library refuses (more than 1024 candidates) is logged and decided by ``_host_decide``, a plain-loop
  restatement kept only for that case.

As in the reference, ``DiversityScheduler.__init__`` never passes ``enable_evidence_quota`` to its ``DiversityConfig``:
the quota form runs unless ``scheduler.diversity_config.enable_evidence_quota`` is set to False afterwards.
"""
from __future__ import annotations

import hashlib
import logging
import threading
import time
from abc import ABC, abstractmethod
from collections import defaultdict
from dataclasses import dataclass, field
from enum import Enum
from typing import Any, Dict, List, Optional, Set, Tuple

import numpy as np

logger = logging.getLogger(__name__)


class DiversityStrategy(Enum):
    SEMANTIC = "semantic"
    TOPICAL = "topical"
    TEMPORAL = "temporal"
    SOURCE = "source"
    ENTITY = "entity"
    HYBRID = "hybrid"


class DeduplicationMethod(Enum):
    EXACT = "exact"
    FUZZY = "fuzzy"
    SEMANTIC = "semantic"
    HASH = "hash"
    HYBRID = "hybrid"


class CoverageMetric(Enum):
    ENTITY_COVERAGE = "entity_coverage"
    TOPIC_COVERAGE = "topic_coverage"
    TEMPORAL_COVERAGE = "temporal_coverage"
    SOURCE_COVERAGE = "source_coverage"
    SEMANTIC_COVERAGE = "semantic_coverage"


def _default_coverage_weights() -> Dict[str, float]:
    return {"entity": 0.3, "topic": 0.3, "temporal": 0.2, "source": 0.2}


def _default_quotas() -> Dict[str, int]:
    return {"vector": 15, "graph": 10, "path_aware": 8, "semantic": 12, "entity_rich": 6}


@dataclass
class DiversityConfig:
    strategy: DiversityStrategy = DiversityStrategy.HYBRID
    max_candidates: int = 50
    diversity_threshold: float = 0.7
    deduplication_method: DeduplicationMethod = DeduplicationMethod.HYBRID
    similarity_threshold: float = 0.85
    coverage_weights: Dict[str, float] = field(default_factory=_default_coverage_weights)
    enable_clustering: bool = True
    cluster_threshold: float = 0.6
    evidence_type_quotas: Dict[str, int] = field(default_factory=_default_quotas)
    enable_evidence_quota: bool = True
    quota_balance_factor: float = 0.8


@dataclass
class CandidateItem:
    id: str
    content: str
    score: float
    metadata: Dict[str, Any] = field(default_factory=dict)
    entities: List[str] = field(default_factory=list)
    topics: List[str] = field(default_factory=list)
    timestamp: Optional[float] = None
    source: Optional[str] = None
    embedding: Optional[List[float]] = None
    content_hash: Optional[str] = None
    evidence_types: Set[str] = field(default_factory=set)
    path_score: float = 0.0
    entity_density: float = 0.0
    source_types: Set[str] = field(default_factory=set)

    def __post_init__(self):
        if not self.content_hash:
            self.content_hash = hashlib.md5(self.content.encode()).hexdigest()[:12]
        self._infer_evidence_types()

    def _infer_evidence_types(self):
        """evidence types from where the candidate came from and how it scored; 'general' when nothing applies"""
        for origin in ("vector", "graph"):
            if origin in self.source_types:
                self.evidence_types.add(origin)
        if self.path_score > 0.3:
            self.evidence_types.add("path_aware")
        if self.entity_density > 0.5:
            self.evidence_types.add("entity_rich")
        if self.score > 0.7:
            self.evidence_types.add("semantic")
        if not self.evidence_types:
            self.evidence_types.add("general")


@dataclass
class DiversityResult:
    selected_candidates: List[CandidateItem]
    diversity_score: float
    coverage_metrics: Dict[str, float]
    deduplication_stats: Dict[str, int]
    execution_time: float
    metadata: Dict[str, Any] = field(default_factory=dict)


def _jaccard(a: set, b: set) -> float:
    if not a or not b:
        return 0.0
    union = len(a | b)
    return len(a & b) / union if union > 0 else 0.0


def _word_similarity(text1: str, text2: str) -> float:
    return _jaccard(set(text1.lower().split()), set(text2.lower().split()))


def _embedding_similarity(item1: CandidateItem, item2: CandidateItem) -> float:
    """cosine of the two embedding lists in float64, clamped to [0, 1]; word Jaccard when either has none"""
    if not item1.embedding or not item2.embedding:
        return _word_similarity(item1.content, item2.content)
    a, b = np.array(item1.embedding), np.array(item2.embedding)
    dot = np.dot(a, b)
    na, nb = np.linalg.norm(a), np.linalg.norm(b)
    if na == 0 or nb == 0:
        return 0.0
    return max(0.0, min(1.0, dot / (na * nb)))


def _pair_matrix(items: List[CandidateItem], rule) -> np.ndarray:
    n = len(items)
    m = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        for j in range(i, n):
            m[i, j] = m[j, i] = rule(items[i], items[j])
    return m


def _semantic_matrix(items: List[CandidateItem]) -> np.ndarray:
    """the per-pair semantic rule as one matrix: the cosine block at once, word Jaccard for pairs without embeddings"""
    n = len(items)
    has = [bool(it.embedding) for it in items]
    m = np.zeros((n, n), dtype=np.float64)
    idx = [i for i in range(n) if has[i]]
    if idx and len({len(items[i].embedding) for i in idx}) == 1:
        a = np.array([items[i].embedding for i in idx], dtype=np.float64)
        nrm = np.sqrt(np.einsum("ij,ij->i", a, a))
        g = a @ a.T
        den = nrm[:, None] * nrm[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = g / den
        s = np.where(s < 1.0, s, 1.0)
        s = np.where(s > 0.0, s, 0.0)
        s[den == 0.0] = 0.0
        m[np.ix_(idx, idx)] = s
    else:
        for x, i in enumerate(idx):
            for j in idx[x:]:
                m[i, j] = m[j, i] = _embedding_similarity(items[i], items[j])
    for i in range(n):
        for j in range(i, n):
            if not (has[i] and has[j]):
                m[i, j] = m[j, i] = _word_similarity(items[i].content, items[j].content)
    return m


class DiversityEvaluator(ABC):
    @abstractmethod
    def evaluate_diversity(self, candidates: List[CandidateItem]) -> float:
        ...

    @abstractmethod
    def calculate_similarity(self, item1: CandidateItem, item2: CandidateItem) -> float:
        ...


class SemanticDiversityEvaluator(DiversityEvaluator):
    def __init__(self, config: Dict[str, Any]):
        self.config = config.get("semantic_diversity", {})
        self.embedding_dim = self.config.get("embedding_dim", 768)

    def evaluate_diversity(self, candidates: List[CandidateItem]) -> float:
        if len(candidates) <= 1:
            return 1.0
        return self.diversity_from_matrix(_pair_matrix(candidates, self.calculate_similarity))

    @staticmethod
    def diversity_from_matrix(sim) -> float:
        """one minus the mean similarity of the pairs i < j, summed in that order"""
        k = len(sim)
        if k <= 1:
            return 1.0
        total, pairs = 0.0, 0
        for i in range(k):
            for j in range(i + 1, k):
                total += float(sim[i][j])
                pairs += 1
        return max(0.0, min(1.0, 1.0 - total / pairs))

    def calculate_similarity(self, item1: CandidateItem, item2: CandidateItem) -> float:
        return _embedding_similarity(item1, item2)

    def _text_similarity(self, text1: str, text2: str) -> float:
        return _word_similarity(text1, text2)


class TopicalDiversityEvaluator(DiversityEvaluator):
    def __init__(self, config: Dict[str, Any]):
        self.config = config.get("topical_diversity", {})

    def evaluate_diversity(self, candidates: List[CandidateItem]) -> float:
        """normalised entropy of the topic distribution; 0.5 without topics"""
        if len(candidates) <= 1:
            return 1.0
        counts: Dict[str, int] = defaultdict(int)
        for c in candidates:
            for t in c.topics:
                counts[t] += 1
        if not counts:
            return 0.5
        total = sum(counts.values())
        entropy = 0.0
        for n in counts.values():
            p = n / total
            entropy -= p * np.log2(p)
        top = np.log2(len(counts))
        diversity = entropy / top if top > 0 else 0.0
        return max(0.0, min(1.0, diversity))

    def calculate_similarity(self, item1: CandidateItem, item2: CandidateItem) -> float:
        return _jaccard(set(item1.topics), set(item2.topics))


def _host_decide(sim, scores, masks, *, max_candidates, similarity_threshold, dedup, quota, quotas, balance_factor):
    """The decision procedure of anr_index_diversify as a plain loop, for lists the library refuses (> 1024 candidates).
    -> (kept, selected) positions."""
    n = len(scores)
    kept: List[int] = []
    if dedup:
        for i in range(n):
            hit = next((p for p, k in enumerate(kept) if sim[i][k] >= similarity_threshold), None)
            if hit is None:
                kept.append(i)
            elif scores[i] > scores[kept[hit]]:
                del kept[hit]
                kept.append(i)
    else:
        kept = list(range(n))
    if len(kept) <= max_candidates:
        return kept, list(kept)
    srt = [kept[p] for p in sorted(range(len(kept)), key=lambda p: (-scores[kept[p]], p))]
    counts = [0] * 32
    types = [[t for t in range(32) if (int(masks[c]) >> t) & 1] for c in range(n)]
    selected: List[int] = []
    remaining = list(srt)
    if quota:
        for c in srt:
            if len(selected) >= max_candidates:
                break
            if any(counts[t] < quotas[t] for t in types[c]):
                selected.append(c)
                for t in types[c]:
                    counts[t] += 1
        chosen = set(selected)
        remaining = [c for c in srt if c not in chosen]
    else:
        selected.append(remaining.pop(0))
    while len(selected) < max_candidates and remaining:
        best, best_c = -1.0, None
        for c in remaining:
            gain = 1.0
            if selected:
                total = 0.0
                for s in selected:
                    total += sim[s][c]
                gain = 0.7 * (1.0 - total / len(selected)) + 0.3 * min(1.0, scores[c])
            value = gain
            if quota:
                bonus = 0.0
                for t in types[c]:
                    if quotas[t] > 0:
                        fill = counts[t] / quotas[t]
                        if fill < balance_factor:
                            bonus += (balance_factor - fill) * 0.5
                value = scores[c] * 0.5 + gain * 0.3 + bonus * 0.2
            if value > best:
                best, best_c = value, c
        if best_c is None:
            break
        selected.append(best_c)
        remaining.remove(best_c)
        for t in types[best_c]:
            counts[t] += 1
    return kept, selected


class DeduplicationProcessor:
    """Dedup of candidate items.  The semantic method needs the similarity machinery of the scheduler and is run by
    it (``DiversityScheduler._semantic_dedup``); used on its own, this class decides it on the host matrix."""

    def __init__(self, config: Dict[str, Any]):
        self.config = config.get("deduplication", {})
        self.method = DeduplicationMethod(self.config.get("method", "hybrid"))
        self.similarity_threshold = self.config.get("similarity_threshold", 0.85)
        self.hash_cache: Dict[str, str] = {}
        self.semantic_backend = None   # set by the scheduler: items -> kept items

    def deduplicate(self, candidates: List[CandidateItem]) -> Tuple[List[CandidateItem], Dict[str, int]]:
        if not candidates:
            return [], {"total": 0, "removed": 0, "kept": 0}
        n = len(candidates)
        if self.method == DeduplicationMethod.EXACT:
            out = self._exact_deduplication(candidates)
        elif self.method == DeduplicationMethod.FUZZY:
            out = self._fuzzy_deduplication(candidates)
        elif self.method == DeduplicationMethod.SEMANTIC:
            out = self._semantic_deduplication(candidates)
        elif self.method == DeduplicationMethod.HASH:
            out = self._hash_deduplication(candidates)
        else:
            out = self._hybrid_deduplication(candidates)
        return out, {"total": n, "removed": n - len(out), "kept": len(out)}

    @staticmethod
    def _first_of_each(candidates, key):
        seen, out = set(), []
        for c in candidates:
            k = key(c)
            if k not in seen:
                seen.add(k)
                out.append(c)
        return out

    def _exact_deduplication(self, candidates):
        return self._first_of_each(candidates, lambda c: c.content)

    def _hash_deduplication(self, candidates):
        return self._first_of_each(candidates, lambda c: c.content_hash)

    def _by_matrix(self, candidates, sim):
        kept, _ = _host_decide(sim, [c.score for c in candidates], [0] * len(candidates), max_candidates=len(candidates),
                               similarity_threshold=self.similarity_threshold, dedup=True, quota=False, quotas=[0] * 32,
                               balance_factor=0.0)
        return [candidates[i] for i in kept]

    def _fuzzy_deduplication(self, candidates):
        return self._by_matrix(candidates, _pair_matrix(candidates, lambda a, b: _word_similarity(a.content, b.content)))

    def _semantic_deduplication(self, candidates):
        if self.semantic_backend is not None:
            return self.semantic_backend(candidates)
        return self._by_matrix(candidates, _semantic_matrix(candidates))

    def _hybrid_deduplication(self, candidates):
        return self._semantic_deduplication(self._hash_deduplication(candidates))

    def _calculate_text_similarity(self, text1: str, text2: str) -> float:
        return _word_similarity(text1, text2)

    def _calculate_semantic_similarity(self, item1: CandidateItem, item2: CandidateItem) -> float:
        return _embedding_similarity(item1, item2)


_DEFAULTS = {"strategy": "hybrid", "max_candidates": 50, "diversity_threshold": 0.7, "deduplication_method": "hybrid",
             "similarity_threshold": 0.85}


def _load_config(config: Dict[str, Any]) -> Dict[str, Any]:
    """the inline ``diversity_scheduler`` section, overlaid with ``diversity_scheduler_config_file`` (JSON or YAML) when
    that file can be read; every key that is missing takes its default where it is used"""
    inline = dict(config.get("diversity_scheduler", {}) or {})
    path = config.get("diversity_scheduler_config_file")
    if path:
        try:
            import json
            import os
            if os.path.exists(path):
                with open(path, "r", encoding="utf-8") as f:
                    if path.endswith((".yaml", ".yml")):
                        import yaml
                        loaded = yaml.safe_load(f)
                    else:
                        loaded = json.load(f)
                if isinstance(loaded, dict):
                    inline.update(loaded)
        except Exception as e:  # an unreadable file leaves the inline section, as in the reference
            logger.warning(f"could not read {path}: {e}")
    return inline


class DiversityScheduler:
    def __init__(self, config: Dict[str, Any], vector_retriever=None, device: int = 0):
        self.config = _load_config(config)
        g = self.config.get
        self.diversity_config = DiversityConfig(
            strategy=DiversityStrategy(g("strategy", _DEFAULTS["strategy"])),
            max_candidates=g("max_candidates", _DEFAULTS["max_candidates"]),
            diversity_threshold=g("diversity_threshold", _DEFAULTS["diversity_threshold"]),
            deduplication_method=DeduplicationMethod(g("deduplication_method", _DEFAULTS["deduplication_method"])),
            similarity_threshold=g("similarity_threshold", _DEFAULTS["similarity_threshold"]))
        self.vector_retriever = vector_retriever
        self.device = int(device)
        self.deduplication_processor = DeduplicationProcessor(self.config)
        self.deduplication_processor.semantic_backend = self._semantic_dedup
        self.diversity_evaluators = self._initialize_evaluators()
        self.stats = self._zero_stats()
        self._lock = threading.Lock()
        self._last_selected_sim = None
        logger.info(f"DiversityScheduler initialized with strategy: {self.diversity_config.strategy.value}")

    @staticmethod
    def _zero_stats():
        return {"total_requests": 0, "candidates_processed": 0, "candidates_selected": 0, "duplicates_removed": 0,
                "average_diversity_score": 0.0}

    def _initialize_evaluators(self) -> Dict[str, DiversityEvaluator]:
        return {"semantic": SemanticDiversityEvaluator(self.config), "topical": TopicalDiversityEvaluator(self.config)}

    # -- the library call ------------------------------------------------------------------------------------------
    def _rows_of(self, items: List[CandidateItem]):
        """(flat index, row ids) when every item is a stored row of the retriever's flat index, else (None, None)"""
        vr = self.vector_retriever
        if vr is None or not items:
            return None, None
        from anorag_hip.flat_index import FlatIndex
        index = getattr(getattr(vr, "vector_index", None), "index", None)
        if not isinstance(index, FlatIndex):
            return None, None
        table = vr.note_id_to_index
        rows = [table.get(it.id, -1) for it in items]
        if any(r is None or r < 0 for r in rows):
            return None, None
        return index, rows

    def _decide(self, items, sim_rule, **kw):
        """one query through anr_index_diversify: stored rows when the rule is the semantic one and every item has a row,
        else the host matrix of ``sim_rule``.  -> (kept, selected, selected_sim or None)"""
        from anorag_hip.diversity import DiversityShapeError, diversify
        scores = [float(it.score) for it in items]
        masks, quotas = self._type_masks(items)
        index, rows = self._rows_of(items) if sim_rule == "semantic" else (None, None)
        sim = None
        try:
            if index is not None:
                try:
                    return diversify(index, [rows], [scores], [masks], quotas=quotas, **kw)[0]
                except DiversityShapeError as e:
                    logger.warning(f"stored rows refused ({e}); building the similarity matrix on the host")
            sim = _semantic_matrix(items) if sim_rule == "semantic" else _pair_matrix(
                items, self.diversity_evaluators["topical"].calculate_similarity)
            return diversify(None, None, [scores], [masks], quotas=quotas, sim=[sim], device=self.device, **kw)[0]
        except DiversityShapeError as e:
            logger.warning(f"the library refused the list ({e}); deciding it on the host")
            if sim is None:
                sim = _semantic_matrix(items)
            q = list(quotas) + [0] * (32 - len(quotas))
            kept, sel = _host_decide(sim, scores, masks, max_candidates=kw["max_candidates"],
                                     similarity_threshold=kw["similarity_threshold"], dedup=kw["dedup"], quota=kw["quota"],
                                     quotas=q, balance_factor=kw["balance_factor"])
            return np.array(kept, dtype=np.int64), np.array(sel, dtype=np.int64), sim[np.ix_(sel, sel)]

    def _type_masks(self, items):
        """evidence types as bits: the quota table's types first, in its order, then every other type seen"""
        names = list(self.diversity_config.evidence_type_quotas)
        for t in sorted({t for it in items for t in it.evidence_types} - set(names)):
            names.append(t)
        if len(names) > 32:
            raise ValueError("more than 32 evidence types")
        bit = {t: i for i, t in enumerate(names)}
        masks = [sum(1 << bit[t] for t in it.evidence_types) for it in items]
        quotas = [int(self.diversity_config.evidence_type_quotas.get(t, 0)) for t in names]
        return masks, quotas

    def _semantic_dedup(self, items: List[CandidateItem]) -> List[CandidateItem]:
        if not items:
            return []
        kept, _, _ = self._decide(items, "semantic", max_candidates=max(len(items), 1), dedup=True, quota=False,
                                  similarity_threshold=float(self.deduplication_processor.similarity_threshold),
                                  balance_factor=float(self.diversity_config.quota_balance_factor))
        return [items[int(i)] for i in kept]

    # -- the reference's flow --------------------------------------------------------------------------------------
    def schedule_candidates(self, candidates: List[Dict[str, Any]], query: Optional[str] = None,
                            context: Optional[Dict[str, Any]] = None) -> DiversityResult:
        start = time.time()
        context = context or {}
        with self._lock:
            self.stats["total_requests"] += 1
            self.stats["candidates_processed"] += len(candidates)
        items = self._convert_to_candidate_items(candidates)
        deduplicated, dedup_stats = self.deduplication_processor.deduplicate(items)
        selected = self._select_diverse_candidates(deduplicated, query, context)
        diversity_score = self._evaluate_overall_diversity(selected)
        coverage = self._calculate_coverage_metrics(selected)
        elapsed = time.time() - start
        with self._lock:
            self.stats["candidates_selected"] += len(selected)
            self.stats["duplicates_removed"] += dedup_stats["removed"]
            n, avg = self.stats["total_requests"], self.stats["average_diversity_score"]
            self.stats["average_diversity_score"] = (avg * (n - 1) + diversity_score) / n
        return DiversityResult(selected_candidates=selected, diversity_score=diversity_score, coverage_metrics=coverage,
                               deduplication_stats=dedup_stats, execution_time=elapsed,
                               metadata={"query": query, "context": context,
                                         "strategy": self.diversity_config.strategy.value})

    def _convert_to_candidate_items(self, candidates: List[Dict[str, Any]]) -> List[CandidateItem]:
        items = []
        for i, cand in enumerate(candidates):
            source_types = set()
            if "source_info" in cand:
                st = cand["source_info"].get("source_type", "")
                if st:
                    source_types.add(st)
            if "source_types" in cand:
                source_types.update(cand["source_types"])
            entities = cand.get("entities", [])
            content = cand.get("content", "")
            density = len(entities) / max(len(content.split()), 1) if content else 0.0
            meta = dict(cand.get("metadata", {}))
            meta["paragraph_idxs"] = cand.get("paragraph_idxs", [])
            items.append(CandidateItem(id=cand.get("id", f"candidate_{i}"), content=content, score=cand.get("score", 0.0),
                                       metadata=meta, entities=entities, topics=cand.get("topics", []),
                                       timestamp=cand.get("timestamp"), source=cand.get("source"),
                                       embedding=cand.get("embedding"), path_score=cand.get("path_score", 0.0),
                                       entity_density=density, source_types=source_types))
        return items

    def _select_diverse_candidates(self, candidates: List[CandidateItem], query: Optional[str],
                                   context: Dict[str, Any]) -> List[CandidateItem]:
        cfg = self.diversity_config
        self._last_selected_sim = None
        if len(candidates) <= cfg.max_candidates:
            return candidates
        candidates.sort(key=lambda x: x.score, reverse=True)   # the reference sorts the caller's list in place
        rule = "topical" if cfg.strategy == DiversityStrategy.TOPICAL else "semantic"
        _, sel, ks = self._decide(candidates, rule, max_candidates=int(cfg.max_candidates), dedup=False,
                                  quota=bool(cfg.enable_evidence_quota), similarity_threshold=float(cfg.similarity_threshold),
                                  balance_factor=float(cfg.quota_balance_factor))
        out = [candidates[int(i)] for i in sel]
        if rule == "semantic":
            self._last_selected_sim = (out, ks)
        return out

    def _select_with_evidence_quota(self, candidates, query, context):
        saved = self.diversity_config.enable_evidence_quota
        self.diversity_config.enable_evidence_quota = True
        try:
            return self._select_diverse_candidates(list(candidates), query, context)
        finally:
            self.diversity_config.enable_evidence_quota = saved

    def _calculate_quota_balance_bonus(self, candidate, current_counts, quotas) -> float:
        bonus, balance = 0.0, self.diversity_config.quota_balance_factor
        for t in candidate.evidence_types:
            quota = quotas.get(t, 0)
            if quota > 0:
                fill = current_counts.get(t, 0) / quota
                if fill < balance:
                    bonus += (balance - fill) * 0.5
        return bonus

    def _calculate_diversity_gain(self, current_selected, new_candidate) -> float:
        if not current_selected:
            return 1.0
        total = 0.0
        for s in current_selected:
            total += self._calculate_candidate_similarity(s, new_candidate)
        return 0.7 * (1.0 - total / len(current_selected)) + 0.3 * min(1.0, new_candidate.score)

    def _calculate_candidate_similarity(self, item1: CandidateItem, item2: CandidateItem) -> float:
        name = "topical" if self.diversity_config.strategy == DiversityStrategy.TOPICAL else "semantic"
        evaluator = self.diversity_evaluators.get(name)
        return evaluator.calculate_similarity(item1, item2) if evaluator else 0.0

    def _evaluate_overall_diversity(self, candidates: List[CandidateItem]) -> float:
        if not candidates:
            return 0.0
        last = self._last_selected_sim
        reuse = (last is not None and len(last[0]) == len(candidates)
                 and all(x is y for x, y in zip(last[0], candidates)))
        scores = []
        for name, evaluator in self.diversity_evaluators.items():
            if name == "semantic" and reuse and type(evaluator) is SemanticDiversityEvaluator:
                scores.append(evaluator.diversity_from_matrix(last[1]))   # the matrix the selection already produced
            else:
                scores.append(self._evaluate_with(name, evaluator, candidates))
        return sum(scores) / len(scores) if scores else 0.0

    def _evaluate_with(self, name, evaluator, candidates):
        if name == "semantic" and type(evaluator) is SemanticDiversityEvaluator and len(candidates) > 1:
            index, rows = self._rows_of(candidates)
            if index is not None:
                # stored rows: the K x K matrix through the library (no dedup, everything kept and returned)
                from anorag_hip.diversity import DiversityShapeError, diversify
                try:
                    _, sel, ks = diversify(index, [rows], [[0.0] * len(rows)], max_candidates=len(rows), dedup=False,
                                           similarity_threshold=2.0)[0]
                    return evaluator.diversity_from_matrix(ks)
                except DiversityShapeError:
                    pass
            return evaluator.diversity_from_matrix(_semantic_matrix(candidates))
        return evaluator.evaluate_diversity(candidates)

    def _calculate_coverage_metrics(self, candidates: List[CandidateItem]) -> Dict[str, float]:
        if not candidates:
            return {}
        metrics: Dict[str, float] = {}
        for key, attr in (("entity_coverage", "entities"), ("topic_coverage", "topics")):
            distinct, total = set(), 0
            for c in candidates:
                values = getattr(c, attr)
                distinct.update(values)
                total += len(values)
            metrics[key] = min(1.0, len(distinct) / max(1, total)) if total > 0 else 0.0
        sources = [c.source for c in candidates if c.source]
        metrics["source_coverage"] = len(set(sources)) / len(sources) if sources else 0.0
        stamps = [c.timestamp for c in candidates if c.timestamp]
        metrics["temporal_coverage"] = min(1.0, (max(stamps) - min(stamps)) / 86400) if len(stamps) > 1 else 0.0
        return metrics

    def get_stats(self) -> Dict[str, Any]:
        with self._lock:
            return self.stats.copy()

    def reset_stats(self) -> None:
        with self._lock:
            self.stats = self._zero_stats()
        logger.info("Statistics reset")


def create_diversity_scheduler(config: Dict[str, Any], vector_retriever=None) -> DiversityScheduler:
    return DiversityScheduler(config, vector_retriever=vector_retriever)


def create_diversity_config(strategy: str = "hybrid", **kwargs) -> DiversityConfig:
    return DiversityConfig(strategy=DiversityStrategy(strategy), max_candidates=kwargs.get("max_candidates", 50),
                           diversity_threshold=kwargs.get("diversity_threshold", 0.7),
                           deduplication_method=DeduplicationMethod(kwargs.get("deduplication_method", "hybrid")),
                           similarity_threshold=kwargs.get("similarity_threshold", 0.85))


def schedule_diverse_candidates(scheduler: DiversityScheduler, candidates: List[Dict[str, Any]],
                                query: Optional[str] = None) -> DiversityResult:
    return scheduler.schedule_candidates(candidates, query)


__all__ = ["DiversityScheduler", "DiversityConfig", "CandidateItem", "DiversityResult", "DiversityStrategy",
           "DeduplicationMethod", "CoverageMetric", "DiversityEvaluator", "SemanticDiversityEvaluator",
           "TopicalDiversityEvaluator", "DeduplicationProcessor", "create_diversity_scheduler", "create_diversity_config",
           "schedule_diverse_candidates"]
