"""Related notes on the device: ``NoteSimilarityCalculator.find_related_notes`` (utils/note_similarity.py:115-233).

The reference builds the N x N ``cosine_similarity`` matrix (:144) and then runs a Python double loop over all N^2 pairs
(:182-216): a cluster filter, entity Jaccard through ``set`` objects, a weighted sum, a threshold, a sort, the top
``max_related_notes``.  Here the pass is ``anr_index_related_notes`` (csrc/related.hip) on the stored rows of
a cosine ``FlatIndex``: an MFMA walk of the f16 image nominates the pairs that can still pass, a float64 kernel scores each
from the float32 rows and the sorted entity rows, and one wave per row keeps the first M.

* ``related_pairs`` is the thin binding: arrays in, arrays out.
* ``NoteSimilarityCalculator`` is the drop-in class: the reference's config keys and defaults, the same
  ``find_related_notes(notes)`` return value and the same ``compute_similarity_statistics``.  It loads no model of its
  own: the embeddings come from the caller's array (``embeddings=``) or from an encoder object (``EmbeddingManager`` with
  ``encode_texts``, ``SentenceEncoder`` with ``encode``).

``base_similarity`` is the float64 dot product of the index's normalised float32 rows; the reference's is sklearn's
float32 ``normalize`` + sgemm.  The two differ by float32 rounding (about 1e-7) and a pair whose combined score lies that
close to the threshold may be decided differently.  A repeated note id raises ``ValueError``: the
reference silently mis-indexes such input.  Fails loudly when the HIP library is missing; there is no CPU path here (a
brute-force restatement lives in tests/related_ref.py).
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .flat_index import METRIC_IP, FlatIndex
from .note_relations import encode_rows

STAT_NAMES = ("nominated", "scored", "kept", "strips", "pair_capacity", "band_resolved", "scratch_bytes", "reserved")
MAX_RELATED = 64


def set_pair_capacity(pairs: int) -> None:
    """pairs one nominating walk may hold (0 = default, from the free device memory); results never depend on it"""
    _lib.check(_lib.load().anr_related_set_option(_lib.RELATED_OPT_PAIR_CAP, int(pairs)), "anr_related_set_option")


def timing(enable: bool = True) -> Tuple[float, float, float]:
    """switch the developer timing of later calls; returns the last timed call's (walk, score, select) milliseconds"""
    ms = (C.c_float * 3)()
    _lib.check(_lib.load().anr_related_timing(int(bool(enable)), ms), "anr_related_timing")
    return float(ms[0]), float(ms[1]), float(ms[2])


def encode_clusters(values: Iterable[Any]) -> np.ndarray:
    """host half (no device): int32 codes that compare as the values do under ``==`` (:187, :199).  A value equal to -1
    keeps the code -1 ("no cluster"); every other value, ``None`` included, gets the rank of its first appearance."""
    codes: List[int] = []
    index: Dict[Any, int] = {}
    loose: List[Any] = []  # unhashable values, compared one by one
    for v in values:
        if v == -1:
            codes.append(-1)
            continue
        try:
            k = index.get(v)
            if k is None:
                k = index[v] = len(index) + len(loose)
        except TypeError:
            for k, u in loose:
                if u == v:
                    break
            else:
                k = len(index) + len(loose)
                loose.append((k, v))
        codes.append(k)
    return np.asarray(codes, dtype=np.int32)


def entity_similarity(inter: int, uni: int, len_a: int, len_b: int, min_shared: int) -> float:
    """_calculate_entity_similarity (:235-259) from the set sizes"""
    if not len_a and not len_b:
        return 0.5
    if not len_a or not len_b:
        return 0.0
    jaccard = inter / uni
    if inter >= min_shared:
        jaccard += 0.1
    return min(jaccard, 1.0)


def related_pairs(index: FlatIndex, entities: Sequence[Iterable[Any]], clusters: Optional[Sequence[Any]] = None, *,
                  threshold: float = 0.75, entity_weight: float = 0.3, min_shared: int = 1,
                  exclude_same_cluster: bool = True, cluster_bonus: float = 0.1, max_related: int = 5,
                  return_stats: bool = False):
    """The related rows of every stored row of a normalising inner-product ``FlatIndex``.  ``entities[i]`` is row i's
    entity collection (any hashables), ``clusters[i]`` its cluster id (``None``: no row has one).  Returns a dict of
    arrays: ``nbr`` int32 [n, M] (-1 beyond ``n_nbr``), ``n_nbr`` int32 [n], ``combined`` / ``base`` float64 [n, M],
    ``inter`` / ``uni`` int32 [n, M], ``ent_len`` int64 [n] (distinct entities per row); with ``return_stats`` the dict
    also holds ``stats`` (STAT_NAMES)."""
    n, M = index.ntotal, int(max_related)
    _, indptr, ids = encode_rows(entities)
    if len(indptr) - 1 != n:
        raise ValueError(f"{len(indptr) - 1} entity rows for an index of {n} rows")
    codes = None
    if clusters is not None:
        codes = encode_clusters(clusters)
        if len(codes) != n:
            raise ValueError(f"{len(codes)} cluster ids for an index of {n} rows")
    params = _lib.RelatedParams(float(threshold), float(entity_weight), float(cluster_bonus), int(min_shared),
                                int(bool(exclude_same_cluster)), M, 0)
    rows = max(n, 0) * max(M, 0)
    out = {"nbr": np.full(rows, -1, dtype=np.int32), "n_nbr": np.zeros(n, dtype=np.int32),
           "combined": np.zeros(rows, dtype=np.float64), "base": np.zeros(rows, dtype=np.float64),
           "inter": np.zeros(rows, dtype=np.int32), "uni": np.zeros(rows, dtype=np.int32)}
    stats = np.zeros(8, dtype=np.int64)
    _lib.check(index._lib.anr_index_related_notes(
        index._h, C.byref(params), codes.ctypes.data if codes is not None else None, indptr.ctypes.data, ids.ctypes.data,
        out["nbr"].ctypes.data, out["n_nbr"].ctypes.data, out["combined"].ctypes.data, out["base"].ctypes.data,
        out["inter"].ctypes.data, out["uni"].ctypes.data, stats.ctypes.data), "anr_index_related_notes")
    for k in ("nbr", "combined", "base", "inter", "uni"):
        out[k] = out[k].reshape(n, M)
    out["ent_len"] = np.diff(indptr)
    if return_stats:
        out["stats"] = dict(zip(STAT_NAMES, (int(s) for s in stats)))
    return out


def note_id(note: Dict[str, Any]) -> Any:
    """the reference's key of a note (:75, :132, :150, :224)"""
    return note.get('id', str(hash(note.get('content', ''))))


def shape_related(valid_notes: Sequence[Dict[str, Any]], res: Dict[str, np.ndarray], min_shared: int) -> List[List[Dict[str, Any]]]:
    """host half (no device): the ``related_notes`` lists of :221-231 from the arrays of ``related_pairs``"""
    nbr, cnt = res["nbr"].tolist(), res["n_nbr"].tolist()
    comb, base = res["combined"].tolist(), res["base"].tolist()
    inter, uni, ent_len = res["inter"].tolist(), res["uni"].tolist(), res["ent_len"].tolist()
    out = []
    for i in range(len(valid_notes)):
        related = []
        for t in range(cnt[i]):
            j = nbr[i][t]
            note = valid_notes[j]
            related.append({
                'id': note_id(note),
                'title': note.get('content', '')[:50] + '...',
                'similarity': round(comb[i][t], 3),
                'base_similarity': round(base[i][t], 3),
                'entity_similarity': round(entity_similarity(inter[i][t], uni[i][t], ent_len[i], ent_len[j], min_shared), 3),
                'cluster_id': note.get('cluster_id', -1),
            })
        out.append(related)
    return out


class NoteSimilarityCalculator:
    """Drop-in for the reference's class of the same name (utils/note_similarity.py:11): same config keys and defaults,
    same ``find_related_notes`` result.  ``encoder``: an object with ``encode_texts(texts)`` or ``encode(texts)``
    returning an [n, d] array; alternatively every call passes ``embeddings=``."""

    def __init__(self, config: Optional[Dict[str, Any]] = None, encoder: Any = None, device: int = 0):
        self.config = config or {}
        self.model_name = self.config.get('model_name', 'all-MiniLM-L6-v2')
        self.similarity_threshold = self.config.get('similarity_threshold', 0.75)
        self.max_related_notes = self.config.get('max_related_notes', 5)
        self.batch_size = self.config.get('batch_size', 32)
        self.use_content = self.config.get('use_content', True)
        self.use_summary = self.config.get('use_summary', True)
        self.content_weight = self.config.get('content_weight', 0.6)
        self.summary_weight = self.config.get('summary_weight', 0.4)
        self.entity_similarity_weight = self.config.get('entity_similarity_weight', 0.3)
        self.min_shared_entities = self.config.get('min_shared_entities', 1)
        self.exclude_same_cluster = self.config.get('exclude_same_cluster', True)
        self.cluster_similarity_bonus = self.config.get('cluster_similarity_bonus', 0.1)
        self.encoder = encoder
        self.device = int(device)
        self.last_stats: Dict[str, int] = {}

    def _prepare_text_for_encoding(self, note: Dict[str, Any]) -> str:
        """:261-280"""
        texts = []
        if self.use_content and note.get('content'):
            content = note['content'].strip()
            if content:
                texts.append(content)
        if not texts and note.get('keywords'):
            keywords = note['keywords']
            if isinstance(keywords, list):
                texts.append(' '.join(keywords))
            elif isinstance(keywords, str):
                texts.append(keywords)
        return ' '.join(texts) if texts else ''

    def _encode(self, texts: List[str]) -> np.ndarray:
        if self.encoder is None:
            raise ValueError("NoteSimilarityCalculator: pass embeddings= or construct with an encoder "
                             "(EmbeddingManager / SentenceEncoder); the class loads no model of its own")
        if hasattr(self.encoder, 'encode_texts'):
            return np.asarray(self.encoder.encode_texts(texts))
        return np.asarray(self.encoder.encode(texts, batch_size=self.batch_size))

    def find_related_notes(self, notes: List[Dict[str, Any]], embeddings=None) -> List[Dict[str, Any]]:
        """:115-167.  ``embeddings``: [len(notes), d], row k for ``notes[k]`` (rows of notes without text are ignored).
        A note without text is no candidate and gets ``related_notes: []``; with fewer than two notes with text the
        input is returned unchanged, as the reference does."""
        ids = [note_id(note) for note in notes]
        try:
            repeated = len(set(ids)) != len(ids)
        except TypeError:
            repeated = any(ids[a] == ids[b] for a in range(len(ids)) for b in range(a))
        if repeated:
            raise ValueError("find_related_notes: a note id is given twice; the reference keys its matrix rows by id and "
                             "mis-indexes such notes")
        valid = [k for k, note in enumerate(notes) if self._prepare_text_for_encoding(note)]
        if len(valid) < 2:
            return notes
        if embeddings is None:
            emb = self._encode([self._prepare_text_for_encoding(notes[k]) for k in valid])
            if emb.ndim != 2 or emb.shape[0] != len(valid):
                raise ValueError(f"the encoder returned shape {emb.shape} for {len(valid)} texts")
        else:
            emb = np.asarray(embeddings)
            if emb.ndim != 2 or emb.shape[0] != len(notes):
                raise ValueError(f"embeddings: expected one row per note ({len(notes)}), got shape {emb.shape}")
            emb = emb[valid]
        valid_notes = [notes[k] for k in valid]
        index = FlatIndex(emb.shape[1], METRIC_IP, normalize=True, device=self.device)
        try:
            index.add(np.ascontiguousarray(emb, dtype=np.float32))
            res = related_pairs(index, [note.get('entities', []) for note in valid_notes],
                                [note.get('cluster_id', -1) for note in valid_notes],
                                threshold=self.similarity_threshold, entity_weight=self.entity_similarity_weight,
                                min_shared=self.min_shared_entities, exclude_same_cluster=self.exclude_same_cluster,
                                cluster_bonus=self.cluster_similarity_bonus, max_related=self.max_related_notes,
                                return_stats=True)
        finally:
            index.close()
        self.last_stats = res["stats"]
        related = shape_related(valid_notes, res, self.min_shared_entities)
        position = {k: r for r, k in enumerate(valid)}
        enhanced_notes = []
        for k, note in enumerate(notes):
            enhanced = note.copy()
            enhanced['related_notes'] = related[position[k]] if k in position else []
            enhanced_notes.append(enhanced)
        return enhanced_notes

    def compute_similarity_statistics(self, notes: List[Dict[str, Any]]) -> Dict[str, Any]:
        """:287-328, host only"""
        total_notes = len(notes)
        notes_with_relations = sum(1 for note in notes if note.get('related_notes'))
        total_relations = sum(len(note.get('related_notes', [])) for note in notes)
        similarities = []
        for note in notes:
            for related in note.get('related_notes', []):
                similarities.append(related.get('similarity', 0))
        cross_cluster_relations = 0
        same_cluster_relations = 0
        for note in notes:
            note_cluster = note.get('cluster_id', -1)
            for related in note.get('related_notes', []):
                if note_cluster != related.get('cluster_id', -1):
                    cross_cluster_relations += 1
                else:
                    same_cluster_relations += 1
        return {
            'total_notes': total_notes,
            'notes_with_relations': notes_with_relations,
            'total_relations': total_relations,
            'avg_relations_per_note': total_relations / max(total_notes, 1),
            'coverage_rate': notes_with_relations / max(total_notes, 1),
            'cross_cluster_relations': cross_cluster_relations,
            'same_cluster_relations': same_cluster_relations,
            'similarity_stats': {
                'mean': np.mean(similarities) if similarities else 0,
                'std': np.std(similarities) if similarities else 0,
                'min': np.min(similarities) if similarities else 0,
                'max': np.max(similarities) if similarities else 0,
            },
        }


__all__ = ["NoteSimilarityCalculator", "related_pairs", "encode_clusters", "entity_similarity", "shape_related",
           "set_pair_capacity", "timing", "STAT_NAMES", "MAX_RELATED"]
