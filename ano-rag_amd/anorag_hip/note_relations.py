"""The two integer O(N^2) passes of the reference's graph builder on the device.

``RelationExtractor._extract_basic_relations`` (graph/relation_extractor.py:104-147) runs on every build.  Two of its
passes are joins on set overlap and hold no floating point until their last division:

* ``entity_coexistence_relations`` replaces ``extract_entity_coexistence_relations`` (:418-481): every pair of notes that
  shares at least ``threshold`` entities, with the shared entities, their count and the Jaccard ratio.
* ``topic_relations`` replaces ``extract_topic_relations`` (:543-589) with ``_calculate_note_topic_similarity``
  (:738-767): every pair of notes inside a topic group, weighted by ``0.7 * keyword Jaccard + 0.3 * entity Jaccard``.

Both stand on ``SetJoin`` (csrc/setjoin.hip): the device returns integers only, and the reference's own
expressions turn them into floats on the host, so every float equals the reference's bit for bit.  Fails loudly when the
HIP library is missing; there is no CPU path here (a brute-force restatement lives in tests/setjoin_ref.py).
"""
from __future__ import annotations

import ctypes as C
import math
from collections import Counter
from typing import Any, Dict, Hashable, Iterable, List, Sequence, Tuple

import numpy as np

from . import _lib

STAT_NAMES = ("rows", "insertions", "pairs", "shared_ids", "rows_overflowed", "table_slots", "passes", "scratch_bytes")


def encode_rows(rows: Iterable[Iterable[Hashable]]) -> Tuple[List[Any], np.ndarray, np.ndarray]:
    """host half (no device): (items, indptr int64 [n+1], ids int32 [nnz]).  An item's id is its rank of first appearance
    over the rows in order; every row is de-duplicated and sorted by id."""
    index: Dict[Any, int] = {}
    items: List[Any] = []
    indptr = [0]
    ids: List[int] = []
    for row in rows:
        seen = set()
        for x in row:
            k = index.get(x)
            if k is None:
                k = index[x] = len(items)
                items.append(x)
            seen.add(k)
        ids.extend(sorted(seen))
        indptr.append(len(ids))
    return items, np.asarray(indptr, dtype=np.int64), np.asarray(ids, dtype=np.int32)


class SetJoin:
    """One family of sets on one device: ``rows`` is an iterable of iterables of hashable items."""

    def __init__(self, rows: Iterable[Iterable[Hashable]], device: int = 0):
        self._h = None
        self._lib = _lib.load()
        self.items, self.indptr, self.ids = encode_rows(rows)
        self.n_rows, self.device = len(self.indptr) - 1, int(device)
        h = C.c_void_p()
        _lib.check(self._lib.anr_setjoin_create(self.n_rows, len(self.items), self.indptr.ctypes.data, self.ids.ctypes.data,
                                                self.device, C.byref(h)), "anr_setjoin_create")
        self._h = h

    def set_table_slots(self, slots: int) -> None:
        """slots of the LDS table of ``cooccur`` (a power of two in [64, 4096]; 0 = default); results do not depend on it"""
        _lib.check(self._lib.anr_setjoin_set_option(self._h, _lib.SETJOIN_OPT_TABLE_SLOTS, int(slots)),
                   "anr_setjoin_set_option")

    def cooccur(self, min_common: int, return_stats: bool = False):
        """every pair i < j of rows with at least ``min_common`` shared items, sorted by (i, j):
        (I, J, inter, uni, common_ptr, common_items) — int32 except common_ptr (int64); the shared ids of pair p are
        ``common_items[common_ptr[p]:common_ptr[p + 1]]``, ascending.  With ``return_stats`` a dict of STAT_NAMES follows."""
        npairs, ncommon = C.c_int64(0), C.c_int64(0)
        stats = np.zeros(8, dtype=np.int64)
        _lib.check(self._lib.anr_setjoin_cooccur(self._h, int(min_common), C.byref(npairs), C.byref(ncommon),
                                                 stats.ctypes.data), "anr_setjoin_cooccur")
        out = self._fetch(npairs.value, ncommon.value)
        return out + (dict(zip(STAT_NAMES, (int(s) for s in stats))),) if return_stats else out

    def _fetch(self, npairs: int, ncommon: int):
        I, J, inter, uni = (np.empty(npairs, dtype=np.int32) for _ in range(4))
        ptr = np.empty(npairs + 1, dtype=np.int64)
        common = np.empty(ncommon, dtype=np.int32)
        _lib.check(self._lib.anr_setjoin_cooccur_fetch(self._h, I.ctypes.data, J.ctypes.data, inter.ctypes.data, uni.ctypes.data,
                                                       ptr.ctypes.data, common.ctypes.data), "anr_setjoin_cooccur_fetch")
        return I, J, inter, uni, ptr, common

    def pair_counts(self, I, J) -> Tuple[np.ndarray, np.ndarray]:
        """(inter, uni) int32 for the row pairs (I[p], J[p]): the sizes of the intersection and of the union"""
        I = np.ascontiguousarray(I, dtype=np.int32).reshape(-1)
        J = np.ascontiguousarray(J, dtype=np.int32).reshape(-1)
        if len(I) != len(J):
            raise ValueError("I and J must have one entry per pair")
        inter, uni = np.empty(len(I), dtype=np.int32), np.empty(len(I), dtype=np.int32)
        _lib.check(self._lib.anr_setjoin_pair_counts(self._h, len(I), I.ctypes.data, J.ctypes.data, inter.ctypes.data,
                                                     uni.ctypes.data), "anr_setjoin_pair_counts")
        return inter, uni

    def close(self) -> None:
        if self._h is not None:
            self._lib.anr_setjoin_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _note_ids(atomic_notes: Sequence[Dict[str, Any]]) -> List[Any]:
    ids = [note.get('note_id') for note in atomic_notes]
    if any(i is None for i in ids) or len(set(ids)) != len(ids):
        raise ValueError("entity_coexistence_relations: a note_id is missing or given twice; the reference keys this "
                         "method by note_id and merges such notes — keep the reference for this input")
    return ids


def entity_coexistence_relations(atomic_notes: Sequence[Dict[str, Any]], threshold=2, weight: float = 0.8,
                                 device: int = 0) -> List[Dict[str, Any]]:
    """extract_entity_coexistence_relations (relation_extractor.py:418-481).  ``threshold`` is
    ``graph.entity_cooccurrence_threshold`` and ``weight`` is ``relation_weights['entity_coexistence']``.  Same keys, nesting
    and types; the relations come ascending by (source index, target index) and ``common_entities`` in order of first
    appearance in the notes — the reference's order of both follows Python's string hashing."""
    ids = _note_ids(atomic_notes)
    min_common = max(int(math.ceil(threshold)), 1)  # `len(common) >= max(threshold, 1)` (:463) over integers
    with SetJoin((note.get('entities', []) for note in atomic_notes), device) as sj:
        I, J, inter, uni, ptr, common = sj.cooccur(min_common)
        names = sj.items
    relations = []
    I, J, inter, uni, ptr, common = I.tolist(), J.tolist(), inter.tolist(), uni.tolist(), ptr.tolist(), common.tolist()
    for p in range(len(I)):
        n_common = inter[p]
        relations.append({
            'source_id': ids[I[p]],
            'target_id': ids[J[p]],
            'relation_type': 'entity_coexistence',
            'weight': weight * min(n_common / 5.0, 1.0),
            'metadata': {
                'common_entities': [names[e] for e in common[ptr[p]:ptr[p + 1]]],
                'entity_count': n_common,
                'jaccard_similarity': n_common / uni[p],
            },
        })
    return relations


def topic_cohesion(notes: Sequence[Dict[str, Any]]) -> float:
    """_calculate_topic_cohesion (relation_extractor.py:713-736), the reference's host expression"""
    if len(notes) < 2:
        return 1.0
    all_keywords: List[Any] = []
    for note in notes:
        all_keywords.extend(note.get('keywords', []))
    if not all_keywords:
        return 0.5
    counts = Counter(all_keywords)
    unique = len(counts)
    repeated = sum(1 for c in counts.values() if c > 1)
    cohesion = repeated / unique if unique > 0 else 0.0
    return min(cohesion, 1.0)


def topic_groups(atomic_notes: Sequence[Dict[str, Any]]) -> Dict[Any, List[int]]:
    """the grouping of :547-556 as note indices: ``cluster_id`` unless it is None, else ``topic``; a falsy key (cluster 0,
    an empty topic) is dropped; groups in order of first appearance"""
    groups: Dict[Any, List[int]] = {}
    for i, note in enumerate(atomic_notes):
        cluster_id = note.get('cluster_id')
        key = cluster_id if cluster_id is not None else note.get('topic', '')
        if key:
            groups.setdefault(key, []).append(i)
    return groups


def note_similarity(kw_len_a, kw_len_b, kw_inter, kw_uni, ent_inter, ent_uni) -> np.ndarray:
    """_calculate_note_topic_similarity (:738-767) from the integer set sizes, float64 [n]"""
    kw_len_a, kw_len_b = np.asarray(kw_len_a), np.asarray(kw_len_b)
    kw_inter, kw_uni = np.asarray(kw_inter, dtype=np.float64), np.asarray(kw_uni, dtype=np.float64)
    ent_inter, ent_uni = np.asarray(ent_inter, dtype=np.float64), np.asarray(ent_uni, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        jac = np.where(kw_uni > 0, kw_inter / kw_uni, 0.0)
        ent = np.where(ent_uni > 0, ent_inter / ent_uni, 0.0)
    sim = np.minimum(0.7 * jac + 0.3 * ent, 1.0)
    sim = np.where((kw_len_a == 0) | (kw_len_b == 0), 0.1, sim)
    return np.where((kw_len_a == 0) & (kw_len_b == 0), 0.5, sim)


def topic_relations(atomic_notes: Sequence[Dict[str, Any]], weight: float = 0.7, device: int = 0) -> List[Dict[str, Any]]:
    """extract_topic_relations (relation_extractor.py:543-589) in the reference's order: groups in order of first
    appearance, pairs i < j inside a group.  ``weight`` is ``relation_weights['topic']``."""
    groups = [(key, idx) for key, idx in topic_groups(atomic_notes).items() if len(idx) >= 2]
    if not groups:
        return []
    I = np.concatenate([np.asarray(idx, dtype=np.int32)[np.triu_indices(len(idx), 1)[0]] for _, idx in groups])
    J = np.concatenate([np.asarray(idx, dtype=np.int32)[np.triu_indices(len(idx), 1)[1]] for _, idx in groups])
    with SetJoin((note.get('keywords', []) for note in atomic_notes), device) as kw:
        kw_inter, kw_uni = kw.pair_counts(I, J)
        kw_len = np.diff(kw.indptr)
    with SetJoin((note.get('entities', []) for note in atomic_notes), device) as ent:
        ent_inter, ent_uni = ent.pair_counts(I, J)
    sims = note_similarity(kw_len[I], kw_len[J], kw_inter, kw_uni, ent_inter, ent_uni).tolist()
    I, J = I.tolist(), J.tolist()
    relations = []
    p = 0
    for key, idx in groups:
        topic_weight = topic_cohesion([atomic_notes[i] for i in idx])
        topic = str(key)
        for _ in range(len(idx) * (len(idx) - 1) // 2):
            sim = sims[p]
            relations.append({
                'source_id': atomic_notes[I[p]].get('note_id'),
                'target_id': atomic_notes[J[p]].get('note_id'),
                'relation_type': 'topic_relation',
                'weight': weight * topic_weight * sim,
                'metadata': {
                    'topic': topic,
                    'topic_cohesion': topic_weight,
                    'note_similarity': sim,
                },
            })
            p += 1
    return relations
