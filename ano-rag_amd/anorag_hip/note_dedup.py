"""Duplicate notes on the device: ``NoteValidator.detect_duplicate_notes`` (utils/note_validator.py:1037-1086).

``semantic_duplicates`` keeps the reference's vectoriser call and replaces the dense N x N ``cosine_similarity`` matrix and
the i < j loop of ``_find_semantic_duplicates`` (:363-393) by ``TfidfJoin.duplicates`` (csrc/tfidf.hip), whose values equal
sklearn's bit for bit; the set-Jaccard loops of ``_find_entity_duplicates`` (:420-440) and ``_find_lexical_duplicates``
(:395-418) go through ``SetJoin.cooccur(1)`` and divide the two integers on the host as the reference does.  Why the bits
agree (the stored order of a vectoriser's rows, ``relabel_terms``, the ascending merge): DESIGN.md §5o.  Fails loudly
when the HIP library is missing; there is no CPU path for the joins (a numpy restatement lives in tests/tfidf_ref.py).
"""
from __future__ import annotations

import ctypes as C
import hashlib
from typing import Any, Dict, List, Sequence, Set, Tuple

import numpy as np

from . import _lib
from .compat import logger
from .note_relations import SetJoin

STAT_NAMES = ("rows", "insertions", "pairs_nominated", "pairs_kept", "rows_overflowed", "table_slots", "nominate_us",
              "decide_us")


def _csr_arrays(csr) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int, int]:
    """(indptr int64, indices int64, data float64, n_rows, n_cols) of a scipy CSR, or of any object with its attributes"""
    if getattr(csr, "format", "csr") != "csr":
        raise ValueError("a CSR matrix is expected")
    n_rows, n_cols = (int(v) for v in csr.shape)
    indptr = np.ascontiguousarray(csr.indptr, dtype=np.int64)
    indices = np.ascontiguousarray(csr.indices, dtype=np.int64)
    data = np.asarray(csr.data)
    if data.dtype != np.float64:
        raise ValueError(f"float64 values are expected, not {data.dtype}")
    data = np.ascontiguousarray(data)
    if len(indptr) != n_rows + 1 or indptr[0] != 0 or len(indices) != indptr[-1] or len(data) != indptr[-1]:
        raise ValueError("inconsistent CSR arrays")
    if np.any(np.diff(indptr) < 0):
        raise ValueError("indptr descends")
    if len(indices) and (indices.min() < 0 or indices.max() >= n_cols):
        raise ValueError("a column index is outside the matrix")
    return indptr, indices, data, n_rows, n_cols


def normalize_rows(indptr: np.ndarray, data: np.ndarray) -> np.ndarray:
    """sklearn's ``normalize(X, copy=True)`` for a CSR (``inplace_csr_row_normalize_l2``): the squares of a row added one at
    a time in stored order, the square root, one division per value; an all-zero row is left alone.  Returns new values."""
    lens = np.diff(indptr)
    sq = np.zeros(len(lens), dtype=np.float64)
    for p in range(int(lens.max()) if len(lens) else 0):  # position p of every row that has one: sequential per row
        rows = np.flatnonzero(lens > p)
        v = data[indptr[rows] + p]
        sq[rows] = sq[rows] + v * v
    norm = np.sqrt(sq)
    norm[norm == 0.0] = 1.0
    return data / np.repeat(norm, lens)


def relabel_terms(csr) -> Tuple[np.ndarray, np.ndarray]:
    """(terms int32 [nnz], label int32 [n_cols]): ``label[c]`` is the rank of column c by the key (first row that holds it,
    position in that row) — columns no row holds follow in column order — and ``terms = label[csr.indices]``.  Every row
    must be strictly ascending in the new labels: a matrix one vectoriser made is; ``ValueError`` otherwise (rows that hold
    two terms in opposite orders have no single global order, and no merge reproduces the product's sums)."""
    indptr, indices, _, n_rows, n_cols = _csr_arrays(csr)
    lens = np.diff(indptr)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), lens)
    pos = np.arange(len(indices), dtype=np.int64) - indptr[rows]
    width = int(lens.max()) + 1 if n_rows and len(indices) else 1
    never = np.iinfo(np.int64).max
    first = np.full(n_cols, never, dtype=np.int64)
    np.minimum.at(first, indices, rows * width + pos)
    order = np.argsort(first, kind="stable")
    label = np.empty(n_cols, dtype=np.int32)
    label[order] = np.arange(n_cols, dtype=np.int32)
    terms = label[indices]
    if len(terms) > 1:
        inside = np.ones(len(terms), dtype=bool)   # entry k and k - 1 lie in the same row
        inside[indptr[:-1][lens > 0]] = False
        bad = np.flatnonzero(inside[1:] & (terms[1:] <= terms[:-1]))
        if len(bad):
            r = int(np.searchsorted(indptr, bad[0] + 1, side="right") - 1)
            raise ValueError(f"row {r} does not ascend in the first-seen order of the terms (or repeats a term): the rows "
                             "have no single global order; a matrix made by one vectoriser has")
    return np.ascontiguousarray(terms, dtype=np.int32), label


class TfidfJoin:
    """One sparse float64 matrix (rows = notes, columns = terms) on one device.  ``csr`` is a scipy CSR as
    ``TfidfVectorizer.fit_transform`` returns it (or any object with ``shape``, ``indptr``, ``indices``, ``data``); the rows
    are re-normalised as ``cosine_similarity`` does and the terms relabelled on the host."""

    def __init__(self, csr, device: int = 0):
        self._h = None
        self._lib = _lib.load()
        self.indptr, _, data, self.n_rows, self.n_cols = _csr_arrays(csr)
        self.values = normalize_rows(self.indptr, data)
        self.terms, self.label = relabel_terms(csr)
        self.device = int(device)
        h = C.c_void_p()
        _lib.check(self._lib.anr_tfidf_create(self.device, self.n_rows, self.n_cols, self.indptr.ctypes.data,
                                              self.terms.ctypes.data, self.values.ctypes.data, C.byref(h)),
                   "anr_tfidf_create")
        self._h = h

    def set_table_slots(self, slots: int) -> None:
        """slots of the LDS table of ``duplicates`` (a power of two in [64, 4096]; 0 = default); results do not depend on it"""
        _lib.check(self._lib.anr_tfidf_set_option(self._h, _lib.TFIDF_OPT_TABLE_SLOTS, int(slots)), "anr_tfidf_set_option")

    def duplicates(self, threshold: float, return_stats: bool = False):
        """every pair i < j of rows with cosine >= ``threshold`` (0 < threshold <= 2), sorted by (i, j):
        (I int32, J int32, sim float64) — sim[p] is ``cosine_similarity(csr)[I[p], J[p]]`` bit for bit.  With
        ``return_stats`` a dict of STAT_NAMES follows."""
        npairs = C.c_int64(0)
        stats = np.zeros(8, dtype=np.int64)
        _lib.check(self._lib.anr_tfidf_self_join(self._h, float(threshold), C.byref(npairs), stats.ctypes.data),
                   "anr_tfidf_self_join")
        I, J = np.empty(npairs.value, dtype=np.int32), np.empty(npairs.value, dtype=np.int32)
        sim = np.empty(npairs.value, dtype=np.float64)
        _lib.check(self._lib.anr_tfidf_self_join_fetch(self._h, I.ctypes.data, J.ctypes.data, sim.ctypes.data),
                   "anr_tfidf_self_join_fetch")
        return (I, J, sim, dict(zip(STAT_NAMES, (int(s) for s in stats)))) if return_stats else (I, J, sim)

    def scores(self, query_csr) -> np.ndarray:
        """``cosine_similarity(query_csr, csr)``: float64 [n_queries][n_rows].  ``query_csr`` is what the same vectoriser's
        ``transform`` returns (column ids ascending inside a row); it is re-normalised as sklearn does."""
        q_indptr, q_indices, q_data, nq, q_cols = _csr_arrays(query_csr)
        if q_cols != self.n_cols:
            raise ValueError(f"the queries have {q_cols} columns, the matrix {self.n_cols}")
        weights = normalize_rows(q_indptr, q_data)
        terms = np.ascontiguousarray(self.label[q_indices], dtype=np.int32)
        out = np.zeros((nq, self.n_rows), dtype=np.float64)
        _lib.check(self._lib.anr_tfidf_scores(self._h, nq, q_indptr.ctypes.data, terms.ctypes.data, weights.ctypes.data,
                                              out.ctypes.data), "anr_tfidf_scores")
        return out

    def close(self) -> None:
        if self._h is not None:
            self._lib.anr_tfidf_destroy(self._h)
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


def _jaccard_duplicates(atomic_notes: Sequence[Dict[str, Any]], sets: List[set], threshold, device: int):
    """the loop shared by :395-418 and :420-440: pairs i < j of non-empty sets with len(a & b) / len(a | b) >= threshold"""
    duplicates = []
    if threshold <= 0:  # a pair without a shared item passes too: the join never looks at one, keep the reference's loop
        for i, a in enumerate(sets):
            for j in range(i + 1, len(sets)):
                b = sets[j]
                if not a or not b:
                    continue
                similarity = len(a & b) / len(a | b)
                if similarity >= threshold:
                    duplicates.append((atomic_notes[i].get('note_id', ''), atomic_notes[j].get('note_id', ''), similarity))
        return duplicates
    with SetJoin(sets, device) as sj:
        I, J, inter, uni, _, _ = sj.cooccur(1)
    for i, j, n_inter, n_uni in zip(I.tolist(), J.tolist(), inter.tolist(), uni.tolist()):
        similarity = n_inter / n_uni   # two non-empty sets: the union is not empty
        if similarity >= threshold:
            duplicates.append((atomic_notes[i].get('note_id', ''), atomic_notes[j].get('note_id', ''), similarity))
    return duplicates


def lexical_duplicates(atomic_notes: Sequence[Dict[str, Any]], threshold: float = 0.85,
                       device: int = 0) -> List[Tuple[Any, Any, float]]:
    """_find_lexical_duplicates (:395-418): Jaccard of the lower-cased whitespace-split word sets"""
    return _jaccard_duplicates(atomic_notes, [set(note.get('content', '').lower().split()) for note in atomic_notes],
                               threshold, device)


def entity_duplicates(atomic_notes: Sequence[Dict[str, Any]], threshold: float = 0.8,
                      device: int = 0) -> List[Tuple[Any, Any, float]]:
    """_find_entity_duplicates (:420-440): Jaccard of the entity sets"""
    return _jaccard_duplicates(atomic_notes, [set(note.get('entities', [])) for note in atomic_notes], threshold, device)


def semantic_duplicates(atomic_notes: Sequence[Dict[str, Any]], threshold: float = 0.85,
                        device: int = 0) -> List[Tuple[Any, Any, Any]]:
    """_find_semantic_duplicates (:363-393): (note_id_i, note_id_j, similarity) for every i < j with TF-IDF cosine >=
    threshold, in (i, j) order, the values np.float64 as the reference's matrix entries are.  When the vectoriser raises
    (an empty vocabulary) the lexical duplicates are returned, as the reference does; a failure of the device is not
    swallowed."""
    from sklearn.feature_extraction.text import TfidfVectorizer
    contents = [note.get('content', '') for note in atomic_notes]
    note_ids = [note.get('note_id', '') for note in atomic_notes]
    if len(contents) < 2:
        return []
    try:
        tfidf_matrix = TfidfVectorizer(stop_words='english', max_features=1000).fit_transform(contents)
    except Exception as e:
        logger.warning(f"Failed to compute semantic similarity: {e}")
        return lexical_duplicates(atomic_notes, threshold, device)
    if not threshold > 0:  # pairs that share no term pass as well: only the dense matrix lists them
        from sklearn.metrics.pairwise import cosine_similarity
        similarity_matrix = cosine_similarity(tfidf_matrix)
        return [(note_ids[i], note_ids[j], similarity_matrix[i][j]) for i in range(len(contents))
                for j in range(i + 1, len(contents)) if similarity_matrix[i][j] >= threshold]
    with TfidfJoin(tfidf_matrix, device) as join:
        I, J, sim = join.duplicates(threshold)
    return [(note_ids[i], note_ids[j], s) for i, j, s in zip(I.tolist(), J.tolist(), sim)]


def exact_duplicates(atomic_notes: Sequence[Dict[str, Any]]) -> Dict[str, List[Any]]:
    """_find_exact_duplicates (:351-361): md5 of the content -> the note ids that carry it, groups of two or more, in order
    of first appearance"""
    groups: Dict[str, List[Any]] = {}
    for note in atomic_notes:
        digest = hashlib.md5(note.get('content', '').encode('utf-8')).hexdigest()
        groups.setdefault(digest, []).append(note.get('note_id', ''))
    return {digest: ids for digest, ids in groups.items() if len(ids) > 1}


def merge_duplicate_results(exact: Dict[str, List[Any]], semantic, entity) -> Dict[Any, Set[Any]]:
    """_merge_duplicate_results (:442-463): primary note id -> the ids it makes redundant; the first note of an exact group
    and the earlier note of every pair are the primaries"""
    merged: Dict[Any, Set[Any]] = {}
    for ids in exact.values():
        for other in ids[1:]:
            merged.setdefault(ids[0], set()).add(other)
    for pairs in (semantic, entity):
        for first, second, _ in pairs:
            merged.setdefault(first, set()).add(second)
    return merged


def deduplicate_notes(atomic_notes: Sequence[Dict[str, Any]], duplicates: Dict[Any, Set[Any]]) -> List[Dict[str, Any]]:
    """_deduplicate_notes (:465-481): the notes no primary makes redundant, in order; a surviving primary receives
    ``duplicates_removed`` (written into the caller's dict, as the reference does)"""
    redundant: Set[Any] = set()
    for ids in duplicates.values():
        redundant |= ids
    kept = []
    for note in atomic_notes:
        note_id = note.get('note_id', '')
        if note_id in redundant:
            continue
        if note_id in duplicates:
            note['duplicates_removed'] = list(duplicates[note_id])
        kept.append(note)
    return kept


def detect_duplicate_notes(atomic_notes: Sequence[Dict[str, Any]], device: int = 0) -> Dict[str, Any]:
    """NoteValidator.detect_duplicate_notes (:1037-1086): the same dict — keys, their order, the status rule (duplicate
    rate above 0.3 fails, above 0.1 warns) and the 'error' branch."""
    try:
        exact = exact_duplicates(atomic_notes)
        semantic = semantic_duplicates(atomic_notes, device=device)
        entity = entity_duplicates(atomic_notes, device=device)
        merged = merge_duplicate_results(exact, semantic, entity)
        kept = deduplicate_notes(atomic_notes, merged)
        removed = sum(len(ids) for ids in merged.values())
        rate = removed / max(len(atomic_notes), 1)
        status = 'failed' if rate > 0.3 else 'warning' if rate > 0.1 else 'passed'
        return {
            'status': status,
            'exact_duplicates': exact,
            'semantic_duplicates': semantic,
            'entity_duplicates': entity,
            'deduplicated_notes': kept,
            'duplicate_rate': rate,
            'removed_count': removed,
            'remaining_count': len(kept),
        }
    except Exception as e:
        logger.error(f"Duplicate detection failed: {e}")
        return {
            'status': 'error',
            'error': str(e),
            'exact_duplicates': {},
            'semantic_duplicates': [],
            'entity_duplicates': [],
            'deduplicated_notes': atomic_notes,
        }
