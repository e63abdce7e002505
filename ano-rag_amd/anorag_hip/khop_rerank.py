"""The second hop of the reference's multi-hop query path on the device: the rerank of
``QueryProcessor._rerank_khop_candidates`` (query/query_processor.py:1549-1635) and the near-duplicate suppression of
``_apply_cluster_suppression`` (:1637-1697), for a batch of queries with ragged candidate lists.

``rerank_khop`` is ``anr_index_khop_rerank``: the dense and the focused cosine of every candidate from the index's stored
rows, the three rankings, the RRF bonus, the final score and the stable order, float64 in the reference's order of
operations.  ``cluster_suppression`` is ``anr_index_cluster_suppress``: the greedy suppression on the float64 cosines of
the stored rows.  With ``dense=`` / ``sim=`` those values are the caller's and no index is needed.

OPT-IN: nothing in the reference's call path is replaced by importing this module — the reference
re-encodes every candidate's text for the dense and the focused score, stored embeddings change the scores.

Everything here fails loudly when the HIP library is missing; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import KhopParams

MAX_CANDIDATES_PER_QUERY = 1024
EINVAL = -1
RRF_K = 50.0   # _rrf_score's k (:1603)


class KhopShapeError(_lib.AnoragError):
    """The call was refused as ANR_EINVAL (a list longer than 1024 candidates, a row id outside the index, a NaN, ...)."""


def _ragged(lists, dtype, offs, what):
    arrs = [np.asarray(a, dtype=dtype).reshape(-1) for a in lists]
    if len(arrs) != len(offs) - 1 or any(a.size != n for a, n in zip(arrs, np.diff(offs))):
        raise ValueError(f"{what}: one entry per candidate of every query")
    flat = np.concatenate(arrs) if arrs else np.zeros(0, dtype=dtype)
    return np.ascontiguousarray(flat, dtype=dtype)


def _offsets(lists):
    offs = np.zeros(len(lists) + 1, dtype=np.int64)
    if len(lists):
        offs[1:] = np.cumsum([len(a) for a in lists])
    return offs


def check_unique_note_ids(note_ids):
    """The reference keys its rank dicts by note_id (:1593): a query whose candidates repeat one is not this arithmetic."""
    for q, ids in enumerate(note_ids):
        if len(set(ids)) != len(ids):
            raise ValueError(f"query {q}: candidates repeat a note_id; the reference ranks by note_id, keep the reference "
                             "for such input")


def decay_factors(hop_decay: float, hop_no: Sequence[int]) -> List[float]:
    """what every final score is multiplied by (:1628-1629), with Python's own ``**``; 1.0 where the reference does not
    multiply (hop_no <= 1, or hop_decay outside (0, 1))"""
    hop_decay = float(hop_decay)
    return [hop_decay ** (int(h) - 1) if (int(h) > 1 and 0.0 < hop_decay < 1.0) else 1.0 for h in hop_no]


def _ptr(x):
    return x.ctypes.data if x is not None else None


def rerank_khop(index, rows, bm25, is_prf, prf_sim, cov, cons, hop_no, *, query_vecs=None, focus_vecs=None, has_focus=None,
                dense=None, focused=None, hop_decay=0.85, dense_weight=1.0, bm25_weight=0.6, focused_weight_hop2=0.30,
                cov_weight=0.10, cons_weight=0.05, rrf_lambda=0.2, rrf_k=RRF_K, note_ids=None,
                device=0) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
    """Rerank, per query.

    Ragged inputs, one sequence per query and one entry per candidate: ``rows`` (index row ids; ignored, and may be
    ``None``, when ``dense`` is given), ``bm25``, ``is_prf`` (retrieval_method == "prf_bridge"), ``prf_sim`` (the
    candidate's similarity_score), ``cov`` / ``cons`` (_compute_cov_cons), ``hop_no``.  Per query: ``query_vecs`` [nq, d]
    float32, ``focus_vecs`` [nq, d] or ``None``, ``has_focus`` [nq] bools (default: every query, when focus_vecs is given).
    ``dense`` / ``focused``: ragged float64 scores used instead of the cosines of the stored rows (``index`` may then be
    ``None``; the call runs on ``device``).  ``note_ids``: ragged ids, only checked: a query that repeats one raises
    ``ValueError``.

    Returns, per query, ``(dense, focused, final, order)``: float64 arrays by candidate, and the candidate positions best
    first (stable)."""
    lib = _lib.load()
    if note_ids is not None:
        check_unique_note_ids(note_ids)
    offs = _offsets(bm25)
    nq, total = len(offs) - 1, int(offs[-1])
    hop_lists = [[int(h) for h in hs] for hs in hop_no]
    a_bm25 = _ragged(bm25, np.float64, offs, "bm25")
    a_prf = _ragged(is_prf, np.uint8, offs, "is_prf")
    a_psim = _ragged(prf_sim, np.float64, offs, "prf_sim")
    a_cov = _ragged(cov, np.float64, offs, "cov")
    a_cons = _ragged(cons, np.int32, offs, "cons")
    a_hop = _ragged(hop_lists, np.int32, offs, "hop_no")
    a_decay = _ragged([decay_factors(hop_decay, hs) for hs in hop_lists], np.float64, offs, "hop_no")
    a_rows = a_q = a_f = a_hf = a_dense = a_foc = None
    if dense is not None:
        a_dense = _ragged(dense, np.float64, offs, "dense")
        if focused is not None:
            a_foc = _ragged(focused, np.float64, offs, "focused")
    else:
        if index is None:
            raise ValueError("rerank_khop needs an index or dense=")
        a_rows = _ragged(rows, np.int64, offs, "rows")
        a_q = np.ascontiguousarray(query_vecs, dtype=np.float32)
        if a_q.ndim != 2 or a_q.shape != (nq, index.d):
            raise ValueError("query_vecs: one [dim] float32 vector per query")
        if focus_vecs is not None:
            a_f = np.ascontiguousarray(focus_vecs, dtype=np.float32)
            if a_f.shape != a_q.shape:
                raise ValueError("focus_vecs: the shape of query_vecs")
            a_hf = (np.ones(nq, dtype=np.uint8) if has_focus is None
                    else np.ascontiguousarray([1 if v else 0 for v in has_focus], dtype=np.uint8))
            if a_hf.shape != (nq,):
                raise ValueError("has_focus: one flag per query")
    prm = KhopParams(float(dense_weight), float(bm25_weight), float(focused_weight_hop2), float(cov_weight),
                     float(cons_weight), float(rrf_lambda), float(rrf_k))
    o_dense = np.zeros(max(total, 1), dtype=np.float64)
    o_foc = np.zeros(max(total, 1), dtype=np.float64)
    o_fin = np.zeros(max(total, 1), dtype=np.float64)
    o_ord = np.zeros(max(total, 1), dtype=np.int32)
    handle = index._h if (index is not None and a_dense is None) else None
    dev = index.device if index is not None else int(device)
    rc = lib.anr_index_khop_rerank(handle, dev, nq, _ptr(offs), _ptr(a_rows), _ptr(a_q), _ptr(a_f), _ptr(a_hf), _ptr(a_dense),
                                   _ptr(a_foc), _ptr(a_bm25), _ptr(a_prf), _ptr(a_psim), _ptr(a_cov), _ptr(a_cons),
                                   _ptr(a_hop), _ptr(a_decay), C.byref(prm), _ptr(o_dense), _ptr(o_foc), _ptr(o_fin),
                                   _ptr(o_ord))
    if rc == EINVAL:
        raise KhopShapeError(f"anr_index_khop_rerank refused the call (code {rc}): {_lib.last_error()}")
    _lib.check(rc, "anr_index_khop_rerank")
    return [(o_dense[offs[q]:offs[q + 1]], o_foc[offs[q]:offs[q + 1]], o_fin[offs[q]:offs[q + 1]],
             o_ord[offs[q]:offs[q + 1]].astype(np.int64)) for q in range(nq)]


def cluster_suppression(index, rows, scores, *, cos_threshold=0.90, keep_per_cluster=2, sim=None,
                        device=0) -> List[np.ndarray]:
    """Suppress near-duplicates, per query: ``rows`` (index row ids; ignored when ``sim`` is given) and ``scores`` (the
    candidates' final_score) are ragged, ``sim`` one [C, C] float64 cosine matrix per query (``index`` may then be
    ``None``).  The input need not be sorted.  Returns, per query, the kept positions in final order."""
    lib = _lib.load()
    offs = _offsets(scores)
    nq, total = len(offs) - 1, int(offs[-1])
    a_score = _ragged(scores, np.float64, offs, "scores")
    a_rows = a_sim = None
    if sim is not None:
        mats = [np.ascontiguousarray(m, dtype=np.float64) for m in sim]
        if len(mats) != nq or any(m.shape != (c, c) for m, c in zip(mats, np.diff(offs))):
            raise ValueError("sim: one [C, C] matrix per query, C the length of that query's scores")
        a_sim = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in mats]) if mats else np.zeros(0), dtype=np.float64)
    else:
        if index is None:
            raise ValueError("cluster_suppression needs an index or sim=")
        a_rows = _ragged(rows, np.int64, offs, "rows")
    kept = np.zeros(max(total, 1), dtype=np.int32)
    n_kept = np.zeros(max(nq, 1), dtype=np.int32)
    handle = index._h if (index is not None and a_sim is None) else None
    dev = index.device if index is not None else int(device)
    rc = lib.anr_index_cluster_suppress(handle, dev, nq, _ptr(offs), _ptr(a_rows), _ptr(a_sim), _ptr(a_score),
                                        float(cos_threshold), int(keep_per_cluster), _ptr(kept), _ptr(n_kept))
    if rc == EINVAL:
        raise KhopShapeError(f"anr_index_cluster_suppress refused the call (code {rc}): {_lib.last_error()}")
    _lib.check(rc, "anr_index_cluster_suppress")
    return [kept[offs[q]:offs[q] + n_kept[q]].astype(np.int64) for q in range(nq)]


__all__ = ["rerank_khop", "cluster_suppression", "decay_factors", "check_unique_note_ids", "KhopShapeError",
           "MAX_CANDIDATES_PER_QUERY"]
