"""Diversity scheduling on the device: semantic dedup and greedy diverse selection of fused candidates, the arithmetic of
the reference's ``DiversityScheduler.schedule_candidates`` (retrieval/diversity_scheduler.py:523).

``diversify`` is ``anr_index_diversify``: for a batch of queries with ragged candidate lists it builds one C x C float64
cosine matrix per query from the index's stored rows (f64 MFMA) and runs the decision procedure on it,
one workgroup per query.  With ``sim=`` the matrices are the caller's and no index is needed.

Everything here fails loudly when the HIP library is missing; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DiversityParams

MAX_CANDIDATES_PER_QUERY = 1024
EINVAL = -1


class DiversityShapeError(_lib.AnoragError):
    """The call was refused as ANR_EINVAL (a list longer than 1024 candidates, a row id outside the index, ...)."""


def _ragged(lists, dtype, what):
    arrs = [np.ascontiguousarray(a, dtype=dtype).reshape(-1) for a in lists]
    offs = np.zeros(len(arrs) + 1, dtype=np.int64)
    if arrs:
        offs[1:] = np.cumsum([a.size for a in arrs])
    flat = np.concatenate(arrs) if arrs else np.zeros(0, dtype=dtype)
    return offs, np.ascontiguousarray(flat, dtype=dtype)


def diversify(index, rows, scores, type_masks=None, *, max_candidates, similarity_threshold, dedup=True, quota=False,
              quotas=None, balance_factor=0.8, sim=None, device=0):
    """Dedup and select, per query.

    ``rows``: one sequence of index row ids per query (ignored, and may be ``None``, when ``sim`` is given);
    ``scores``: one float sequence per query; ``type_masks``: one uint32 sequence per query (bit t = evidence type t) or
    ``None``; ``quotas``: up to 32 ints, the quota of type t; ``sim``: one [C, C] float64 matrix per query, used instead
    of the cosine of the stored rows (``index`` may then be ``None``; the call runs on ``device``).

    Returns, per query, ``(kept, selected, selected_sim)``: the positions (within the query's list) that survive the
    dedup, in kept order; the positions selected, in selection order; the [K, K] float64 similarities of the selected."""
    lib = _lib.load()
    score_offs, score_flat = _ragged(scores, np.float64, "scores")
    nq = len(score_offs) - 1
    offs = score_offs
    sizes = np.diff(offs)
    rows_flat = None
    sim_flat = None
    if sim is not None:
        mats = [np.ascontiguousarray(m, dtype=np.float64) for m in sim]
        if len(mats) != nq or any(m.shape != (c, c) for m, c in zip(mats, sizes)):
            raise ValueError("sim: one [C, C] matrix per query, C the length of that query's scores")
        sim_flat = np.concatenate([m.reshape(-1) for m in mats]) if mats else np.zeros(0)
        sim_flat = np.ascontiguousarray(sim_flat, dtype=np.float64)
    else:
        if index is None:
            raise ValueError("diversify needs an index or sim=")
        row_offs, rows_flat = _ragged(rows, np.int64, "rows")
        if not np.array_equal(row_offs, offs):
            raise ValueError("rows and scores must have the same lengths per query")
    types_flat = None
    if type_masks is not None:
        t_offs, types_flat = _ragged(type_masks, np.uint32, "type_masks")
        if not np.array_equal(t_offs, offs):
            raise ValueError("type_masks and scores must have the same lengths per query")
    prm = DiversityParams()
    prm.max_candidates = int(max_candidates)
    prm.dedup = 1 if dedup else 0
    prm.quota = 1 if quota else 0
    prm.similarity_threshold = float(similarity_threshold)
    prm.balance_factor = float(balance_factor)
    q = list(quotas) if quotas is not None else []
    if len(q) > 32:
        raise ValueError("at most 32 evidence types")
    for t, v in enumerate(q):
        prm.quotas[t] = int(v)
    total = int(offs[-1])
    kcap = np.minimum(sizes, max(int(max_candidates), 0))
    koff = np.zeros(nq + 1, dtype=np.int64)
    koff[1:] = np.cumsum(kcap * kcap)
    kept = np.zeros(max(total, 1), dtype=np.int32)
    sel = np.zeros(max(total, 1), dtype=np.int32)
    n_kept = np.zeros(max(nq, 1), dtype=np.int32)
    n_sel = np.zeros(max(nq, 1), dtype=np.int32)
    sel_sim = np.zeros(max(int(koff[-1]), 1), dtype=np.float64)
    handle = index._h if (index is not None and sim_flat is None) else None
    dev = index.device if index is not None else int(device)
    rc = lib.anr_index_diversify(handle, dev, nq, offs.ctypes.data,
                                 rows_flat.ctypes.data if rows_flat is not None else None,
                                 sim_flat.ctypes.data if sim_flat is not None else None,
                                 score_flat.ctypes.data, types_flat.ctypes.data if types_flat is not None else None,
                                 C.byref(prm), kept.ctypes.data, n_kept.ctypes.data, sel.ctypes.data, n_sel.ctypes.data,
                                 sel_sim.ctypes.data)
    if rc == EINVAL:
        raise DiversityShapeError(f"anr_index_diversify refused the call (code {rc}): {_lib.last_error()}")
    _lib.check(rc, "anr_index_diversify")
    out = []
    for i in range(nq):
        o, nk, ns = int(offs[i]), int(n_kept[i]), int(n_sel[i])
        ks = sel_sim[koff[i]:koff[i] + ns * ns].reshape(ns, ns).copy()
        out.append((kept[o:o + nk].astype(np.int64), sel[o:o + ns].astype(np.int64), ks))
    return out


__all__ = ["diversify", "DiversityShapeError", "MAX_CANDIDATES_PER_QUERY"]
