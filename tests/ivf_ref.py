"""Test helper: the IVF-Flat index (anr_ivf_*, csrc/ivf.hip) restated in numpy with float64 scoring — assignment,
Lloyd's iterations from given centroids (with the empty-list split rule), the probed-list set and the exact top-k over
the probed rows.  Keys: IP x.c; L2 -|x - c|^2 (larger is better in both); ties go to the lower list id / row id."""
from __future__ import annotations

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def keys(a: np.ndarray, b: np.ndarray, metric: str) -> np.ndarray:
    """float64 keys [len(a), len(b)] of float32 rows"""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    if metric == "ip":
        return a64 @ b64.T
    d2 = (a64 * a64).sum(1)[:, None] - 2.0 * (a64 @ b64.T) + (b64 * b64).sum(1)[None, :]
    return -np.maximum(d2, 0.0)


def assign(x: np.ndarray, cent: np.ndarray, metric: str) -> np.ndarray:
    """list of each row: the best key, the lowest list id among equal keys (argmax returns the first)"""
    return np.argmax(keys(x, cent, metric), axis=1).astype(np.int64)


def means(x: np.ndarray, a: np.ndarray, cent: np.ndarray) -> np.ndarray:
    """Lloyd's update with the split rule of csrc/ivf.hip: an empty list j (ascending) takes the second half (ascending
    row order) of the currently largest list (lowest id among equals; only if it holds >= 2 rows)"""
    nlist = cent.shape[0]
    members = [list(np.flatnonzero(a == l)) for l in range(nlist)]
    for j in range(nlist):
        if members[j]:
            continue
        sizes = [len(m) for m in members]
        b = int(np.argmax(sizes))
        if sizes[b] < 2:
            break
        keep = sizes[b] - sizes[b] // 2
        members[j] = members[b][keep:]
        members[b] = members[b][:keep]
    out = cent.copy()
    for l, m in enumerate(members):
        if m:
            out[l] = x[m].astype(np.float64).mean(axis=0).astype(np.float32)
    return out


def normalize_rows(c: np.ndarray) -> np.ndarray:
    """every row divided by the float32 of its float64 norm (zero rows stay zero), as the device does"""
    s = np.sqrt((c.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    return np.where(s[:, None] != 0, c / np.where(s == 0, 1, s)[:, None], c).astype(np.float32)


def lloyd(x: np.ndarray, init: np.ndarray, niter: int, metric: str, spherical: bool = False) -> np.ndarray:
    """niter iterations; spherical: every centroid normalised after each update"""
    c = init.astype(np.float32).copy()
    for _ in range(niter):
        c = means(x, assign(x, c, metric), c)
        if spherical:
            c = normalize_rows(c)
    return c


def inertia(x: np.ndarray, cent: np.ndarray, metric: str) -> float:
    """sum over rows of the best key's distance form: L2 sum of squared distances; IP minus the sum of best products"""
    return float(-keys(x, cent, metric).max(axis=1).sum())


def probed(q: np.ndarray, cent: np.ndarray, nprobe: int, metric: str) -> np.ndarray:
    """[nq, nprobe] list ids, best first (ties to the lower id)"""
    k = keys(q, cent, metric)
    order = np.lexsort((np.broadcast_to(np.arange(cent.shape[0]), k.shape), -k), axis=1)
    return order[:, :nprobe]


def probe_margin(q: np.ndarray, cent: np.ndarray, nprobe: int, metric: str) -> np.ndarray:
    """gap between the nprobe-th and (nprobe+1)-th best centroid keys (inf when nprobe >= nlist)"""
    k = -np.sort(-keys(q, cent, metric), axis=1)
    if nprobe >= cent.shape[0]:
        return np.full(q.shape[0], np.inf)
    return k[:, nprobe - 1] - k[:, nprobe]


def search(q: np.ndarray, x: np.ndarray, ids: np.ndarray, lists: np.ndarray, cent: np.ndarray, k: int, nprobe: int,
           metric: str):
    """exact top-k over the rows (ids, list of each row) of the probed lists: D float32 (IP score / squared L2), I int64
    with -1 / -FLT_MAX (IP) / +FLT_MAX (L2) padding"""
    nq = q.shape[0]
    D = np.full((nq, k), -FLT_MAX if metric == "ip" else FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    P = probed(q, cent, nprobe, metric)
    for i in range(nq):
        sel = np.flatnonzero(np.isin(lists, P[i]))
        if len(sel) == 0:
            continue
        s = keys(q[i:i + 1], x[sel], metric)[0]
        order = np.lexsort((ids[sel], -s))[:k]
        D[i, :len(order)] = (s[order] if metric == "ip" else -s[order]).astype(np.float32)
        I[i, :len(order)] = ids[sel][order]
    return D, I
