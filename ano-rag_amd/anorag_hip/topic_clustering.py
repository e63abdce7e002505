"""DBSCAN topic clustering on the device: the ``dbscan`` branch of the reference's ``TopicClustering._cpu_clustering``
(doc/clustering.py:88-99) and its eps selection ``_find_optimal_eps`` (:149-169).

The reference sends clustering to cuML (utils/gpu_utils.py:123-152), which does not exist on ROCm, and so ends on sklearn
on the host: O(N^2 d) for the k-distance curve and again for DBSCAN.  Here both run on the index's stored rows:

* ``find_optimal_eps`` is one exact k-nearest search of every row on an L2 index;
* ``dbscan_labels`` is ``anr_index_dbscan``: the MFMA self join's tile walk with the eps pairs consumed where they are
  produced (degree, union and border pass).  The labels are sklearn's, label for label.

``hdbscan`` (the reference's default) and ``kmeans`` are not provided: their results are not functions of the data alone
(tie order in the spanning tree, sklearn's RNG stream); they stay on sklearn.

Everything here fails loudly when the HIP library is missing; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .flat_index import METRIC_IP, METRIC_L2, FlatIndex

# find_optimal_eps multiplies an unclipped eps by this: the reference's eps is the distance of an actual pair, and whether
# sklearn then counts that pair inside its own neighbourhood hangs on the rounding of sqrt(x)^2 against x.  Inflated,
# the defining pair is always inside and the labels are a function of the data (behavioural differences).
EPS_INFLATION = 1.0 + 2.0 ** -20

STATS_NAMES = ("n_clusters", "n_core", "n_noise", "n_rescored", "tile_walks", "jump_rounds", "list_regrown",
               "n_rescored_in")


def _own_index(embeddings, metric: str, device: int) -> FlatIndex:
    emb = np.ascontiguousarray(embeddings, dtype=np.float32)
    if emb.ndim != 2:
        raise ValueError(f"expected an [N, d] array of embeddings, got shape {emb.shape}")
    if metric == "euclidean":
        index = FlatIndex(emb.shape[1], METRIC_L2, normalize=False, device=device)
    else:
        index = FlatIndex(emb.shape[1], METRIC_IP, normalize=True, device=device)
    try:
        if emb.shape[0]:
            index.add(emb)
    except Exception:
        index.close()
        raise
    return index


def _check_metric(metric: str) -> None:
    if metric not in ("euclidean", "cosine"):
        raise ValueError(f"unsupported metric {metric!r}: dbscan_labels knows 'euclidean' and 'cosine'")


def dbscan_labels(embeddings_or_index, eps: float, min_samples: int = 3, metric: str = "euclidean", device: int = 0,
                  return_stats: bool = False):
    """sklearn's ``DBSCAN(eps, min_samples, metric).fit_predict`` of the rows: int64 labels, -1 for noise.  Given an
    array, a temporary index is built (L2, or inner product with normalisation for ``"cosine"``); a ``FlatIndex`` of
    the matching kind is used as it is.  ``return_stats=True`` adds the call's counters (``STATS_NAMES``)."""
    _check_metric(metric)
    own = not isinstance(embeddings_or_index, FlatIndex)
    if own:
        index = _own_index(embeddings_or_index, metric, device)
    else:
        index = embeddings_or_index
        want = (METRIC_L2, False) if metric == "euclidean" else (METRIC_IP, True)
        if (index.metric, index.normalize) != want:
            raise ValueError(f"metric {metric!r} needs " + ("an L2 index" if metric == "euclidean" else
                                                            "an inner-product index that normalises its rows"))
    try:
        labels = np.empty((index.ntotal,), dtype=np.int32)
        stats = np.zeros((8,), dtype=np.int64)
        _lib.check(index._lib.anr_index_dbscan(index._h, C.c_double(float(eps)), int(min_samples), labels.ctypes.data,
                                               stats.ctypes.data), "anr_index_dbscan")
    finally:
        if own:
            index.close()
    out = labels.astype(np.int64)
    if return_stats:
        return out, dict(zip(STATS_NAMES, (int(v) for v in stats)))
    return out


def find_optimal_eps(embeddings_or_index, min_samples: int = 3, device: int = 0) -> float:
    """The reference's ``_find_optimal_eps``: the Euclidean distance from every row to its ``min_samples``-th nearest
    stored row (itself included), sorted; the value where the curve makes its largest step up; clipped to [0.1, 2.0].
    Always Euclidean, whatever metric the clustering uses (the reference's ``NearestNeighbors`` is built with its
    default metric), so an index passed in must be an L2 one.  An unclipped result is multiplied by ``EPS_INFLATION``."""
    k = int(min_samples)
    own = not isinstance(embeddings_or_index, FlatIndex)
    index = _own_index(embeddings_or_index, "euclidean", device) if own else embeddings_or_index
    try:
        if index.metric != METRIC_L2:
            raise ValueError("find_optimal_eps measures Euclidean distances: it needs an L2 index")
        n = index.ntotal
        if k < 1 or k > n:
            raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {n}")
        if n < 2:
            raise ValueError("the k-distance curve of a single row has no step")
        kth = np.empty((n,), dtype=np.float64)
        step = 1 << 16
        for i in range(0, n, step):
            m = min(step, n - i)
            D, _ = index.search(index.reconstruct_n(i, m), k)
            kth[i:i + m] = np.sqrt(np.maximum(D[:, k - 1].astype(np.float64), 0.0))
    finally:
        if own:
            index.close()
    kth.sort()
    eps = float(kth[int(np.argmax(np.diff(kth)))])
    if eps < 0.1:
        return 0.1
    if eps > 2.0:
        return 2.0
    return min(2.0, eps * EPS_INFLATION)


def cluster_labels(embeddings, algorithm: str = "dbscan", min_samples: int = 3, metric: str = "euclidean",
                   device: int = 0) -> np.ndarray:
    """What ``_cpu_clustering`` returns for ``clustering.algorithm: dbscan``: ``find_optimal_eps`` then
    ``dbscan_labels``.  The other algorithms are not provided; the caller keeps the reference's sklearn path."""
    algo = str(algorithm).lower()
    if algo in ("hdbscan", "kmeans"):
        raise NotImplementedError(f"{algo} is not provided on the device: keep the reference's sklearn path "
                                  "(TopicClustering._cpu_clustering) for it")
    if algo != "dbscan":
        raise ValueError(f"Unsupported clustering algorithm: {algorithm}")
    _check_metric(metric)
    emb = np.ascontiguousarray(embeddings, dtype=np.float32)
    l2 = _own_index(emb, "euclidean", device)
    try:
        eps = find_optimal_eps(l2, min_samples, device)
        if metric == "euclidean":
            return dbscan_labels(l2, eps, min_samples, "euclidean", device)
    finally:
        l2.close()
    return dbscan_labels(emb, eps, min_samples, "cosine", device)


__all__ = ["dbscan_labels", "find_optimal_eps", "cluster_labels", "EPS_INFLATION", "STATS_NAMES"]
