"""DBSCAN topic clustering on the device: the ``dbscan`` branch of the reference's ``TopicClustering._cpu_clustering``
(doc/clustering.py:88-99) and its eps selection ``_find_optimal_eps`` (:149-169).

The reference sends clustering to cuML (utils/gpu_utils.py:123-152), which does not exist on ROCm, and so ends on sklearn
on the host: O(N^2 d) for the k-distance curve and again for DBSCAN.  Here both run on the index's stored rows:

* ``find_optimal_eps`` is one exact k-nearest search of every row on an L2 index;
* ``dbscan_labels`` is ``anr_index_dbscan``: the MFMA self join's tile walk with the eps pairs consumed where they are
  produced (degree, union and border pass).  The labels are sklearn's, label for label.

``hdbscan`` (the reference's default, :73-79) has names of its own: ``hdbscan_mst`` is ``anr_index_hdbscan_mst``, the two
O(N^2 d) passes on the stored rows (core distances, then Prim's spanning tree of the mutual-reachability distance, both
sklearn's float64 bit for bit), ``hdbscan_labels`` adds the tree stage on the host (``anr_hdbscan_labels``)
and ``hdbscan_topic_labels`` is what the reference's branch returns.  One step of sklearn's is not a function of the data:
it orders the tree's edges with an unstable ``np.argsort``, so edges of equal weight come in an order that neither the data
nor the code defines.  Here the order is defined: a stable sort, equal weights keep Prim's order.  Where the reference's
labels hang on that order, ours are the stable-order ones (behavioural differences).  ``cluster_labels``
keeps refusing ``hdbscan`` and ``kmeans``: it is the ``dbscan`` branch.

K-means has names of its own.  The reference fixes ``random_state=42`` and every draw sklearn makes is independent of the
data, so the host draws them all up front (``kmeans_draws``) and ``anr_index_kmeans`` runs the rest on the stored rows
(DESIGN.md §5j): ``kmeans_fit`` is ``KMeans(n_clusters, n_init, random_state).fit``, ``find_optimal_k`` the reference's
``_find_optimal_k`` (:110-147), ``kmeans_topic_labels`` what the ``kmeans`` branch (:80-87) returns and ``fallback_labels``
what ``_fallback_clustering`` (:101-108) returns.  An input on which a cluster loses all its rows raises
``EmptyClusterError``: sklearn relocates such a centre in an order that is not defined, so that input stays on sklearn.

What the reference does with the labels of ANY of the three algorithms, ``_analyze_clusters`` (:171-215), is a function of
(rows, labels) alone and is provided: ``analyze_clusters`` returns its ``cluster_info`` dict, ``silhouette_samples`` /
``silhouette_score`` sklearn's Euclidean silhouette and ``cluster_cohesion`` scipy's cosine ``pdist`` mean and standard
deviation per cluster — ``anr_index_cluster_quality``: one float64 MFMA Gram of the stored float32 rows walked in label
order.  The cluster centres are the reference's own host expression.  Not provided: ``_create_topic_pools``
and the rest of ``cluster_notes`` (string counting), a drop-in ``TopicClustering`` class, other metrics.

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
KMEANS_STATS_NAMES = ("lloyd_iterations", "assignment_passes", "seeding_steps", "scratch_bytes", "mfma_steps_per_tile",
                      "emptied_init", "strict_inits", "tol")
KMEANS_MAX_CLUSTERS = 64
HDBSCAN_MAX_MIN_SAMPLES = 16
HDBSCAN_STATS_NAMES = ("prim_steps", "core_tiles", "scratch_bytes", "partials_per_step", "core_us", "prim_us",
                       "reserved6", "reserved7")
HDBSCAN_TREE_STATS_NAMES = ("n_clusters", "n_noise", "condensed_clusters", "tied_edges", "true_splits", "rows_through_eps",
                            "reserved6", "reserved7")
QUALITY_STATS_NAMES = ("n_labels", "n_noise", "silhouette_tiles", "cohesion_tiles", "n_cohesion_clusters",
                       "scratch_bytes", "mfma_steps_per_tile", "reserved")


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


class EmptyClusterError(_lib.AnoragError):
    """A k-means cluster lost all its rows.  sklearn relocates such a centre through an ``argpartition`` whose order is
    not defined, so the device does not follow it: keep sklearn for this input."""


def kmeans_draws(n_samples: int, n_clusters: int, n_init: int, random_state=42):
    """Every random draw of sklearn's ``KMeans(n_clusters, n_init=n_init, random_state=random_state).fit`` on
    ``n_samples`` float32 rows, in sklearn's order from one ``np.random.RandomState``: per init the first centre,
    ``choice(n, p=w / w.sum())`` with ``w`` the float32 unit sample weights, then per further centre one
    ``uniform(size=2 + int(log(k)))``.  Returns (first_rows int64 [n_init], uniforms float64 [n_init, k - 1, trials])."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    trials = 2 + int(np.log(n_clusters))
    w = np.ones(n_samples, dtype=np.float32)
    first = np.empty((n_init,), dtype=np.int64)
    uniforms = np.empty((n_init, n_clusters - 1, trials), dtype=np.float64)
    for i in range(n_init):
        first[i] = rs.choice(n_samples, p=w / w.sum())
        for c in range(n_clusters - 1):
            uniforms[i, c] = rs.uniform(size=trials)
    return first, uniforms


def kmeans_fit(embeddings_or_index, n_clusters: int, n_init: int, random_state=42, device: int = 0,
               return_stats: bool = False, max_iter: int = 300, tol: float = 1e-4):
    """sklearn's ``KMeans(n_clusters, n_init=n_init, random_state=random_state).fit`` of the rows (k-means++, Lloyd):
    ``(labels int64 [N], centres float64 [k, d], inertia, n_iter)``; ``return_stats=True`` adds a dict
    (``KMEANS_STATS_NAMES`` and ``best_init``).  Given an array, a temporary L2 index is built; a ``FlatIndex`` must be
    an L2 one that does not normalise its rows.  ``ValueError`` for k < 2, k > N or k > ``KMEANS_MAX_CLUSTERS``;
    ``EmptyClusterError`` when a cluster loses all its rows."""
    k, n_init = int(n_clusters), int(n_init)
    own = not isinstance(embeddings_or_index, FlatIndex)
    index = _own_index(embeddings_or_index, "euclidean", device) if own else embeddings_or_index
    try:
        if index.metric != METRIC_L2 or index.normalize:
            raise ValueError("k-means runs on the rows as given: it needs an L2 index without normalisation")
        n = index.ntotal
        if k < 2:
            raise ValueError(f"n_clusters={k}: the device k-means needs at least 2")
        if k > KMEANS_MAX_CLUSTERS:
            raise ValueError(f"n_clusters={k} is above the {KMEANS_MAX_CLUSTERS} the device k-means holds")
        if n < k:
            raise ValueError(f"n_samples={n} should be >= n_clusters={k}.")
        if n_init < 1:
            raise ValueError(f"n_init={n_init} must be at least 1")
        first, uniforms = kmeans_draws(n, k, n_init, random_state)
        uniforms = np.ascontiguousarray(uniforms)
        labels = np.empty((n,), dtype=np.int32)
        centres = np.empty((k, index.d), dtype=np.float64)
        inertia, n_iter, best = C.c_double(0.0), C.c_int32(0), C.c_int32(-1)
        stats = np.zeros((8,), dtype=np.int64)
        rc = index._lib.anr_index_kmeans(index._h, k, n_init, uniforms.shape[2], first.ctypes.data, uniforms.ctypes.data,
                                         int(max_iter), C.c_double(float(tol)), labels.ctypes.data, centres.ctypes.data,
                                         C.addressof(inertia), C.addressof(n_iter), C.addressof(best), stats.ctypes.data)
        if rc == _lib.ANR_EEMPTY:
            raise EmptyClusterError(f"anr_index_kmeans failed (code {rc}): {_lib.last_error()}")
        _lib.check(rc, "anr_index_kmeans")
    finally:
        if own:
            index.close()
    out = (labels.astype(np.int64), centres, float(inertia.value), int(n_iter.value))
    if return_stats:
        st = dict(zip(KMEANS_STATS_NAMES, (int(v) for v in stats)))
        st["tol"] = float(stats[7:8].view(np.float64)[0])
        st["best_init"] = int(best.value)
        return out + (st,)
    return out


def _find_elbow_point(k_values, inertias) -> int:
    if len(k_values) < 3:  # the reference's _find_elbow_point (:136-147), its own expression
        return k_values[0] if k_values else 2
    diffs = np.diff(inertias)
    second_diffs = np.diff(diffs)
    elbow_idx = np.argmax(second_diffs) + 1
    return k_values[elbow_idx]


def find_optimal_k(embeddings_or_index, max_k=None, device: int = 0, return_inertias: bool = False):
    """The reference's ``_find_optimal_k`` (:110-134): ``KMeans(k, random_state=42, n_init=5)`` for k = 2 .. max_k
    (default ``min(10, N // 5)``), a fresh stream per k, then the elbow of the inertias by the reference's own host
    expression; 2 when ``max_k < 2`` or fewer than two fits succeed.  The reference's ``except`` ends the loop at the
    first fit that raises, which for sklearn is k > N; the loop ends there here too.  Every other failure (a k above
    ``KMEANS_MAX_CLUSTERS``, ``EmptyClusterError``) is raised: sklearn would have gone on.
    ``return_inertias=True``: ``(k, inertias)``."""
    own = not isinstance(embeddings_or_index, FlatIndex)
    index = _own_index(embeddings_or_index, "euclidean", device) if own else embeddings_or_index
    try:
        if max_k is None:
            max_k = min(10, index.ntotal // 5)
        inertias = []
        k_range = range(2, max_k + 1)
        if max_k >= 2:
            for k in k_range:
                if k > index.ntotal:
                    break
                inertias.append(kmeans_fit(index, k, 5, 42, device)[2])
    finally:
        if own:
            index.close()
    if max_k < 2 or len(inertias) < 2:
        optimal_k = 2
    else:
        optimal_k = int(_find_elbow_point(list(k_range)[:len(inertias)], inertias))
    return (optimal_k, inertias) if return_inertias else optimal_k


def kmeans_topic_labels(embeddings, device: int = 0) -> np.ndarray:
    """What ``_cpu_clustering`` returns for ``clustering.algorithm: kmeans`` (:80-87, :99): ``find_optimal_k``, then
    ``KMeans(optimal_k, random_state=42, n_init=10).fit_predict``.  The rows go to one temporary index once for all
    fits."""
    index = _own_index(embeddings, "euclidean", device)
    try:
        return kmeans_fit(index, find_optimal_k(index, device=device), 10, 42, device)[0]
    finally:
        index.close()


def fallback_labels(embeddings, device: int = 0) -> np.ndarray:
    """What ``_fallback_clustering`` returns (:101-108): ``KMeans(min(8, max(2, N // 10)), random_state=42)`` with
    sklearn's default ``n_init='auto'``, which is 1 for k-means++ from sklearn 1.4 on (10 before)."""
    emb = np.ascontiguousarray(embeddings, dtype=np.float32)
    n_clusters = min(8, max(2, len(emb) // 10))
    return kmeans_fit(emb, n_clusters, 1, 42, device)[0]


def hdbscan_mst(embeddings_or_index, min_samples: int = 3, device: int = 0, return_stats: bool = False):
    """What sklearn's ``HDBSCAN(min_samples=min_samples, metric='euclidean')`` computes before its tree stage:
    ``(core, src, dst, w)`` — the float64 core distances [N] (the ``min_samples``-th smallest distance of a row, itself
    included) and the N - 1 edges of Prim's spanning tree of ``max(core_a, core_b, dist)`` from row 0, in the order they
    are added (int64, int64, float64), all bit-equal to sklearn's.  Given an array, a temporary L2 index is built; a
    ``FlatIndex`` must be an L2 one that does not normalise its rows; its rows stay on the device (they are checked for
    NaN and infinities there, before either pass).  ``ValueError`` before either pass for fewer than 2 rows,
    ``min_samples`` outside 1 .. min(``HDBSCAN_MAX_MIN_SAMPLES``, N), and rows that are not finite (sklearn's handling of
    infinite rows stays on sklearn).  The index is locked for the whole call.  ``return_stats=True`` adds a dict (``HDBSCAN_STATS_NAMES``)."""
    ms = int(min_samples)
    if ms < 1:
        raise ValueError(f"min_samples={ms} must be at least 1")
    if ms > HDBSCAN_MAX_MIN_SAMPLES:
        raise ValueError(f"min_samples={ms} is above the {HDBSCAN_MAX_MIN_SAMPLES} the device core distances keep")
    own = not isinstance(embeddings_or_index, FlatIndex)
    if own:
        rows = np.ascontiguousarray(embeddings_or_index, dtype=np.float32)
        if rows.ndim != 2:
            raise ValueError(f"expected an [N, d] array of embeddings, got shape {rows.shape}")
        n = rows.shape[0]
    else:
        index = embeddings_or_index
        if index.metric != METRIC_L2 or index.normalize:
            raise ValueError("hdbscan runs on the rows as given: it needs an L2 index without normalisation")
        n = index.ntotal
        rows = None
    if n < 2:
        raise ValueError(f"n_samples={n}: hdbscan needs at least 2 rows")
    if ms > n:
        raise ValueError(f"min_samples ({ms}) must be at most the number of samples in X ({n})")
    if rows is not None and not np.isfinite(rows).all():  # the rows of an index are looked at on the device
        raise ValueError("the rows hold NaN or infinite values: keep sklearn for such an input")
    if own:
        index = _own_index(rows, "euclidean", device)
    try:
        core = np.empty((n,), dtype=np.float64)
        src = np.empty((n - 1,), dtype=np.int64)
        dst = np.empty((n - 1,), dtype=np.int64)
        w = np.empty((n - 1,), dtype=np.float64)
        stats = np.zeros((8,), dtype=np.int64)
        rc = index._lib.anr_index_hdbscan_mst(index._h, ms, core.ctypes.data, src.ctypes.data, dst.ctypes.data,
                                              w.ctypes.data, stats.ctypes.data)
        if rc == -1 and "NaN or infinite" in _lib.last_error():
            raise ValueError("the rows hold NaN or infinite values: keep sklearn for such an input")
        _lib.check(rc, "anr_index_hdbscan_mst")
    finally:
        if own:
            index.close()
    if return_stats:
        return core, src, dst, w, dict(zip(HDBSCAN_STATS_NAMES, (int(v) for v in stats)))
    return core, src, dst, w


def hdbscan_tree_labels(src, dst, w, min_cluster_size: int = 5, cluster_selection_epsilon: float = 0.0,
                        return_stats: bool = False):
    """``anr_hdbscan_labels`` as it is (host only, no device needed): int64 labels [N], -1 for noise, from the N - 1 edges
    of a spanning tree — sklearn's single linkage, condensed tree, stability, excess of mass and epsilon search, with equal
    weights kept in the order given.  ``ValueError`` for what the library refuses."""
    src = np.ascontiguousarray(src, dtype=np.int64)
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    w = np.ascontiguousarray(w, dtype=np.float64)
    if not (src.ndim == dst.ndim == w.ndim == 1 and src.shape == dst.shape == w.shape):
        raise ValueError(f"expected three arrays of N - 1 edges, got shapes {src.shape}, {dst.shape}, {w.shape}")
    n = int(w.shape[0]) + 1
    labels = np.empty((n,), dtype=np.int32)
    stats = np.zeros((8,), dtype=np.int64)
    lib = _lib.load()
    rc = lib.anr_hdbscan_labels(n, src.ctypes.data, dst.ctypes.data, w.ctypes.data, int(min_cluster_size),
                                C.c_double(float(cluster_selection_epsilon)), labels.ctypes.data, stats.ctypes.data)
    if rc == -1:
        raise ValueError(_lib.last_error())
    _lib.check(rc, "anr_hdbscan_labels")
    out = labels.astype(np.int64)
    if return_stats:
        return out, dict(zip(HDBSCAN_TREE_STATS_NAMES, (int(v) for v in stats)))
    return out


def hdbscan_labels(embeddings_or_index, min_cluster_size: int = 5, min_samples=None, cluster_selection_epsilon: float = 0.0,
                   device: int = 0, return_stats: bool = False):
    """sklearn's ``HDBSCAN(min_cluster_size, min_samples, metric='euclidean', cluster_selection_epsilon).fit_predict`` of
    the rows with the stable tie order: int64 labels, -1 for noise.  ``min_samples=None`` means ``min_cluster_size``, as in
    sklearn.  ``hdbscan_mst`` on the device, then ``hdbscan_tree_labels`` on the host.  Only ``eom`` selection without
    ``allow_single_cluster`` and ``max_cluster_size``; no ``probabilities_``, no medoids."""
    mcs = int(min_cluster_size)
    if mcs < 2:
        raise ValueError(f"min_cluster_size={mcs} must be at least 2")
    ms = mcs if min_samples is None else int(min_samples)
    got = hdbscan_mst(embeddings_or_index, ms, device, return_stats)
    labels = hdbscan_tree_labels(got[1], got[2], got[3], mcs, cluster_selection_epsilon, return_stats)
    if return_stats:
        return labels[0], {**got[4], **labels[1]}
    return labels


def hdbscan_topic_labels(embeddings, min_cluster_size: int = 5, min_samples: int = 3, device: int = 0) -> np.ndarray:
    """What ``_cpu_clustering`` returns for ``clustering.algorithm: hdbscan``, the reference's default (:73-79, :99):
    ``HDBSCAN(min_cluster_size, min_samples, metric='euclidean', cluster_selection_epsilon=0.1).fit_predict``."""
    return hdbscan_labels(embeddings, min_cluster_size, min_samples, 0.1, device)


def _int32_labels(labels, n: int) -> np.ndarray:
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.shape[0] != n:
        raise ValueError(f"expected one label per row: {n} rows, labels of shape {lab.shape}")
    if lab.dtype.kind not in "iu":
        raise ValueError(f"labels must be integers, got {lab.dtype}")
    if lab.size and (int(lab.min()) < -2 ** 31 or int(lab.max()) >= 2 ** 31):
        raise ValueError("labels must fit a 32-bit integer")
    return np.ascontiguousarray(lab, dtype=np.int32)


def cluster_quality(embeddings_or_index, labels, device: int = 0, silhouette: bool = True, cohesion: bool = True,
                    return_stats: bool = False):
    """``anr_index_cluster_quality`` as it is: a dict with ``labels`` (the distinct labels, ascending, int64), ``sizes``,
    and, as asked for, ``samples`` (float64 silhouette of every row) and ``mean``, ``cohesion`` and ``std`` (per distinct
    label, NaN where not defined).  Given an array, a temporary L2 index is built; a ``FlatIndex`` must be an L2 one that
    does not normalise its rows."""
    own = not isinstance(embeddings_or_index, FlatIndex)
    index = _own_index(embeddings_or_index, "euclidean", device) if own else embeddings_or_index
    try:
        if index.metric != METRIC_L2 or index.normalize:
            raise ValueError("cluster quality is measured on the rows as given: it needs an L2 index without normalisation")
        n = index.ntotal
        lab = _int32_labels(labels, n)
        cap = max(1, int(np.unique(lab).size))
        out_labels = np.empty((cap,), dtype=np.int32)
        sizes = np.zeros((cap,), dtype=np.int64)
        samples = np.zeros((n,), dtype=np.float64) if silhouette else None
        mean = C.c_double(0.0)
        coh = np.full((cap,), np.nan) if cohesion else None
        std = np.full((cap,), np.nan) if cohesion else None
        n_labels = C.c_int64(0)
        stats = np.zeros((8,), dtype=np.int64)
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        _lib.check(index._lib.anr_index_cluster_quality(
            index._h, lab.ctypes.data, ptr(samples), C.addressof(mean) if silhouette else None, cap, out_labels.ctypes.data,
            sizes.ctypes.data, ptr(coh), ptr(std), C.addressof(n_labels), stats.ctypes.data), "anr_index_cluster_quality")
    finally:
        if own:
            index.close()
    k = int(n_labels.value)
    out = {"labels": out_labels[:k].astype(np.int64), "sizes": sizes[:k]}
    if silhouette:
        out["samples"], out["mean"] = samples, float(mean.value)
    if cohesion:
        out["cohesion"], out["std"] = coh[:k], std[:k]
    if return_stats:
        out["stats"] = dict(zip(QUALITY_STATS_NAMES, (int(v) for v in stats)))
    return out


def _check_number_of_labels(n_labels: int, n_samples: int) -> None:
    if not 1 < n_labels < n_samples:  # sklearn.metrics.cluster._unsupervised.check_number_of_labels
        raise ValueError(f"Number of labels is {n_labels}. Valid values are 2 to n_samples - 1 (inclusive)")


def silhouette_samples(embeddings_or_index, labels, device: int = 0) -> np.ndarray:
    """sklearn's ``silhouette_samples(X, labels, metric='euclidean')``: float64 [N]; every distinct label value is a
    cluster (-1 too, as in the reference's call).  Raises ``ValueError`` where sklearn does: a number of distinct labels
    outside 2 .. N - 1."""
    q = cluster_quality(embeddings_or_index, labels, device, cohesion=False)
    _check_number_of_labels(int(q["labels"].size), int(q["samples"].size))
    return q["samples"]


def silhouette_score(embeddings_or_index, labels, device: int = 0) -> float:
    """sklearn's ``silhouette_score(X, labels)`` (Euclidean): the mean of ``silhouette_samples``, summed on the device in
    one fixed order."""
    q = cluster_quality(embeddings_or_index, labels, device, cohesion=False)
    _check_number_of_labels(int(q["labels"].size), int(q["samples"].size))
    return q["mean"]


def cluster_cohesion(embeddings_or_index, labels, device: int = 0) -> dict:
    """``{label: {'cohesion', 'std'}}`` for every label >= 0 with at least two rows: ``np.mean`` and ``np.std`` of scipy's
    ``pdist(rows_of_the_label, metric='cosine')`` (:197-203).  A zero row makes both values of its cluster NaN, as scipy's
    do."""
    q = cluster_quality(embeddings_or_index, labels, device, silhouette=False)
    return {int(lab): {"cohesion": float(c), "std": float(s)}
            for lab, m, c, s in zip(q["labels"], q["sizes"], q["cohesion"], q["std"]) if lab >= 0 and m > 1}


def analyze_clusters(embeddings, labels, device: int = 0) -> dict:
    """The reference's ``TopicClustering._analyze_clusters(cluster_labels, embeddings)`` (:171-215): its ``cluster_info``
    dict, same keys, nesting and value types — ``n_clusters``, ``n_noise``, ``cluster_sizes``, ``cluster_centers``,
    ``cluster_quality`` (clusters of two rows or more) and ``silhouette_score``; noise (-1) has no size, centre or quality.
    The two O(N^2 d) measures are one ``anr_index_cluster_quality`` call on a temporary L2 index of the float32 rows.
    ``cluster_centers`` stay on the host: the reference's own expression ``np.mean(embeddings[mask], axis=0).tolist()`` on
    the float32 rows, O(N d) and bit-identical by construction.  ``silhouette_score`` is 0.0 where the reference's is:
    unless ``n_clusters > 1 and N > n_clusters``, and where sklearn raises (distinct labels, noise included, outside
    2 .. N - 1), which the reference's ``except`` turns into 0.0."""
    emb = np.ascontiguousarray(embeddings, dtype=np.float32)
    if emb.ndim != 2:
        raise ValueError(f"expected an [N, d] array of embeddings, got shape {emb.shape}")
    cluster_labels = np.asarray(labels)
    _int32_labels(cluster_labels, emb.shape[0])
    unique_labels = np.unique(cluster_labels)
    n_clusters = len(unique_labels[unique_labels >= 0])
    info = {"n_clusters": n_clusters, "n_noise": np.sum(cluster_labels == -1), "cluster_sizes": {}, "cluster_centers": {},
            "cluster_quality": {}}
    q = cluster_quality(emb, cluster_labels, device) if emb.shape[0] else None
    for label in unique_labels:
        if label == -1:
            continue
        mask = cluster_labels == label
        info["cluster_sizes"][label] = int(np.sum(mask))
        info["cluster_centers"][label] = np.mean(emb[mask], axis=0).tolist()
        if info["cluster_sizes"][label] > 1:
            at = int(np.searchsorted(q["labels"], int(label)))
            info["cluster_quality"][label] = {"cohesion": float(q["cohesion"][at]), "std": float(q["std"][at])}
    info["silhouette_score"] = 0.0
    if n_clusters > 1 and len(emb) > n_clusters and 1 < len(unique_labels) < len(emb):
        info["silhouette_score"] = float(q["mean"])
    return info


__all__ = ["dbscan_labels", "find_optimal_eps", "cluster_labels", "EPS_INFLATION", "STATS_NAMES", "analyze_clusters",
           "silhouette_samples", "silhouette_score", "cluster_cohesion", "cluster_quality", "QUALITY_STATS_NAMES", "kmeans_fit",
           "kmeans_draws", "find_optimal_k", "kmeans_topic_labels", "fallback_labels", "EmptyClusterError",
           "KMEANS_STATS_NAMES", "KMEANS_MAX_CLUSTERS", "hdbscan_mst", "hdbscan_tree_labels", "hdbscan_labels",
           "hdbscan_topic_labels", "HDBSCAN_MAX_MIN_SAMPLES", "HDBSCAN_STATS_NAMES", "HDBSCAN_TREE_STATS_NAMES"]
