"""GPU tests of anr_index_dbscan and anorag_hip.topic_clustering: device labels against the float64 restatement
(tests/cluster_ref.py) and, on the golden cases, against sklearn's and the reference's recorded output.  Equality
throughout: the decision D <= eps is the float64 one on both sides, and every eps is chosen away from any pair."""
import ctypes as C

import numpy as np
import pytest

import cluster_ref as cr
from test_cluster_cpu import CASES, IDS

pytestmark = pytest.mark.gpu


def _index(x, metric):
    from anorag_hip import METRIC_IP, METRIC_L2, FlatIndex
    x = np.ascontiguousarray(x, dtype=np.float32)
    idx = FlatIndex(x.shape[1], METRIC_L2 if metric == "euclidean" else METRIC_IP, normalize=metric == "cosine")
    idx.add(x)
    return idx


def device_and_rows(x, eps, ms, metric):
    """device labels, the call's counters, and the rows as the index stores them (what the restatement is given)"""
    from anorag_hip.topic_clustering import dbscan_labels
    idx = _index(x, metric)
    try:
        labels, stats = dbscan_labels(idx, eps, ms, metric, return_stats=True)
        rows = idx.reconstruct_n(0, idx.ntotal)
    finally:
        idx.close()
    return labels, stats, rows


def eps_between_pairs(D, q):
    """an eps at quantile q of the pair distances, half way between two neighbouring values: no pair sits on it"""
    d = np.unique(D[np.triu_indices(len(D), 1)])
    if d.size < 2:
        return float(d[0]) * 1.5 if d.size else 1.0
    i = min(int(q * d.size), d.size - 2)
    return float(0.5 * (d[i] + d[i + 1]))


def blobs(n, d, seed):
    rng = np.random.default_rng(seed)
    c = max(1, min(5, n // 50))
    centres = rng.standard_normal((c, d))
    x = centres[rng.integers(0, c, n)] + rng.standard_normal((n, d)) * 0.2
    stray = rng.random(n) < 0.05
    x[stray] += rng.standard_normal((int(stray.sum()), d)) * 0.6
    return x.astype(np.float32)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_golden_labels(c):
    from anorag_hip.topic_clustering import EPS_INFLATION
    eps = c["eps"] * EPS_INFLATION if c["auto"] and 0.1 < c["eps"] < 2.0 else c["eps"]
    labels, stats, rows = device_and_rows(c["x"], eps, c["ms"], c["metric"])
    assert np.array_equal(labels, c["labels"])                                  # sklearn / the reference
    assert np.array_equal(labels, cr.dbscan_ref(rows, eps, c["ms"], c["metric"]))  # the restatement, on the stored rows
    assert stats["n_clusters"] == c["labels"].max() + 1 and stats["n_noise"] == int((c["labels"] < 0).sum())
    assert stats["tile_walks"] == 3


@pytest.mark.parametrize("c", [c for c in CASES if c["auto"]], ids=[i for i, c in zip(IDS, CASES) if c["auto"]])
def test_golden_auto_eps_and_cluster_labels(c):
    from anorag_hip.topic_clustering import cluster_labels, find_optimal_eps
    eps = find_optimal_eps(c["x"], c["ms"])
    print(f"eps {eps!r} reference {c['eps']!r} rel {abs(eps - c['eps']) / c['eps']:.3e}")
    assert abs(eps - c["eps"]) <= 2e-6 * c["eps"]
    assert np.array_equal(cluster_labels(c["x"], "dbscan", c["ms"], c["metric"]), c["labels"])


# one 256-row block, the block edge, an off-diagonal block pair with both triangles of the diagonal ones, and more
# blocks than one patch row; d below one k-stage, a multiple of it, and neither
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("d", [8, 384, 770])
@pytest.mark.parametrize("n", [255, 256, 257, 513, 2049])
def test_shapes_at_the_kernel_edges(n, d, metric):
    x = blobs(n, d, 7 * n + d)
    rows = x if metric == "euclidean" else cr.normalize_rows(x)
    eps = eps_between_pairs(cr.distances(rows, metric), 0.08)
    labels, stats, stored = device_and_rows(x, eps, 4, metric)
    ref = cr.dbscan_ref(stored, eps, 4, metric)
    print(f"n={n} d={d} {metric}: eps={eps:.6g} stats={stats}")
    assert np.array_equal(labels, ref)
    assert stats["n_clusters"] == ref.max() + 1 and stats["n_noise"] == int((ref < 0).sum())


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("d", [8, 384, 770])
def test_tiny_inputs(d, metric):
    x = blobs(3, d, d)
    one, _, _ = device_and_rows(x[:1], 0.5, 1, metric)
    assert one.tolist() == [0]                         # min_samples = 1: a single row is its own cluster
    one, _, _ = device_and_rows(x[:1], 0.5, 2, metric)
    assert one.tolist() == [-1]
    two, _, _ = device_and_rows(x[:2], 1e3, 3, metric)  # n < min_samples: nothing can be core
    assert two.tolist() == [-1, -1]
    far = np.eye(3, d, dtype=np.float32)               # min_samples = 1 and nothing within eps: every row its own cluster
    lab, _, _ = device_and_rows(far, 0.01, 1, metric)
    assert lab.tolist() == [0, 1, 2]


def test_chain_on_a_line_is_one_cluster():
    # 1 500 core rows on a line, spacing 0.8 eps, in shuffled row order, across six row blocks.  At coordinates up to 60
    # the f16 image cannot decide the close pairs: they are listed (more than the list's first size) and re-scored, and
    # the unions of the listed pairs and the pointer jumping must carry the chain from end to end
    n, eps = 1500, 0.05
    x = _line(np.arange(n) * (0.8 * eps))
    order = np.random.default_rng(5).permutation(n)
    labels, stats, _ = device_and_rows(x[order], eps, 2, "euclidean")
    print(stats)
    assert (labels == 0).all() and stats["n_clusters"] == 1 and stats["n_core"] == n
    assert stats["n_rescored_in"] >= n - 1
    labels, stats, _ = device_and_rows(x[order], 0.7 * 0.8 * eps, 2, "euclidean")  # eps below the spacing: no chain
    assert (labels == -1).all() and stats["n_clusters"] == 0


def test_chain_decided_by_the_tile_walk_is_one_cluster():
    # 1 000 rows, row k = 0.5 on coordinates [k, k + 8): neighbours in the chain are sqrt(0.5) apart, the next but one
    # is 1.0 apart; eps = sqrt(0.5) / 0.8.  Values exact in f16, norms small: the tile walk decides every pair itself,
    # so its unions and the pointer jumping carry the chain across the four row blocks, in shuffled row order
    n, W = 1000, 8
    x = np.zeros((n, n + W), dtype=np.float32)
    for k in range(n):
        x[k, k:k + W] = 0.5
    order = np.random.default_rng(6).permutation(n)
    labels, stats, _ = device_and_rows(x[order], float(np.sqrt(0.5) / 0.8), 2, "euclidean")
    print(stats)
    assert (labels == 0).all() and stats["n_clusters"] == 1 and stats["n_core"] == n and stats["n_rescored"] == 0
    labels, stats, _ = device_and_rows(x[order], 0.7, 2, "euclidean")  # eps below the spacing
    assert (labels == -1).all() and stats["n_clusters"] == 0


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_identical_rows_are_one_cluster(metric):
    x = np.tile(np.random.default_rng(2).standard_normal((1, 40)).astype(np.float32), (300, 1))
    labels, stats, _ = device_and_rows(x, 0.1, 5, metric)
    assert (labels == 0).all() and stats["n_core"] == 300


def _line(coords, d=8):
    x = np.zeros((len(coords), d), dtype=np.float32)
    x[:, 0] = coords
    return x


def test_shared_border_row_takes_the_smaller_label():
    # rows 0-3: cluster at 2.7..3.6; row 4: 1.8, within 1 of 2.7 and of 0.9 but with only three rows in reach; rows 5-8:
    # cluster at 0..0.9
    x = _line([2.7, 3.0, 3.3, 3.6, 1.8, 0.0, 0.3, 0.6, 0.9])
    labels, stats, rows = device_and_rows(x, 1.0, 4, "euclidean")
    assert labels.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1] and stats["n_core"] == 8
    assert np.array_equal(labels, cr.dbscan_ref(rows, 1.0, 4))


def test_labels_rank_by_smallest_core_row_not_smallest_member():
    # row 0 is a border row of the cluster whose core rows come last
    x = _line([11.8, 0.0, 0.3, 0.6, 0.9, 10.0, 10.3, 10.6, 10.9])
    labels, _, rows = device_and_rows(x, 1.0, 4, "euclidean")
    assert labels.tolist() == [1, 0, 0, 0, 0, 1, 1, 1, 1]
    assert np.array_equal(labels, cr.dbscan_ref(rows, 1.0, 4))


def test_dense_cluster_lists_no_pairs():
    # 8 192 rows, every one of the 3.3e7 pairs inside eps and far from it: nothing is listed, nothing re-scored
    x = (np.random.default_rng(3).standard_normal((8192, 32)) * 0.01).astype(np.float32)
    labels, stats, _ = device_and_rows(x, 1.0, 5, "euclidean")
    print(stats)
    assert (labels == 0).all()
    assert stats["n_clusters"] == 1 and stats["n_core"] == 8192 and stats["n_noise"] == 0
    assert stats["n_rescored"] == 0 and stats["list_regrown"] == 0


def test_pairs_inside_the_f16_band_are_rescored():
    # 24 pairs far from each other; within a pair the distance is eps * (1 + delta), delta on both sides of 0 and beyond
    # the 4e-6 margin.  At coordinates of this size the f16 image cannot tell them apart: all are re-scored
    eps = 0.37
    deltas = np.array([-1e-3, -1e-4, -1e-5, 1e-5, 1e-4, 1e-3])
    a = np.repeat(np.arange(24, dtype=np.float64) * 3.0 + 1.0, 2)
    a[1::2] += eps * (1.0 + np.tile(deltas, 4))
    x = _line(a.astype(np.float32))
    D = cr.distances(x, "euclidean")
    assert (np.abs(D[np.triu_indices(48, 1)] - eps) / eps > 4e-6).all()
    labels, stats, rows = device_and_rows(x, eps, 2, "euclidean")
    ref = cr.dbscan_ref(rows, eps, 2)
    print(stats)
    assert stats["n_rescored"] >= 24 and 0 < stats["n_rescored_in"] < stats["n_rescored"]
    assert np.array_equal(labels, ref) and ref.max() >= 1 and (ref < 0).any()


def test_argument_errors():
    from anorag_hip import METRIC_IP, METRIC_L2, FlatIndex, _lib
    from anorag_hip.topic_clustering import cluster_labels, dbscan_labels, find_optimal_eps
    lib = _lib.load()
    x = blobs(64, 16, 1)
    idx = _index(x, "euclidean")
    lab = np.empty(64, dtype=np.int32)
    call = lambda h, eps, ms: lib.anr_index_dbscan(h, C.c_double(eps), ms, lab.ctypes.data, None)  # noqa: E731
    assert call(idx._h, float("nan"), 3) == -1 and call(idx._h, -0.5, 3) == -1 and call(idx._h, 0.5, 0) == -1
    assert call(None, 0.5, 3) == -1
    assert call(idx._h, 0.5, 3) == 0
    idx.close()
    ip = FlatIndex(16, METRIC_IP, normalize=False)
    ip.add(x)
    assert call(ip._h, 0.5, 3) == -1 and b"cosine" in lib.anr_last_error()
    with pytest.raises(ValueError):
        dbscan_labels(ip, 0.5, 3, "cosine")
    ip.close()
    empty = FlatIndex(16, METRIC_L2)
    lab[:] = 77
    assert call(empty._h, 0.5, 3) == 0 and (lab == 77).all()
    assert dbscan_labels(empty, 0.5).shape == (0,)
    empty.close()
    with pytest.raises(ValueError):
        dbscan_labels(x, 0.5, 3, "manhattan")
    with pytest.raises(ValueError):
        find_optimal_eps(x[:2], 3)
    for algo in ("hdbscan", "kmeans"):
        with pytest.raises(NotImplementedError, match="sklearn"):
            cluster_labels(x, algo)
    with pytest.raises(ValueError):
        cluster_labels(x, "spectral")


def test_values_beyond_f16_are_refused():
    from anorag_hip import _lib
    x = blobs(64, 16, 1)
    x[5, 3] = 1.0e5
    idx = _index(x, "euclidean")
    lab = np.empty(64, dtype=np.int32)
    assert _lib.load().anr_index_dbscan(idx._h, C.c_double(0.5), 3, lab.ctypes.data, None) == -3
    idx.close()


def test_search_is_unchanged_by_dbscan():
    from anorag_hip.topic_clustering import dbscan_labels
    x = blobs(700, 96, 11)
    idx = _index(x, "euclidean")
    q = blobs(5, 96, 12)
    D0, I0 = idx.search(q, 10)
    first = dbscan_labels(idx, 4.0, 4)
    D1, I1 = idx.search(q, 10)
    assert np.array_equal(D0, D1) and np.array_equal(I0, I1)
    assert np.array_equal(first, dbscan_labels(idx, 4.0, 4)) and idx.ntotal == 700
    idx.close()
