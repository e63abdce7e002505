"""GPU tests of anr_index_cluster_quality and the quality functions of anorag_hip.topic_clustering: the device against
the float64 restatement (tests/cluster_quality_ref.py) within the bounds derived in DESIGN.md §5h, and, on the golden
cases, against the reference's recorded ``_analyze_clusters`` output.  Against the reference a float may differ by the
tolerance recorded for the restatement (tests/test_cluster_quality_cpu.py) plus the device's bound to the restatement."""
import ctypes as C

import numpy as np
import pytest

import cluster_quality_ref as qr
from test_cluster_quality_cpu import CASES, IDS, check_against_golden

pytestmark = pytest.mark.gpu


def _l2_index(x):
    from anorag_hip import METRIC_L2, FlatIndex
    x = np.ascontiguousarray(x, dtype=np.float32)
    idx = FlatIndex(x.shape[1], METRIC_L2, normalize=False)
    idx.add(x)
    return idx


def check_against_restatement(x, labels, q=None):
    """every output of one device call against the restatement, within the derived bounds; returns the device's dict"""
    from anorag_hip.topic_clustering import cluster_quality
    x = np.ascontiguousarray(x, dtype=np.float32)
    labels = np.asarray(labels)
    if q is None:
        q = cluster_quality(x, labels)
    uniq, counts = np.unique(labels, return_counts=True)
    assert np.array_equal(q["labels"], uniq) and np.array_equal(q["sizes"], counts)
    s = qr.silhouette_samples(x, labels)
    bound = qr.silhouette_bound(x, labels)
    err = np.abs(q["samples"] - s)
    print("silhouette: max error", err.max(), "largest error / bound", (err / np.maximum(bound, 1e-300)).max())
    assert np.all(np.isfinite(q["samples"])) and np.all(err <= bound)
    assert abs(q["mean"] - s.mean()) <= bound.mean() + 4 * 2.0 ** -53
    ref = qr.cohesion(x, labels)
    d = x.shape[1]
    for lab, m, coh, std in zip(q["labels"], q["sizes"], q["cohesion"], q["std"]):
        if int(lab) not in ref:
            assert np.isnan(coh) and np.isnan(std) and (lab < 0 or m < 2)
            continue
        rc, rs = ref[int(lab)]
        assert np.isnan(coh) == np.isnan(rc) and np.isnan(std) == np.isnan(rs)
        if not np.isnan(rc):
            print("label", lab, "cohesion error / bound", abs(coh - rc) / qr.cohesion_bound(d), "std error / bound",
                  abs(std - rs) / qr.std_bound(d))
            assert abs(coh - rc) <= qr.cohesion_bound(d) and abs(std - rs) <= qr.std_bound(d)
    return q


def clustered(n, d, labels, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    uniq, inv = np.unique(labels, return_inverse=True)
    centres = rng.standard_normal((len(uniq), d)) * 2
    return (centres[inv] + spread * rng.standard_normal((n, d))).astype(np.float32)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_golden_analyze_clusters(c):
    from anorag_hip.topic_clustering import analyze_clusters
    x, labels = c["x"], c["labels"]
    info = analyze_clusters(x, labels)
    d = x.shape[1]
    extra = np.array([0.0, qr.silhouette_bound(x, labels).mean() + 4 * 2.0 ** -53, qr.cohesion_bound(d), qr.std_bound(d)])
    check_against_golden(info, c, extra)  # structure, integers, centres bit for bit, floats near the reference's
    mine = qr.analyze(x, labels)          # floats within the derived bound of the restatement
    assert (info["silhouette_score"] == 0.0) == (mine["silhouette_score"] == 0.0)
    assert abs(info["silhouette_score"] - mine["silhouette_score"]) <= extra[1]
    for k, v in mine["cluster_quality"].items():
        got = info["cluster_quality"][k]
        if np.isnan(v["cohesion"]):
            assert np.isnan(got["cohesion"]) and np.isnan(got["std"])
        else:
            assert abs(got["cohesion"] - v["cohesion"]) <= extra[2] and abs(got["std"] - v["std"]) <= extra[3]
    check_against_restatement(x, labels)


@pytest.mark.parametrize("n", [2, 3, 31, 32, 33, 64, 65, 97, 257])
def test_row_counts_at_the_tile_edges(n):
    rng = np.random.default_rng(n)
    labels = rng.integers(-1, 3, n)
    labels[:2] = [0, 1]
    check_against_restatement(clustered(n, 19, labels, n), labels)


@pytest.mark.parametrize("d", [1, 3, 63, 64, 65, 130])
def test_dimensions_at_the_chunk_edges(d):
    rng = np.random.default_rng(100 + d)
    labels = rng.integers(0, 4, 150)
    check_against_restatement(clustered(150, d, labels, d), labels)


@pytest.mark.parametrize("first", [63, 64, 65, 128, 16, 15, 17])
def test_label_boundary_on_and_beside_a_tile_edge(first):
    labels = np.where(np.arange(200) < first, 0, 1)  # already sorted: the boundary sits at position `first`
    check_against_restatement(clustered(200, 24, labels, first), labels)


def test_forty_small_labels_inside_one_tile():
    rng = np.random.default_rng(40)
    labels = np.repeat(np.arange(40), rng.integers(1, 4, 40))
    assert len(labels) <= 120
    q = check_against_restatement(clustered(len(labels), 16, labels, 41, spread=1.0), labels)
    assert np.all(q["samples"][np.isin(labels, np.flatnonzero(np.bincount(labels) == 1))] == 0.0)


def test_one_label_over_many_tiles_beside_a_singleton():
    labels = np.zeros(700, dtype=np.int64)
    labels[333] = 5
    q = check_against_restatement(clustered(700, 32, labels, 7), labels)
    assert q["samples"][333] == 0.0 and np.isnan(q["cohesion"][1])


def test_all_noise_but_two_and_sparse_label_values():
    labels = np.full(130, -1)
    labels[[17, 90]] = [4, 4]
    check_against_restatement(clustered(130, 20, labels, 3, spread=1.0), labels)
    rng = np.random.default_rng(8)
    labels = rng.choice([-1, 7, 1000], 180)
    q = check_against_restatement(clustered(180, 20, labels, 4), labels)
    assert q["labels"].tolist() == [-1, 7, 1000]


def test_shuffled_rows_give_the_sorted_rows_values():
    from anorag_hip.topic_clustering import cluster_quality
    labels = np.repeat(np.array([-1, 2, 3, 9]), [50, 70, 1, 90])
    x = clustered(len(labels), 33, labels, 11)
    order = np.random.default_rng(12).permutation(len(labels))
    assert not np.array_equal(np.sort(labels[order]), labels[order])
    q = check_against_restatement(x[order], labels[order])
    q0 = cluster_quality(x, labels)
    # the sort is stable, so a shuffle changes the order of the additions: equal within twice the bound, not bit for bit
    bound = qr.silhouette_bound(x, labels)
    assert np.all(np.abs(q["samples"] - q0["samples"][order]) <= 2 * bound[order])


def test_identical_rows():
    from anorag_hip.topic_clustering import cluster_quality
    rng = np.random.default_rng(21)
    x = np.vstack([np.tile(rng.standard_normal((1, 40)), (70, 1)), 50.0 + rng.standard_normal((30, 40))]).astype(np.float32)
    labels = np.repeat([0, 1], [70, 30])
    q = check_against_restatement(x, labels)
    assert np.all(q["samples"][:70] == 1.0)  # a = 0 exactly: the squared norms come from the same product loop
    assert abs(q["cohesion"][0]) <= qr.cohesion_bound(40) and abs(q["std"][0]) <= qr.std_bound(40)
    same = np.tile(rng.standard_normal((1, 40)), (90, 1)).astype(np.float32)
    q = cluster_quality(same, np.arange(90) % 2)
    assert np.all(q["samples"] == 0.0) and q["mean"] == 0.0  # 0 / 0


def test_near_simplex_std_is_not_a_difference_of_squares():
    from anorag_hip.topic_clustering import cluster_cohesion
    d = 64
    x = (np.eye(24, d) + 1e-4 * np.random.default_rng(33).standard_normal((24, d))).astype(np.float32)
    labels = np.zeros(24, dtype=np.int64)
    mean, std = qr.cohesion(x, labels)[0]
    assert abs(mean - 1.0) < 1e-3 and std < 1e-3  # every pair near 1; sum c^2 - m mean^2 would lose std entirely
    got = cluster_cohesion(x, labels)[0]
    print("std", got["std"], "restatement", std, "error", abs(got["std"] - std))
    assert abs(got["std"] - std) <= 4 * (d + 8) * 2.0 ** -53
    assert abs(got["cohesion"] - mean) <= qr.cohesion_bound(d)


def test_zero_row_makes_its_cluster_nan_only():
    labels = np.repeat([0, 1, 2], [30, 40, 20])
    x = clustered(90, 12, labels, 5)
    x[35] = 0.0
    q = check_against_restatement(x, labels)
    assert np.isnan(q["cohesion"]).tolist() == [False, True, False] and np.isnan(q["std"]).tolist() == [False, True, False]
    assert np.all(np.isfinite(q["samples"]))


def test_two_calls_and_both_entry_forms_are_bit_equal():
    from anorag_hip.topic_clustering import analyze_clusters, cluster_quality
    rng = np.random.default_rng(77)
    labels = rng.integers(-1, 12, 1500)
    x = clustered(1500, 48, labels, 78)
    idx = _l2_index(x)
    try:
        runs = [cluster_quality(x, labels), cluster_quality(x, labels), cluster_quality(idx, labels), cluster_quality(idx, labels)]
    finally:
        idx.close()
    for r in runs[1:]:
        for k in ("labels", "sizes", "samples", "cohesion", "std"):
            assert np.array_equal(r[k], runs[0][k], equal_nan=True), k
        assert r["mean"] == runs[0]["mean"]
    assert repr(analyze_clusters(x, labels)) == repr(analyze_clusters(x, labels))
    check_against_restatement(x, labels, runs[0])


def test_values_beyond_the_f16_range():
    rng = np.random.default_rng(91)
    labels = rng.integers(0, 3, 120)
    x = (clustered(120, 30, labels, 92) * 1e5).astype(np.float32)
    assert np.abs(x).max() > 65504
    check_against_restatement(x, labels)


def test_public_functions_follow_sklearn_and_scipy():
    from anorag_hip.topic_clustering import cluster_cohesion, silhouette_samples, silhouette_score
    c = CASES[IDS.index("dbscan_style_noise")]
    x, labels = c["x"], c["labels"]
    s = silhouette_samples(x, labels)
    assert np.all(np.abs(s - c["sk_samples"]) <= qr.silhouette_bound(x, labels) + 4 * float(c["dev"][0]))
    assert abs(silhouette_score(x, labels) - float(c["silhouette"])) <= 4 * float(c["dev"][1]) + 1e-12
    coh = cluster_cohesion(x, labels)
    assert sorted(coh) == c["q_labels"].tolist() and all(set(v) == {"cohesion", "std"} for v in coh.values())
    with pytest.raises(ValueError, match="Number of labels is 1"):
        silhouette_score(x, np.zeros(len(x), dtype=np.int64))
    with pytest.raises(ValueError, match="Number of labels is 3"):
        silhouette_samples(x[:3], [0, 1, -1])


def test_argument_errors():
    from anorag_hip import METRIC_IP, METRIC_L2, FlatIndex, _lib
    from anorag_hip.topic_clustering import cluster_quality
    lib = _lib.load()
    x = np.random.default_rng(3).standard_normal((40, 16)).astype(np.float32)
    lab = (np.arange(40) % 4).astype(np.int32)
    n_labels = C.c_int64(0)
    call = lambda h, labels, cap, out: lib.anr_index_cluster_quality(  # noqa: E731
        h, labels, None, None, cap, out, None, None, None, C.addressof(n_labels), None)
    out = np.zeros(8, dtype=np.int32)
    for metric, normalize in ((METRIC_IP, False), (METRIC_IP, True), (METRIC_L2, True)):
        bad = FlatIndex(16, metric, normalize=normalize)
        bad.add(x)
        assert call(bad._h, lab.ctypes.data, 8, out.ctypes.data) == -1
        with pytest.raises(ValueError):
            cluster_quality(bad, lab)
        bad.close()
    idx = _l2_index(x)
    assert call(None, lab.ctypes.data, 8, out.ctypes.data) == -1
    assert call(idx._h, None, 8, out.ctypes.data) == -1
    assert call(idx._h, lab.ctypes.data, 3, out.ctypes.data) == -1 and n_labels.value == 4  # reports the count needed
    assert b"4 distinct labels" in lib.anr_last_error()
    assert call(idx._h, lab.ctypes.data, 4, out.ctypes.data) == 0 and out[:4].tolist() == [0, 1, 2, 3]
    assert call(idx._h, lab.ctypes.data, 0, None) == 0 and n_labels.value == 4  # no per-label output: no capacity needed
    for wrong in (lab[:39], np.zeros((40, 1), dtype=np.int32), np.zeros(40)):
        with pytest.raises(ValueError):
            cluster_quality(idx, wrong)
    idx.close()
    empty = FlatIndex(16, METRIC_L2)
    n_labels.value = -7
    assert call(empty._h, None, 0, None) == 0 and n_labels.value == -7  # nothing written
    q = cluster_quality(empty, np.zeros(0, dtype=np.int64))
    assert q["labels"].size == 0 and q["samples"].size == 0
    empty.close()


def test_search_is_unchanged_by_a_quality_call():
    from anorag_hip.topic_clustering import cluster_quality
    rng = np.random.default_rng(55)
    x = rng.standard_normal((700, 32)).astype(np.float32)
    idx = _l2_index(x)
    try:
        before = idx.search(x[:16], 10)
        cluster_quality(idx, rng.integers(-1, 6, 700))
        after = idx.search(x[:16], 10)
        assert idx.ntotal == 700
    finally:
        idx.close()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
