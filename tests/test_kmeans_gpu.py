"""GPU tests of anr_index_kmeans through anorag_hip.topic_clustering: the device against the numpy restatement
(tests/kmeans_ref.py) at the smallest shapes that reach every tile, block and chunk edge of csrc/kmeans.hip, and against
the reference's own recorded output (tests/golden/kmeans_cases.npz).

Labels, n_iter and the winning init must be equal.  Centres, inertia and tol are sums whose order the restatement mirrors
(DESIGN.md §5j), so they must be bit-equal; nothing here is compared within a tolerance except the inertia against
sklearn's float32 value, which is allowed twice the largest deviation the fixture records for the restatement."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import kmeans_ref as kr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES, SKLEARN_VERSION, MAX_DEVIATION = kr.load_golden(os.path.join(HERE, "golden", "kmeans_cases.npz"))

# (N, d, k): N = 17 (one partial row tile), 255 / 257 (either side of a scan block, a sum tree and four row tiles),
# 513 (just past two scan blocks and past one 512-row update chunk); d = 5 (one partial MFMA step), 32, 384 (six
# 64-wide k-chunks, three update slabs); k = 2, 10, 16 / 17 (either side of a 16-centre block), 64 (the cap)
SHAPES = [(17, 5, 2), (255, 32, 10), (257, 5, 16), (257, 32, 17), (513, 5, 10), (255, 384, 2), (513, 384, 64), (513, 32, 17),
          (130, 384, 16)]


def shape_rows(n, d, k):
    g = np.random.default_rng(1000 * n + 10 * d + k)
    c = g.standard_normal((max(k, 3), d)) * 2.0
    return (c[g.permutation(n) % len(c)] + 0.5 * g.standard_normal((n, d))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ref_fit(n, d, k, n_init):
    return kr.fit(shape_rows(n, d, k), k, n_init)


def tc():
    from anorag_hip import topic_clustering
    return topic_clustering


def assert_equals_ref(got, want):
    labels, centres, inertia, n_iter, st = got
    assert np.array_equal(labels, want["labels"])
    assert n_iter == want["n_iter"] and st["best_init"] == want["best_init"]
    print(f"inertia {inertia!r} ref {want['inertia']!r}; tol {st['tol']!r} ref {want['tol']!r}; "
          f"max centre diff {np.max(np.abs(centres - want['centres'])):.3e}")
    assert st["tol"] == want["tol"]
    assert np.array_equal(centres, want["centres"])
    assert inertia == want["inertia"]


@pytest.mark.parametrize("n,d,k", SHAPES, ids=[f"{n}x{d}-k{k}" for n, d, k in SHAPES])
def test_device_equals_restatement(n, d, k):
    got = tc().kmeans_fit(shape_rows(n, d, k), k, 3, return_stats=True)
    assert_equals_ref(got, ref_fit(n, d, k, 3))
    assert got[0].dtype == np.int64 and got[1].shape == (k, d) and got[4]["emptied_init"] == -1


def duplicate_rows():
    g = np.random.default_rng(77)
    base = g.standard_normal((40, 7)).astype(np.float32)
    return base[g.permutation(np.repeat(np.arange(40), 3))]


def test_duplicate_rows():
    x = duplicate_rows()
    assert_equals_ref(tc().kmeans_fit(x, 5, 3, return_stats=True), kr.fit(x, 5, 3))


def test_as_many_clusters_as_distinct_rows():
    g = np.random.default_rng(78)
    base = g.standard_normal((6, 5)).astype(np.float32)
    x = base[g.permutation(np.repeat(np.arange(6), 20))]
    want = kr.fit(x, 6, 2)
    got = tc().kmeans_fit(x, 6, 2, return_stats=True)
    assert_equals_ref(got, want)
    assert got[2] == 0.0 and got[3] == 1  # every row sits on its centre: the exact zero of the shared product sequence
    assert {tuple(r) for r in got[1].astype(np.float32)} == {tuple(r) for r in base}


def test_exact_ties_go_to_the_lower_centre():
    # rows at 0 and 2 on one axis and rows at 1, exactly as far from both: whichever pair of rows seeds the centres, the
    # tied rows take the lower centre index, as numpy's argmin does in the restatement
    x = np.zeros((90, 5), dtype=np.float32)
    x[30:60, 0] = 2.0
    x[60:, 0] = 1.0
    x[:, 1] = np.tile(np.array([0.0, 0.25, -0.25], dtype=np.float32), 30)
    for seed in (0, 1, 2, 3):
        assert_equals_ref(tc().kmeans_fit(x, 2, 2, random_state=seed, return_stats=True), kr.fit(x, 2, 2, random_state=seed))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_the_reference_recorded(c):
    t, x = tc(), c["x"]
    k, inertias = t.find_optimal_k(x, return_inertias=True)
    assert k == c["k"]
    assert len(inertias) >= len(c["elbow_inertias"])
    for got, want in zip(inertias, c["elbow_inertias"]):
        print(f"elbow inertia {got!r} sklearn {want!r} rel {abs(got - want) / want:.3e}")
        assert abs(got - want) <= 2 * MAX_DEVIATION * want
    assert np.array_equal(t.kmeans_topic_labels(x), c["labels"])
    labels, _, inertia, n_iter = t.kmeans_fit(x, c["k"], 10)
    print(f"final inertia {inertia!r} sklearn {c['inertia']!r} rel {abs(inertia - c['inertia']) / c['inertia']:.3e}")
    assert np.array_equal(labels, c["labels"]) and n_iter == c["n_iter"]
    assert abs(inertia - c["inertia"]) <= 2 * MAX_DEVIATION * c["inertia"]
    assert np.array_equal(t.fallback_labels(x), c["fallback_labels"])


def test_two_calls_are_bit_equal_and_an_index_gives_the_same():
    from anorag_hip.flat_index import METRIC_L2, FlatIndex

    n, d, k = 513, 32, 17
    x = shape_rows(n, d, k)
    a = tc().kmeans_fit(x, k, 3, return_stats=True)
    index = FlatIndex(d, METRIC_L2, normalize=False, device=0)
    try:
        index.add(x[:300])
        index.add(x[300:])
        b = tc().kmeans_fit(index, k, 3, return_stats=True)
        c = tc().kmeans_fit(index, k, 3, return_stats=True)
        assert tc().find_optimal_k(index, max_k=4) == tc().find_optimal_k(x, max_k=4)
    finally:
        index.close()
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1]) and a[2:4] == other[2:4]
        assert a[4]["tol"] == other[4]["tol"] and a[4]["lloyd_iterations"] == other[4]["lloyd_iterations"]


def test_refusals():
    from anorag_hip import _lib
    from anorag_hip.flat_index import METRIC_IP, METRIC_L2, FlatIndex

    t = tc()
    x = shape_rows(70, 5, 3)
    for bad_k in (1, 0, 71, 65):
        with pytest.raises(ValueError):
            t.kmeans_fit(x, bad_k, 1)
    with pytest.raises(ValueError):
        t.kmeans_fit(np.zeros((3,), dtype=np.float32), 2, 1)
    for metric, normalize in ((METRIC_IP, True), (METRIC_IP, False), (METRIC_L2, True)):
        index = FlatIndex(5, metric, normalize=normalize, device=0)
        try:
            index.add(x)
            with pytest.raises(ValueError):
                t.kmeans_fit(index, 3, 1)
            with pytest.raises(ValueError):
                t.find_optimal_k(index)
        finally:
            index.close()
    # the C entry refuses by itself what the wrapper refuses first
    index = FlatIndex(5, METRIC_L2, normalize=False, device=0)
    try:
        index.add(x)
        first, u = t.kmeans_draws(70, 65, 1)
        labels = np.empty((70,), dtype=np.int32)
        for k, row in ((65, 0), (1, 0), (71, 0), (3, 70), (3, -1)):
            fr = np.array([row], dtype=np.int64)
            rc = index._lib.anr_index_kmeans(index._h, k, 1, u.shape[2], fr.ctypes.data, u.ctypes.data, 300, C.c_double(1e-4),
                                             labels.ctypes.data, None, None, None, None, None)
            assert rc == -1, (k, row, rc)
        assert "above the 64" in _lib.last_error() or "not a row" in _lib.last_error()
    finally:
        index.close()
    with pytest.raises(NotImplementedError):
        t.cluster_labels(x, "kmeans")


def test_an_emptied_cluster_raises_and_faults_nothing():
    t = tc()
    two = np.repeat(np.array([[0.0, 1.0, 0.5], [4.0, 2.0, -1.0]], dtype=np.float32), 10, axis=0)
    with pytest.raises(kr.EmptyCluster):
        kr.fit(two, 3, 1)
    with pytest.raises(t.EmptyClusterError) as e:
        t.kmeans_fit(two, 3, 1)
    assert "lost all its rows" in str(e.value)
    with pytest.raises(t.EmptyClusterError):
        t.find_optimal_k(two, max_k=3)
    # the device is as it was: the next fit is the restatement's
    assert_equals_ref(t.kmeans_fit(shape_rows(17, 5, 2), 2, 3, return_stats=True), ref_fit(17, 5, 2, 3))
