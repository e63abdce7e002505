"""CPU tests of the k-means restatement (tests/kmeans_ref.py) against the goldens recorded from the reference's
TopicClustering and sklearn (tests/golden/make_kmeans_golden.py), of the host-side random draws against sklearn's own, and
of the C ABI's new entry."""
import os

import numpy as np
import pytest

import kmeans_ref as kr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "kmeans_cases.npz")
CASES, SKLEARN_VERSION, MAX_DEVIATION = kr.load_golden(GOLDEN)
IDS = [c["name"] for c in CASES]


def dot_of(c):
    return "blas" if c["x"].size > 100_000 else "ordered"


def test_golden_set_covers_what_it_must():
    names = set(IDS)
    assert {"blobs-600x32-s1", "unit-900x64-s2", "gauss-500x16-s3", "unit-2000x384-s4"} <= names
    assert any(len(c["elbow_inertias"]) == 0 and len(c["x"]) // 5 < 2 for c in CASES)   # max_k < 2
    assert any(len(c["elbow_inertias"]) == 0 and len(c["x"]) // 5 == 2 for c in CASES)  # one k: fewer than two inertias
    assert any(len(c["elbow_inertias"]) == 2 for c in CASES)                            # fewer than three k
    assert os.path.getsize(GOLDEN) < (1 << 20)
    assert 0 < MAX_DEVIATION < 1e-6 and max(c["deviation"] for c in CASES) == MAX_DEVIATION


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_reproduces_the_recorded_case(c):
    x, dot = c["x"], dot_of(c)
    k, inertias, margin = kr.find_optimal_k(x, dot=dot)
    assert k == c["k"]
    for got, want in zip(inertias, c["elbow_inertias"]):
        assert abs(got - want) <= c["deviation"] * abs(want)
    f = kr.fit(x, c["k"], 10, dot=dot)
    assert np.array_equal(f["labels"], c["labels"]) and f["n_iter"] == c["n_iter"]
    assert abs(f["inertia"] - c["inertia"]) <= c["deviation"] * c["inertia"]
    fk = min(8, max(2, len(x) // 10))
    b = kr.fit(x, fk, 1, dot=dot)
    assert np.array_equal(b["labels"], c["fallback_labels"]) and b["n_iter"] == c["fallback_n_iter"]
    assert abs(b["inertia"] - c["fallback_inertia"]) <= c["deviation"] * c["fallback_inertia"]
    margin = min(margin, f["margin"], b["margin"])
    print(f"{c['name']}: margin {margin:.3e} (recorded {c['margin']:.3e}), deviation bound {c['deviation']:.3e}")
    # a condition on the inputs: no recorded decision hangs on a rounding
    assert margin > 1e-7 and c["margin"] > 1e-7


def test_host_draws_are_sklearns():
    """One Lloyd iteration cannot move sklearn's centres off the means of the first assignment, so the centres of
    KMeans(max_iter=1) are a function of the seeding alone: they must equal the means taken around the rows the device
    would be told to start from."""
    import warnings

    from sklearn.cluster import KMeans

    from anorag_hip.topic_clustering import kmeans_draws

    x = kr.make_rows("blobs", 40, 6, 11)
    for k, n_init in ((2, 1), (3, 4), (8, 3)):
        first, u = kmeans_draws(len(x), k, n_init, 42)
        rf, ru = kr.draws(len(x), k, n_init, 42)
        assert np.array_equal(first, rf) and np.array_equal(u, ru) and u.shape == (n_init, k - 1, 2 + int(np.log(k)))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            km = KMeans(n_clusters=k, random_state=42, n_init=n_init, max_iter=1).fit(x.copy())
        f = kr.fit(x, k, n_init, first=first, u=u, max_iter=1)
        assert np.array_equal(km.labels_, f["labels"])
        assert np.allclose(km.cluster_centers_, f["centres"], rtol=0, atol=1e-5)
        # and a stream that is one draw off gives other centres
        g = kr.fit(x, k, n_init, first=(first + 1) % len(x), u=u, max_iter=1)
        assert not np.allclose(km.cluster_centers_, g["centres"], rtol=0, atol=1e-5)


def test_restatement_orders():
    g = np.random.default_rng(5)
    v = g.random(700)
    assert abs(kr.ordered_sum(v) - v.sum()) < 1e-10
    cs = kr.block_scan(v)
    assert np.allclose(cs, np.cumsum(v), rtol=1e-13) and kr.first_reaching(cs, cs[511] * (1 + 1e-12)) == 512
    assert kr.first_reaching(cs, 1e9) == 699 and kr.first_reaching(cs, 0.0) == 0
    x = g.standard_normal((600, 3))
    lab = g.integers(0, 4, 600)
    sums, cnt = kr.centre_sums(x, lab, 4)
    assert np.allclose(sums, np.stack([x[lab == j].sum(0) for j in range(4)])) and cnt.sum() == 600
    with pytest.raises(kr.EmptyCluster):  # two distinct points, three centres
        kr.fit(np.repeat(np.array([[0.0, 1.0], [4.0, 2.0]], dtype=np.float32), 10, axis=0), 3, 1)


def test_library_exports_and_binds_kmeans():
    from anorag_hip import _lib, topic_clustering as tc

    lib = _lib.load()
    assert hasattr(lib, "anr_index_kmeans") and "anr_index_kmeans" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["anr_index_kmeans"][1]) == 14 and _lib.ANR_EEMPTY == -6
    for name in ("kmeans_fit", "find_optimal_k", "kmeans_topic_labels", "fallback_labels", "EmptyClusterError"):
        assert name in tc.__all__ and hasattr(tc, name)
    with pytest.raises(NotImplementedError):
        tc.cluster_labels(np.zeros((4, 2), dtype=np.float32), "kmeans")
