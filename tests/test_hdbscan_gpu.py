"""GPU tests of device HDBSCAN (anr_index_hdbscan_mst + the host tree stage): core distances and Prim's spanning tree
bit-equal to sklearn's (stored in tests/golden/hdbscan_cases.npz) and to the numpy restatement (tests/hdbscan_ref.py) at
every tile edge and on inputs where ties decide every step; labels equal to the reference's."""
import contextlib

import numpy as np
import pytest

import hdbscan_ref as hr

CASES = hr.load_cases()
CASE_IDS = [c["id"] for c in CASES]

pytestmark = pytest.mark.gpu


def tc():
    from anorag_hip import topic_clustering
    return topic_clustering


@contextlib.contextmanager
def flat_index(d, metric, normalize):
    from anorag_hip import FlatIndex
    index = FlatIndex(d, metric, normalize=normalize, device=0)
    try:
        yield index
    finally:
        index.close()


def assert_tree_equal(got, exp):
    for name, a, b in zip(("core", "src", "dst", "w"), got, exp):
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{name}: {int((a != b).sum())} of {a.size} differ"


def restated(x, ms):
    core = hr.core_distances(x, ms)
    return (core,) + hr.prim_mst(x, core)


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_core_distances_and_tree_are_sklearns_bit_for_bit_on_every_golden(c):
    got = tc().hdbscan_mst(c["x"], c["min_samples"], return_stats=True)
    assert_tree_equal(got[:4], (c["core"], c["src"], c["dst"], c["w"]))
    st = got[4]
    assert st["prim_steps"] == c["n"] - 1 and st["partials_per_step"] == -(-c["n"] // 128)
    assert st["core_tiles"] == (-(-c["n"] // 64)) ** 2 and st["scratch_bytes"] > 0


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_labels_are_the_references_on_every_golden(c):
    if c["eps"] == 0.1:
        labels = tc().hdbscan_topic_labels(c["x"], c["min_cluster_size"], c["min_samples"])
    else:  # the parameter grid's call shape: no epsilon
        labels = tc().hdbscan_labels(c["x"], c["min_cluster_size"], c["min_samples"])
    assert labels.dtype == np.int64 and np.array_equal(labels, c["labels"])


# inputs with no stored answer: the restatement is the checker.  lattice: equal distances everywhere, ties span the
# workgroups' partials (128 rows each) and the lowest row must win; dups: a block of 9 identical rows
TIE_HEAVY = [("lattice", 257, 5, 7, 3), ("lattice", 1000, 3, 8, 3), ("dups", 300, 96, 2, 3), ("lattice", 300, 2, 9, 1)]
SHAPES = ([("blobs", 130, d, 20 + d, 3) for d in (1, 5, 63, 64, 65, 100)]
          + [("gauss", n, 7, 40 + n, 2) for n in (2, 63, 64, 65, 257)]
          + [("blobs", 70, 6, 50 + ms, ms) for ms in (1, 2, 3, 5, 16)] + [("blobs", 12, 6, 57, 12)])  # min_samples = N


@pytest.mark.parametrize("kind,n,d,seed,ms", TIE_HEAVY + SHAPES, ids=lambda v: str(v))
def test_core_distances_and_tree_equal_the_restatement(kind, n, d, seed, ms):
    x = hr.make_rows(kind, n, d, seed)
    assert_tree_equal(tc().hdbscan_mst(x, ms), restated(x, ms))


def test_the_tie_heavy_inputs_have_ties_that_cross_workgroups():
    x = hr.make_rows("lattice", 1000, 3, 8)
    _, _, dst, w = restated(x, 3)
    same = w[1:] == w[:-1]
    assert same.sum() > 500 and len({int(r) // 128 for r in dst[1:][same]}) == 8


@pytest.mark.parametrize("kind,n,d,seed,ms", TIE_HEAVY, ids=lambda v: str(v))
def test_labels_follow_the_stable_tie_order(kind, n, d, seed, ms):
    x = hr.make_rows(kind, n, d, seed)
    for mcs, eps in ((5, 0.0), (5, 0.1), (3, 1.5)):
        exp = hr.labels_from_mst(*restated(x, ms)[1:], mcs, eps, "stable")
        assert np.array_equal(tc().hdbscan_labels(x, mcs, ms, eps), exp), (mcs, eps)
    exp = hr.labels_from_mst(*restated(x, 5)[1:], 5, 0.0, "stable")
    assert np.array_equal(tc().hdbscan_labels(x, 5), exp)  # min_samples=None: min_cluster_size


def test_two_calls_give_byte_equal_results():
    x = hr.make_rows("lattice", 1000, 3, 8)
    a, b = tc().hdbscan_mst(x, 3), tc().hdbscan_mst(x, 3)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()
    assert tc().hdbscan_labels(x, 5, 3, 0.1).tobytes() == tc().hdbscan_labels(x, 5, 3, 0.1).tobytes()


def test_an_l2_index_passed_in_gives_the_arrays_result_and_other_indexes_are_refused():
    from anorag_hip import METRIC_IP, METRIC_L2
    x = hr.make_rows("blobs", 257, 5, 2)
    exp = tc().hdbscan_mst(x, 3)
    with flat_index(5, METRIC_L2, False) as index:
        index.add(x[:100])
        index.add(x[100:])
        assert_tree_equal(tc().hdbscan_mst(index, 3), exp)
        assert np.array_equal(tc().hdbscan_labels(index, 5, 3, 0.1), tc().hdbscan_labels(x, 5, 3, 0.1))
        assert index.ntotal == 257
    for metric, normalize in ((METRIC_IP, True), (METRIC_IP, False), (METRIC_L2, True)):
        with flat_index(5, metric, normalize) as index:
            index.add(x)
            with pytest.raises(ValueError, match="L2 index without normalisation"):
                tc().hdbscan_mst(index, 3)


def test_bad_arguments_raise_before_either_pass():
    x = hr.make_rows("gauss", 40, 8, 3)
    with pytest.raises(ValueError, match="above the 16"):
        tc().hdbscan_mst(x, 17)
    with pytest.raises(ValueError, match="at least 2 rows"):
        tc().hdbscan_mst(x[:1], 1)
    bad = x.copy()
    bad[7, 2] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        tc().hdbscan_mst(bad, 3)
    with pytest.raises(ValueError, match="must be at most the number of samples"):
        tc().hdbscan_mst(x[:4], 5)
    from anorag_hip import METRIC_L2
    with flat_index(8, METRIC_L2, False) as index:
        index.add(bad)
        with pytest.raises(ValueError, match="NaN or infinite"):  # found on the device: the rows are not copied back
            tc().hdbscan_mst(index, 3)
    bad[7, 2] = -np.inf
    with flat_index(8, METRIC_L2, False) as index:
        index.add(bad)
        with pytest.raises(ValueError, match="NaN or infinite"):
            tc().hdbscan_labels(index, 5, 3)
