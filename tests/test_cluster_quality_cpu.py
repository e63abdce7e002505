"""CPU tests of the cluster quality restatement (tests/cluster_quality_ref.py) against the goldens recorded from the
reference's own ``_analyze_clusters`` (tests/golden/make_cluster_quality_golden.py): counts, sizes and the 0.0 branches
exactly, centres bit for bit, silhouette and cohesion within 4x the largest deviation the generator observed and wrote
into the file (the margin covers sklearn rounding every distance of its float32 input to float32)."""
import inspect
import os

import numpy as np
import pytest

import cluster_quality_ref as qr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cluster_quality_cases.npz")


def load_cases():
    z = np.load(GOLDEN)
    cases = []
    for i, name in enumerate(z["names"]):
        c = {k[len(f"c{i}_"):]: z[k] for k in z.files if k.startswith(f"c{i}_")}
        c["name"] = str(name)
        cases.append(c)
    return cases


CASES = load_cases()
IDS = [c["name"] for c in CASES]
# 4x the largest recorded deviation of each quantity: [0] samples vs sklearn on float64 rows, [1] the score vs the
# reference's (float32 distances inside sklearn), [2] cohesion, [3] std
TOL = 4.0 * np.max([c["dev"] for c in CASES], axis=0)


def check_against_golden(info, c, extra=np.zeros(4)):
    """info: a cluster_info dict (the restatement's or the device's) against the reference's recorded one; `extra` is
    added to the recorded tolerances (the device's derived bounds)"""
    assert set(info) == {"n_clusters", "n_noise", "cluster_sizes", "cluster_centers", "cluster_quality", "silhouette_score"}
    assert info["n_clusters"] == int(c["n_clusters"]) and int(info["n_noise"]) == int(c["n_noise"])
    keys = list(info["cluster_sizes"])
    assert [int(k) for k in keys] == c["size_labels"].tolist()
    assert [info["cluster_sizes"][k] for k in keys] == c["sizes"].tolist()
    assert list(info["cluster_centers"]) == keys
    for k, centre in zip(keys, c["centers"]):
        got = np.array(info["cluster_centers"][k], dtype=np.float64)
        assert np.array_equal(got, centre.astype(np.float64))  # bit-equal: the same float32 values
    qk = list(info["cluster_quality"])
    assert [int(k) for k in qk] == c["q_labels"].tolist()
    for k, coh, std in zip(qk, c["cohesion"], c["std"]):
        q = info["cluster_quality"][k]
        assert set(q) == {"cohesion", "std"}
        assert np.isnan(q["cohesion"]) == np.isnan(coh) and np.isnan(q["std"]) == np.isnan(std)
        if not np.isnan(coh):
            assert abs(q["cohesion"] - coh) <= TOL[2] + extra[2]
            assert abs(q["std"] - std) <= TOL[3] + extra[3]
    if float(c["silhouette"]) == 0.0:
        assert info["silhouette_score"] == 0.0  # the reference's branches
    else:
        assert abs(info["silhouette_score"] - float(c["silhouette"])) <= TOL[1] + extra[1]
    first = keys[0]
    types = [type(info["n_clusters"]).__name__, type(info["n_noise"]).__name__, type(first).__name__,
             type(info["cluster_sizes"][first]).__name__, type(info["cluster_centers"][first][0]).__name__,
             type(info["cluster_quality"][qk[0]]["cohesion"]).__name__ if qk else "", type(info["silhouette_score"]).__name__]
    assert types == c["types"].tolist()


def test_recorded_deviations_are_small():
    dev = np.max([c["dev"] for c in CASES], axis=0)
    print("largest recorded deviations:", dev)
    assert dev[0] <= 1e-6 and dev[1] <= 1e-6  # beyond that the restatement is wrong, not the tolerance
    assert dev[2] <= 1e-12 and dev[3] <= 1e-12
    assert len(CASES) >= 12 and all(len(c["x"]) <= 600 and c["x"].shape[1] <= 64 and c["x"].dtype == np.float32 for c in CASES)
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "cluster_cases.npz"))


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_matches_reference(c):
    check_against_golden(qr.analyze(c["x"], c["labels"]), c)
    if c["sk_samples"].size:
        assert np.abs(qr.silhouette_samples(c["x"], c["labels"]) - c["sk_samples"]).max() <= TOL[0]


def test_golden_covers_the_branches():
    by = {c["name"]: c for c in CASES}
    assert float(by["degenerate_0_1_noise"]["silhouette"]) == 0.0 and int(by["degenerate_0_1_noise"]["n_clusters"]) == 2
    assert float(by["one_cluster"]["silhouette"]) == 0.0
    assert float(by["every_row_its_own_cluster"]["silhouette"]) == 0.0
    assert 1 in by["singleton_cluster"]["sizes"] and len(by["singleton_cluster"]["q_labels"]) == 2
    assert np.isnan(by["zero_row_in_cluster"]["cohesion"]).sum() == 1
    assert by["non_contiguous_labels"]["size_labels"].tolist() == [3, 7, 1000]
    assert int(by["all_noise_but_two_clusters"]["n_noise"]) > 70


def test_bounds_are_what_the_design_states():
    x = np.array([[3.0, 4.0], [0.0, 0.0], [3.0, 4.0], [6.0, 8.0]], dtype=np.float32)
    lab = np.array([0, 0, 1, 1])
    assert qr.cohesion_bound(64) == 2 * 72 * 2.0 ** -53 and qr.std_bound(64) == 4 * 72 * 2.0 ** -53
    b = qr.silhouette_bound(x, lab)
    assert b.shape == (4,) and np.all(b > 0) and np.all(b < 1e-6)  # rows 0 and 2 are equal: sqrt(E) applies there
    assert b[1] < 1e-13 and b[3] < 1e-13
    s, a, bb = qr.silhouette_parts(x, lab)
    assert a.tolist() == [5.0, 5.0, 5.0, 5.0] and bb.tolist() == [2.5, 7.5, 2.5, 7.5]
    assert np.array_equal(s, (bb - a) / np.maximum(a, bb))


def test_public_interface_exists():
    from anorag_hip import topic_clustering as tc
    for name in ("analyze_clusters", "silhouette_samples", "silhouette_score", "cluster_cohesion"):
        assert name in tc.__all__
        p = inspect.signature(getattr(tc, name)).parameters
        assert list(p)[1:] == ["labels", "device"] and p["device"].default == 0
    assert list(inspect.signature(tc.analyze_clusters).parameters)[0] == "embeddings"
    assert list(inspect.signature(tc.silhouette_samples).parameters)[0] == "embeddings_or_index"
    for name in ("cluster_labels", "dbscan_labels", "find_optimal_eps"):
        assert name in tc.__all__
