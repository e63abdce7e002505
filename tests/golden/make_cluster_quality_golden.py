#!/usr/bin/env python3
"""Golden cases for cluster quality, produced by RUNNING THE REFERENCE's own TopicClustering._analyze_clusters
(doc/clustering.py:171-215) on seeded inputs (build container only; needs scikit-learn, scipy and the reference checkout):

  python tests/golden/make_cluster_quality_golden.py [/root/reference]

writes tests/golden/cluster_quality_cases.npz.  Data only; no reference source is copied.  doc/clustering.py is imported
the way make_cluster_golden.py imports it (stand-ins for loguru and the reference's `utils` / `config` packages, none of
which holds any of the arithmetic pinned here).

Per case c<i>: _x (float32 rows), _labels (int64), and the reference's dict taken apart: _n_clusters, _n_noise,
_size_labels / _sizes, _centers (float32 [clusters, d]: the lists hold float32 values), _q_labels / _cohesion / _std
(cluster_quality, float64, NaN kept), _silhouette (the dict's value), _types (type names of n_clusters, n_noise, a key, a
size, a centre element, a cohesion, the score), _sk_samples (sklearn's silhouette_samples on the rows cast to float64; empty
where sklearn raises) and _dev, the OBSERVED deviation of the float64 restatement (tests/cluster_quality_ref.py): [0] max
|samples - sklearn float64|, [1] |mean - the reference's silhouette_score| (the reference calls sklearn on float32 rows,
where every distance is rounded to float32), [2] max |cohesion - reference|, [3] max |std - reference|.  `names` lists
the cases.  tests/test_cluster_quality_cpu.py allows 4x the largest recorded deviation of each quantity.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cluster_quality_ref as qr  # noqa: E402
from make_cluster_golden import load_reference  # noqa: E402


def blobs(rng, n, d, k, spread=0.25, scale=1.0):
    centres = rng.standard_normal((k, d)) * scale
    lab = rng.integers(0, k, n)
    lab[:k] = np.arange(k)  # every label occurs
    x = centres[lab] + rng.standard_normal((n, d)) * spread
    return x.astype(np.float32), lab.astype(np.int64)


def make_cases():
    rng = np.random.default_rng(20251)
    cases = []

    x, lab = blobs(rng, 300, 32, 6)
    lab[rng.random(300) < 0.12] = -1
    x[lab == -1] += rng.standard_normal((int((lab == -1).sum()), 32)).astype(np.float32)
    cases.append(("dbscan_style_noise", x, lab))

    x, lab = blobs(rng, 200, 16, 5, spread=0.6)
    cases.append(("kmeans_style", x, lab))

    x, lab = blobs(rng, 150, 8, 4)
    cases.append(("non_contiguous_labels", x, np.array([-1, 3, 7, 1000])[lab]))

    x, lab = blobs(rng, 120, 24, 3)
    lab[lab == 2] = 0
    lab[17] = 2
    cases.append(("singleton_cluster", x, lab))

    x, lab = blobs(rng, 100, 64, 2)
    cases.append(("two_clusters", x, lab))

    x, lab = blobs(rng, 90, 16, 2, spread=0.1)
    keep = np.zeros(90, dtype=bool)
    keep[np.flatnonzero(lab == 0)[:6]] = True
    keep[np.flatnonzero(lab == 1)[:5]] = True
    lab[~keep] = -1
    x[~keep] = rng.standard_normal((int((~keep).sum()), 16)).astype(np.float32) * 2
    cases.append(("all_noise_but_two_clusters", x, lab))

    cases.append(("degenerate_0_1_noise", rng.standard_normal((3, 8)).astype(np.float32), np.array([0, 1, -1])))

    x, _ = blobs(rng, 50, 8, 1)
    cases.append(("one_cluster", x, np.zeros(50, dtype=np.int64)))

    x, lab = blobs(rng, 80, 16, 3)
    x[40:60] = x[20:40]
    lab[40:60] = lab[20:40]
    x[60:64] = x[0]  # the same row under whatever labels these four have
    cases.append(("duplicated_rows", x, lab))

    x, lab = blobs(rng, 60, 12, 3)
    x[np.flatnonzero(lab == 1)[2]] = 0.0
    cases.append(("zero_row_in_cluster", x, lab))

    x, lab = blobs(rng, 500, 48, 7)
    lab[rng.random(500) < 0.08] = -1
    lab[lab == 6] = 5
    lab[123] = 6
    cases.append(("seven_clusters_noise_singleton", x, lab))

    cases.append(("every_row_its_own_cluster", rng.standard_normal((4, 8)).astype(np.float32), np.arange(4)))
    return cases


def main():
    from sklearn.metrics import silhouette_samples
    TopicClustering = load_reference()
    tc = TopicClustering()
    out = {"names": np.array([c[0] for c in make_cases()])}
    worst = np.zeros(4)
    for i, (name, x, lab) in enumerate(make_cases()):
        assert x.dtype == np.float32 and len(x) <= 600 and x.shape[1] <= 64
        with np.errstate(all="ignore"):
            info = tc._analyze_clusters(lab, x)
        mine = qr.analyze(x, lab)
        keys = list(info["cluster_sizes"])
        centers = np.array([info["cluster_centers"][k] for k in keys], dtype=np.float64).reshape(len(keys), x.shape[1])
        assert np.array_equal(centers.astype(np.float32).astype(np.float64), centers)
        qk = list(info["cluster_quality"])
        try:
            sk = silhouette_samples(x.astype(np.float64), lab)
        except ValueError:
            sk = np.zeros((0,))
        dev = np.zeros(4)
        if sk.size:
            dev[0] = np.abs(qr.silhouette_samples(x, lab) - sk).max()
        dev[1] = abs(mine["silhouette_score"] - info["silhouette_score"])
        for k in qk:
            for j, f in ((2, "cohesion"), (3, "std")):
                a, b = mine["cluster_quality"][k][f], info["cluster_quality"][k][f]
                assert np.isnan(a) == np.isnan(b), (name, k, f)
                if not np.isnan(a):
                    dev[j] = max(dev[j], abs(a - b))
        worst = np.maximum(worst, dev)
        first = keys[0]
        types = [type(info["n_clusters"]).__name__, type(info["n_noise"]).__name__, type(first).__name__,
                 type(info["cluster_sizes"][first]).__name__, type(info["cluster_centers"][first][0]).__name__,
                 type(info["cluster_quality"][qk[0]]["cohesion"]).__name__ if qk else "",
                 type(info["silhouette_score"]).__name__]
        p = f"c{i}_"
        out[p + "x"], out[p + "labels"] = x, np.asarray(lab, dtype=np.int64)
        out[p + "n_clusters"], out[p + "n_noise"] = np.int64(info["n_clusters"]), np.int64(info["n_noise"])
        out[p + "size_labels"] = np.array(keys, dtype=np.int64)
        out[p + "sizes"] = np.array([info["cluster_sizes"][k] for k in keys], dtype=np.int64)
        out[p + "centers"] = centers.astype(np.float32)
        out[p + "q_labels"] = np.array(qk, dtype=np.int64)
        out[p + "cohesion"] = np.array([info["cluster_quality"][k]["cohesion"] for k in qk], dtype=np.float64)
        out[p + "std"] = np.array([info["cluster_quality"][k]["std"] for k in qk], dtype=np.float64)
        out[p + "silhouette"] = np.float64(info["silhouette_score"])
        out[p + "types"] = np.array(types)
        out[p + "sk_samples"] = sk
        out[p + "dev"] = dev
        print(f"{name}: n={len(x)} d={x.shape[1]} clusters={info['n_clusters']} noise={int(info['n_noise'])} "
              f"silhouette={info['silhouette_score']:.6f} dev={dev}")
    path = os.path.join(HERE, "cluster_quality_cases.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out['names'])} cases, {os.path.getsize(path)} bytes; largest deviations {worst}")
    assert worst[0] < 1e-6 and worst[1] < 1e-6
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "cluster_cases.npz"))


if __name__ == "__main__":
    main()
