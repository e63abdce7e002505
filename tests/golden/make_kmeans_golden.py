#!/usr/bin/env python3
"""Golden cases for k-means topic clustering, produced by RUNNING THE REFERENCE's own TopicClustering methods
(doc/clustering.py): _cpu_clustering with clustering.algorithm = kmeans (:80-87, :99), _find_optimal_k (:110-134) with its
_find_elbow_point (:136-147), and _fallback_clustering (:101-108), on seeded inputs (build container only; needs
scikit-learn and the reference checkout):

  python tests/golden/make_kmeans_golden.py [/root/reference]

writes tests/golden/kmeans_cases.npz.  Per case i: kind / n / d / seed (tests/kmeans_ref.py make_rows) and the rows' float64
checksum; c<i>_x, the float32 rows, unless they exceed 256 KiB (then the seed alone); k, the reference's _find_optimal_k;
c<i>_inertias, the inertias its loop handed to _find_elbow_point (empty where it returned 2 without calling it); c<i>_labels, _cpu_clustering's labels, with inertia and
n_iter of sklearn's same fit KMeans(k, random_state=42, n_init=10); c<i>_fallback, _fallback_clustering's labels, with
fallback_inertia / fallback_n_iter of sklearn's same fit; deviation, the largest relative difference of the restatement's
inertia (tests/kmeans_ref.py) from sklearn's float32 one over all fits of the case; margin, the restatement's smallest
relative decision margin over all fits of the case.  File-wide: sklearn_version, max_deviation.  Data only; no reference
source is copied; the reference's loguru / utils / config imports are the stand-ins of make_cluster_golden.py.

A case is written only if the restatement reproduces the reference exactly (every label of both labellings, the chosen k,
both n_iter) and its margin exceeds 1e-7, so that no recorded decision hangs on a rounding; the script fails otherwise.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import kmeans_ref as kr  # noqa: E402
import make_cluster_golden as mcg  # noqa: E402  (the stand-ins and the loader of doc/clustering.py)

MARGIN = 1e-7
STORE_ROWS_BELOW = 256 << 10
# the four cases of the issue's check, then small ones: a second elbow shape, max_k = 3 (one second difference), max_k = 2
# (fewer than three k: the first k), max_k = 1 (< 2: k = 2 without a fit) with the fallback's n_clusters floor of 2
CASES = [("blobs", 600, 32, 1), ("unit", 900, 64, 2), ("gauss", 500, 16, 3), ("unit", 2000, 384, 4),
         ("blobs", 257, 5, 5), ("blobs", 60, 8, 6), ("gauss", 17, 5, 7), ("blobs", 12, 4, 8), ("unit", 9, 6, 9)]


def rel(a, b):
    return abs(a - b) / abs(b)


def main():
    import sklearn
    from sklearn.cluster import KMeans
    TopicClustering = mcg.load_reference()
    mcg.OVERRIDES.update({"clustering.algorithm": "kmeans"})
    out = {k: [] for k in ("kind", "n", "d", "seed", "checksum", "k", "n_iter", "inertia", "fallback_inertia",
                           "fallback_n_iter", "deviation", "margin")}
    arrays = {}
    for i, (kind, n, d, seed) in enumerate(CASES):
        x = kr.make_rows(kind, n, d, seed)
        tc = TopicClustering()
        seen = {}
        elbow = tc._find_elbow_point

        def spy(k_values, inertias, seen=seen, elbow=elbow):
            seen["k_values"], seen["inertias"] = list(k_values), [float(v) for v in inertias]
            return elbow(k_values, inertias)

        tc._find_elbow_point = spy
        k = int(tc._find_optimal_k(x.copy()))
        labels = np.asarray(tc._cpu_clustering(x.copy()), dtype=np.int64)
        fallback = np.asarray(tc._fallback_clustering(x.copy()), dtype=np.int64)
        ref_inertias = np.array(seen.get("inertias", []), dtype=np.float64)
        km = KMeans(n_clusters=k, random_state=42, n_init=10).fit(x.copy())
        fk = min(8, max(2, n // 10))
        fb = KMeans(n_clusters=fk, random_state=42).fit(x.copy())
        assert np.array_equal(km.labels_, labels) and np.array_equal(fb.labels_, fallback), "sklearn is not reproducible here"

        dot = "blas" if n * d > 100_000 else "ordered"
        rk, r_inertias, margin = kr.find_optimal_k(x, dot=dot)
        rf = kr.fit(x, k, 10, dot=dot)
        rb = kr.fit(x, fk, 1, dot=dot)
        margin = min(margin, rf["margin"], rb["margin"])
        ok = (rk == k and np.array_equal(rf["labels"], labels) and np.array_equal(rb["labels"], fallback)
              and rf["n_iter"] == km.n_iter_ and rb["n_iter"] == fb.n_iter_
              and (not seen or len(r_inertias) == len(ref_inertias)))
        if not ok:
            raise SystemExit(f"case {i} {kind} {n}x{d} seed {seed}: the restatement differs from the reference; not written")
        if not margin > MARGIN:
            raise SystemExit(f"case {i} {kind} {n}x{d} seed {seed}: decision margin {margin:.3e} <= {MARGIN}; not written")
        dev = max([rel(a, b) for a, b in zip(r_inertias, ref_inertias)]
                  + [rel(rf["inertia"], float(km.inertia_)), rel(rb["inertia"], float(fb.inertia_))])
        print(f"case {i}: {kind} {n}x{d} seed {seed}: k={k} of {seen.get('k_values')} n_iter={km.n_iter_} fallback k={fk} "
              f"n_iter={fb.n_iter_} deviation={dev:.3e} margin={margin:.3e}")
        for key, v in (("kind", kr.KINDS.index(kind)), ("n", n), ("d", d), ("seed", seed),
                       ("checksum", float(x.astype(np.float64).sum())), ("k", k), ("n_iter", int(km.n_iter_)),
                       ("inertia", float(km.inertia_)), ("fallback_inertia", float(fb.inertia_)),
                       ("fallback_n_iter", int(fb.n_iter_)), ("deviation", dev), ("margin", margin)):
            out[key].append(v)
        if x.nbytes <= STORE_ROWS_BELOW:
            arrays[f"c{i}_x"] = x
        arrays[f"c{i}_labels"], arrays[f"c{i}_fallback"], arrays[f"c{i}_inertias"] = labels, fallback, ref_inertias
    for key in out:
        arrays[key] = np.array(out[key], dtype=np.float64 if key in ("checksum", "inertia", "fallback_inertia", "deviation",
                                                                      "margin") else np.int64)
    arrays["sklearn_version"] = np.array(sklearn.__version__)
    arrays["max_deviation"] = np.array(max(out["deviation"]))
    path = os.path.join(HERE, "kmeans_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(CASES)} cases, sklearn {sklearn.__version__}, max deviation {max(out['deviation']):.3e}, "
          f"smallest margin {min(out['margin']):.3e}, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
