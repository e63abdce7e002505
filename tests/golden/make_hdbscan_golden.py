#!/usr/bin/env python3
"""Golden cases for HDBSCAN topic clustering, produced by RUNNING THE REFERENCE's own TopicClustering._cpu_clustering with
clustering.algorithm = hdbscan (doc/clustering.py:73-79, :99) and sklearn's own core distances and spanning tree on seeded
inputs (build container only; needs scikit-learn and the reference checkout):

  python tests/golden/make_hdbscan_golden.py [/root/reference]

writes tests/golden/hdbscan_cases.npz.  Per case i: kind / n / d / seed (tests/hdbscan_ref.py make_rows), min_samples,
min_cluster_size, eps, via_reference, n_ties (tied edges of the tree) and the rows' float64 checksum; c<i>_x, the float32
rows, unless they exceed 256 KiB (then the seed alone); c<i>_labels, the reference's labels; c<i>_core, the core distances
of sklearn's KD-tree; c<i>_src / c<i>_dst / c<i>_w, sklearn's mst_from_data_matrix.  File-wide: sklearn_version.  Data
only; no reference source is copied; the reference's loguru / utils / config imports are the stand-ins of
make_cluster_golden.py.

via_reference = 1: the labels are _cpu_clustering's (its eps is 0.1 always).  via_reference = 0: the one case in the call
shape of optimize_clustering_parameters (:388-393), HDBSCAN(min_cluster_size, min_samples, metric) with eps 0, which
_cpu_clustering cannot be made to issue.

A case is written only if
  (a) the restatement's core distances and spanning tree are bit-equal to sklearn's;
  (b) the restatement's labels equal the recorded ones under BOTH tie orders, 'stable' and 'reversed': the recorded labels
      then do not hang on the order numpy's unstable argsort gives equal weights on whatever CPU;
  (c) it is not all noise, unless it is the one case that is meant to be;
the script fails otherwise.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import hdbscan_ref as hr  # noqa: E402
import make_cluster_golden as mcg  # noqa: E402  (the stand-ins and the loader of doc/clustering.py)

STORE_ROWS_BELOW = 256 << 10
KINDS = ("blobs", "dups", "lattice", "gauss")
# (kind, n, d, seed, min_cluster_size, min_samples, eps, all_noise)
CASES = [
    ("blobs", 400, 64, 0, 5, 3, 0.1, False),
    ("dups", 450, 64, 3, 5, 3, 0.1, False),    # a block of 9 identical rows: zero weights, lambda = inf
    ("blobs", 257, 5, 2, 5, 3, 0.1, False),    # neither N nor d a multiple of 64
    ("blobs", 300, 16, 3, 10, 3, 0.0, False),  # the parameter grid's call shape
    ("blobs", 300, 16, 4, 5, 1, 0.1, False),   # min_samples = 1: core distance 0, plain single linkage
    ("gauss", 200, 32, 5, 5, 3, 0.1, False),   # mostly noise
    ("blobs", 500, 8, 8, 8, 5, 0.1, False),
    ("blobs", 500, 4, 9, 5, 2, 0.1, False),
    ("gauss", 60, 32, 11, 5, 3, 0.1, True),    # all noise, on purpose
    ("blobs", 2000, 384, 10, 5, 3, 0.1, False),  # the seed alone
]


def main():
    import sklearn
    from sklearn.cluster import HDBSCAN
    from sklearn.cluster._hdbscan._linkage import mst_from_data_matrix
    from sklearn.metrics import DistanceMetric
    from sklearn.neighbors import NearestNeighbors
    TopicClustering = mcg.load_reference()
    dm = DistanceMetric.get_metric("euclidean")
    names = ("kind", "n", "d", "seed", "min_cluster_size", "min_samples", "eps", "via_reference", "n_ties", "checksum")
    out = {k: [] for k in names}
    arrays = {}
    for i, (kind, n, d, seed, mcs, ms, eps, all_noise) in enumerate(CASES):
        x = hr.make_rows(kind, n, d, seed)
        via = eps == 0.1
        if via:
            mcg.OVERRIDES.clear()
            mcg.OVERRIDES.update({"clustering.algorithm": "hdbscan", "clustering.min_cluster_size": mcs,
                                  "clustering.min_samples": ms, "clustering.metric": "euclidean"})
            labels = np.asarray(TopicClustering()._cpu_clustering(x.copy()), dtype=np.int64)
        else:
            labels = np.asarray(HDBSCAN(min_cluster_size=mcs, min_samples=ms, metric="euclidean").fit_predict(x.copy()),
                                dtype=np.int64)
        x64 = np.ascontiguousarray(x, dtype=np.float64)
        nd, _ = NearestNeighbors(n_neighbors=ms, algorithm="kd_tree", leaf_size=40).fit(x64).kneighbors(
            x64, ms, return_distance=True)
        core = np.ascontiguousarray(nd[:, -1])
        mst = mst_from_data_matrix(x64, core, dm, 1.0)
        src, dst = mst["current_node"].astype(np.int64), mst["next_node"].astype(np.int64)
        w = np.ascontiguousarray(mst["distance"], dtype=np.float64)

        where = f"case {i} {kind} {n}x{d} seed {seed}"
        r_core = hr.core_distances(x, ms)
        r_src, r_dst, r_w = hr.prim_mst(x, r_core)
        if not (np.array_equal(r_core, core) and np.array_equal(r_src, src) and np.array_equal(r_dst, dst)
                and np.array_equal(r_w, w)):
            raise SystemExit(f"{where}: (a) the restatement's core distances or tree differ from sklearn's; not written")
        for order in ("stable", "reversed"):
            if not np.array_equal(hr.labels_from_mst(src, dst, w, mcs, eps, order), labels):
                raise SystemExit(f"{where}: (b) the labels under tie order {order!r} differ from the reference's; not written")
        if bool((labels < 0).all()) != all_noise:
            raise SystemExit(f"{where}: (c) all noise: {bool((labels < 0).all())}, meant: {all_noise}; not written")
        ties = hr.count_ties(w)
        print(f"case {i}: {kind} {n}x{d} seed {seed} mcs={mcs} ms={ms} eps={eps}: {int(labels.max()) + 1} clusters, "
              f"{int((labels < 0).sum())} noise rows, {ties} tied edges")
        for key, v in zip(names, (KINDS.index(kind), n, d, seed, mcs, ms, eps, int(via), ties,
                                  float(x.astype(np.float64).sum()))):
            out[key].append(v)
        if x.nbytes <= STORE_ROWS_BELOW:
            arrays[f"c{i}_x"] = x
        arrays[f"c{i}_labels"], arrays[f"c{i}_core"] = labels, core
        arrays[f"c{i}_src"], arrays[f"c{i}_dst"], arrays[f"c{i}_w"] = src, dst, w
    for key in out:
        arrays[key] = np.array(out[key], dtype=np.float64 if key in ("eps", "checksum") else np.int64)
    arrays["sklearn_version"] = np.array(sklearn.__version__)
    assert len(CASES) >= 8 and sum(t > 0 for t in out["n_ties"]) >= 5
    path = os.path.join(HERE, "hdbscan_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(CASES)} cases, sklearn {sklearn.__version__}, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
