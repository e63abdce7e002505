#!/usr/bin/env python3
"""Developer tool: time device HDBSCAN (anorag_hip.topic_clustering.hdbscan_mst + hdbscan_tree_labels) per stage at N x d
rows on an index that already holds the rows: the core-distance pass and the Prim steps on the device (HIP events, stats
words 4 and 5), the whole anr_index_hdbscan_mst call and the host tree stage (wall clock; warm-up, then the median of
--reps), the time per Prim step against the bytes a step reads (every row once).  --sklearn N ...: beside
it sklearn's HDBSCAN(min_cluster_size=5, min_samples=3, cluster_selection_epsilon=0.1).fit_predict wall time on this box's
host at those sizes.  One JSON line per N.  Nothing here is asserted anywhere.

  python tools/hdbscan_perf.py [--n 5000 20000 100000] [--d 768] [--min-samples 3] [--reps 3] [--sklearn 2000 5000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ano-rag_amd"), ROOT]


def rows(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((12, d)).astype(np.float32)
    return centres[rng.integers(0, 12, n)] + 0.35 * rng.standard_normal((n, d), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[5000, 20000, 100000])
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--min-samples", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sklearn", type=int, nargs="*", default=[])
    a = ap.parse_args()
    from anorag_hip import METRIC_L2, FlatIndex
    from anorag_hip.topic_clustering import hdbscan_mst, hdbscan_tree_labels

    for n in a.n:
        index = FlatIndex(a.d, METRIC_L2, normalize=False, device=0)
        try:
            index.add(rows(n, a.d, n))
            t_mst, t_tree, core_us, prim_us, st = [], [], [], [], None
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                _, src, dst, w, st = hdbscan_mst(index, a.min_samples, return_stats=True)
                t1 = time.perf_counter()
                labels = hdbscan_tree_labels(src, dst, w, 5, 0.1)
                t2 = time.perf_counter()
                if rep:
                    t_mst.append(t1 - t0), t_tree.append(t2 - t1), core_us.append(st["core_us"]), prim_us.append(st["prim_us"])
            prim = statistics.median(prim_us)
            print(json.dumps({"n": n, "d": a.d, "min_samples": a.min_samples,
                              "core_ms": round(statistics.median(core_us) / 1e3, 3), "prim_ms": round(prim / 1e3, 3),
                              "us_per_prim_step": round(prim / (n - 1), 3),
                              "row_gb_per_s_in_prim": round((n - 1) * n * a.d * 4 / 1e9 / (prim / 1e6), 1),
                              "mst_call_ms": round(statistics.median(t_mst) * 1e3, 3),
                              "tree_stage_ms": round(statistics.median(t_tree) * 1e3, 3),
                              "clusters": int(labels.max()) + 1, "scratch_bytes": st["scratch_bytes"]}), flush=True)
        finally:
            index.close()
    for n in a.sklearn:
        from sklearn.cluster import HDBSCAN
        x = rows(n, a.d, n)
        t0 = time.perf_counter()
        HDBSCAN(min_cluster_size=5, min_samples=a.min_samples, cluster_selection_epsilon=0.1).fit_predict(x)
        print(json.dumps({"n": n, "d": a.d, "sklearn_host_s": round(time.perf_counter() - t0, 3)}), flush=True)


if __name__ == "__main__":
    main()
