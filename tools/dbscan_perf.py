#!/usr/bin/env python3
"""Developer tool: time anr_index_dbscan, find_optimal_eps and, on the same handle and rows, anr_index_self_join at a
threshold that yields few pairs (one walk of the same tiles: the yardstick for DBSCAN's three).

  python tools/dbscan_perf.py [--n 20000 100000] [--d 768] [--sklearn 20000] [--skip-eps]

Per size two corpora: clustered (64 centres) and unclustered Gaussian rows, on a cosine index (the self join is
inner-product only).  HIP events around each call after a warm-up call, median of three.  --sklearn N also times
sklearn's DBSCAN on the host at N rows (n_jobs = the CPUs the process may use).  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ano-rag_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from anorag_hip import METRIC_IP, METRIC_L2, FlatIndex  # noqa: E402
from anorag_hip.topic_clustering import dbscan_labels, find_optimal_eps  # noqa: E402


def timed(fn, reps=3):
    fn()  # warm-up
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def corpus(n, d, clustered, seed):
    rng = np.random.default_rng(seed)
    if clustered:
        cent = rng.standard_normal((64, d), dtype=np.float32)
        return cent[rng.integers(0, 64, n)] + 0.3 * rng.standard_normal((n, d), dtype=np.float32)
    return rng.standard_normal((n, d), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--sklearn", type=int, default=0)
    ap.add_argument("--skip-eps", action="store_true")
    a = ap.parse_args()
    for n in a.n:
        for clustered in (True, False):
            x = corpus(n, a.d, clustered, 1)
            idx = FlatIndex(a.d, METRIC_IP, normalize=True)
            idx.add(x)
            # cosine eps: inside a cluster 1 - cos is ~0.08 (noise 0.3 per coordinate against unit centres); Gaussian
            # rows sit at ~1.0 from each other, so the same eps finds nothing there
            eps = 0.15
            ms, (labels, st) = timed(lambda: dbscan_labels(idx, eps, 3, "cosine", return_stats=True))
            join_ms, pairs = timed(lambda: idx.self_join(0.98, sort=False))
            rec = {"n": n, "d": a.d, "corpus": "clustered64" if clustered else "gaussian", "eps": eps,
                   "dbscan_ms": round(ms, 2), "self_join_ms": round(join_ms, 2), "self_join_pairs": int(len(pairs[0])),
                   "dbscan_over_self_join": round(ms / join_ms, 2), "per_walk_over_self_join": round(ms / join_ms / st["tile_walks"], 2),
                   **st}
            idx.close()
            if not a.skip_eps:
                l2 = FlatIndex(a.d, METRIC_L2)
                l2.add(x)
                eps_ms, e = timed(lambda: find_optimal_eps(l2, 3), reps=1)
                l2.close()
                rec.update({"find_optimal_eps_ms": round(eps_ms, 1), "optimal_eps": e})
            print(json.dumps(rec), flush=True)
            if a.sklearn == n:
                from sklearn.cluster import DBSCAN
                jobs = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1
                jobs = min(jobs, int(os.environ.get("OMP_NUM_THREADS", jobs)))
                t0 = time.perf_counter()
                ref = DBSCAN(eps=eps, min_samples=3, metric="cosine", n_jobs=jobs).fit_predict(x)
                dt = time.perf_counter() - t0
                print(json.dumps({"n": n, "d": a.d, "corpus": rec["corpus"], "sklearn_dbscan_s": round(dt, 2), "n_jobs": jobs,
                                  "labels_equal_device": bool(np.array_equal(ref, labels))}), flush=True)


if __name__ == "__main__":
    main()
