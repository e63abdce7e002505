#!/usr/bin/env python3
"""Developer tool: time anr_index_kmeans (anorag_hip.topic_clustering.kmeans_fit) at N x d rows and k clusters: wall clock
of whole fits on an index that already holds the rows (warm-up, then the median of --reps), the time per Lloyd iteration
and per assignment pass taken as the difference of a max_iter = --iters fit and a max_iter = 1 fit with the same draws
(so the seeding and the once-per-call passes cancel), and what that is against the bytes an iteration reads (DESIGN.md
§5j: the rows twice).  One JSON line per N.  Nothing here is asserted anywhere.

  python tools/kmeans_perf.py [--n 100000 1000000] [--d 768] [--k 10] [--n-init 1] [--iters 10] [--reps 3]
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

HBM_PEAK_TBS = 8.0  # MI355X


def rows(n, d, k, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((max(k, 2), d)).astype(np.float32)
    return centres[rng.integers(0, len(centres), n)] + 0.8 * rng.standard_normal((n, d), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--n-init", type=int, default=1)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from anorag_hip import METRIC_L2, FlatIndex
    from anorag_hip.topic_clustering import kmeans_fit

    def timed(index, max_iter):
        t, st = [], None
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            st = kmeans_fit(index, a.k, a.n_init, 42, return_stats=True, max_iter=max_iter, tol=0.0)[4]
            if rep:
                t.append(time.perf_counter() - t0)
        return statistics.median(t), st

    for n in a.n:
        index = FlatIndex(a.d, METRIC_L2, normalize=False, device=0)
        try:
            index.add(rows(n, a.d, a.k, n))
            t_one, st_one = timed(index, 1)
            t_many, st_many = timed(index, a.iters)
            d_iter = st_many["lloyd_iterations"] - st_one["lloyd_iterations"]
            per_iter = (t_many - t_one) / d_iter if d_iter > 0 else float("nan")
            gb = 2 * n * a.d * 4 / 1e9
            print(json.dumps({"n": n, "d": a.d, "k": a.k, "n_init": a.n_init, "fit_ms_max_iter_1": round(t_one * 1e3, 3),
                              f"fit_ms_max_iter_{a.iters}": round(t_many * 1e3, 3), "lloyd_iterations": st_many["lloyd_iterations"],
                              "ms_per_iteration": round(per_iter * 1e3, 4), "row_gb_per_iteration": round(gb, 3),
                              "share_of_hbm_peak": round(gb / 1e3 / per_iter / HBM_PEAK_TBS, 4) if per_iter > 0 else None,
                              "scratch_bytes": st_many["scratch_bytes"]}), flush=True)
        finally:
            index.close()


if __name__ == "__main__":
    main()
