#!/usr/bin/env python3
"""Developer tool: time anr_index_related_notes at N x 768 clustered rows (rows around N / 50 centres, 0-6 entities per row
from a pool its centre shares, seven cluster ids dealt round-robin): the nominating walks, pair scoring, sort and per-row
selection by HIP events (anr_related_timing) and the whole call by wall clock.  Next to them the self join's time on the
same index at the threshold the walk nominates at (what tools/join_perf.py times): the yardstick for the walk, which
multiplies the same tiles.  Warm-up, then the median of --reps calls; one JSON line per N.

  python tools/related_perf.py [--n 10000 100000] [--d 768] [--reps 3] [--threshold 0.75]
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


def clustered_notes(n, d, seed):
    rng = np.random.default_rng(seed)
    k = max(1, n // 50)
    lab = rng.integers(0, k, n)
    centres = rng.standard_normal((k, d)).astype(np.float32)
    x = centres[lab] + 0.6 * rng.standard_normal((n, d), dtype=np.float32)
    ents = [(lab[i] * 8 + rng.choice(8, rng.integers(0, 7), replace=False)).tolist() for i in range(n)]
    clusters = (np.arange(n) % 7).tolist()   # a seventh of the pairs is same-cluster and dropped in the walk
    return x, ents, clusters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.75)
    a = ap.parse_args()
    from anorag_hip import METRIC_IP, FlatIndex, related_pairs
    from anorag_hip.related_notes import timing
    med = statistics.median
    for n in a.n:
        x, ents, clusters = clustered_notes(n, a.d, n)
        index = FlatIndex(a.d, METRIC_IP, normalize=True, device=0)
        index.add(x)
        timing(True)
        res = related_pairs(index, ents, clusters, threshold=a.threshold, return_stats=True)   # warm-up
        t_walk, t_score, t_select, t_py = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            related_pairs(index, ents, clusters, threshold=a.threshold)
            t_py.append((time.perf_counter() - t0) * 1e3)
            w, s, q = timing(True)
            t_walk.append(w), t_score.append(s), t_select.append(q)
        timing(False)
        base_min = (a.threshold - 0.3) / 0.7          # defaults: w = 0.3, no bonus with same-cluster pairs excluded
        I, _, _ = index.self_join(base_min, sort=False)    # warm-up, sizes the lists
        t_join = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            index.self_join(base_min, cap_hint=len(I) + 1024, sort=False)
            t_join.append((time.perf_counter() - t0) * 1e3)
        index.close()
        st = res["stats"]
        print(json.dumps({"n": n, "d": a.d, "reps": a.reps, "threshold": a.threshold, "walk_ms": round(med(t_walk), 3),
                          "score_ms": round(med(t_score), 3), "select_ms": round(med(t_select), 3),
                          "python_call_ms": round(med(t_py), 3), "self_join_ms": round(med(t_join), 3),
                          "self_join_pairs": int(len(I)), "related_rows": int((res["n_nbr"] > 0).sum()), **st}), flush=True)


if __name__ == "__main__":
    main()
