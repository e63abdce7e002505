#!/usr/bin/env python3
"""Developer tool: time anr_index_cluster_quality at N x 768 rows under a DBSCAN-like labelling (a few hundred clusters of
uneven size plus noise): the silhouette group (sort, norms, the N x N walk, the mean) and the cohesion group (two passes
over the clusters' own tiles) by HIP events (anr_cluster_quality_timing), the whole call by events and by wall clock,
with the share of the f64 matrix peak the multiplied tiles amount to.  Warm-up, then the median of --reps calls; one JSON
line per N.  --host N ... also times sklearn's silhouette_score plus scipy's pdist per cluster on the same rows with the
CPUs the process may use (at most 16 threads), once.

  python tools/cluster_quality_perf.py [--n 20000 100000] [--d 768] [--reps 5] [--host 20000]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ano-rag_amd"), ROOT]

F64_MATRIX_PEAK_TFLOPS = 78.6   # MI355X, f64 matrix


def labelled_rows(n, d, seed):
    """rows around ~300 centres with sizes drawn unevenly, a tenth of the rows noise (-1) scattered wide"""
    rng = np.random.default_rng(seed)
    k = 300
    weights = rng.pareto(1.5, k) + 0.05
    labels = rng.choice(k, n, p=weights / weights.sum())
    noise = rng.random(n) < 0.1
    centres = rng.standard_normal((k, d)).astype(np.float32)
    x = centres[labels] + 0.25 * rng.standard_normal((n, d), dtype=np.float32)
    x[noise] = 1.5 * rng.standard_normal((int(noise.sum()), d), dtype=np.float32)
    labels[noise] = -1
    return x, labels.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host", type=int, nargs="*", default=[])
    a = ap.parse_args()
    from anorag_hip import METRIC_L2, FlatIndex, _lib
    from anorag_hip.topic_clustering import cluster_quality
    lib = _lib.load()
    med = statistics.median
    for n in a.n:
        x, labels = labelled_rows(n, a.d, n)
        index = FlatIndex(a.d, METRIC_L2, normalize=False, device=0)
        index.add(x)
        ms = (C.c_float * 3)()
        lib.anr_cluster_quality_timing(1, None)
        for _ in range(2):
            q = cluster_quality(index, labels, return_stats=True)
        t_sil, t_coh, t_call, t_py = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            cluster_quality(index, labels)
            t_py.append((time.perf_counter() - t0) * 1e3)
            lib.anr_cluster_quality_timing(1, ms)
            t_sil.append(ms[0]); t_coh.append(ms[1]); t_call.append(ms[2])
        lib.anr_cluster_quality_timing(0, None)
        index.close()
        st = q["stats"]
        tile_flop = 64 * 64 * 2 * (-(-a.d // 64) * 64)
        sil_flop = (st["silhouette_tiles"] + -(-n // 64)) * tile_flop
        coh_flop = 2 * st["cohesion_tiles"] * tile_flop
        rec = {"n": n, "d": a.d, "reps": a.reps, "n_labels": st["n_labels"], "n_noise": st["n_noise"],
               "largest_cluster": int(q["sizes"][1:].max()), "silhouette_mean": q["mean"],
               "silhouette_group_ms": round(med(t_sil), 3), "cohesion_group_ms": round(med(t_coh), 3),
               "call_events_ms": round(med(t_call), 3), "python_call_ms": round(med(t_py), 3),
               "silhouette_tflops_done": round(sil_flop / med(t_sil) / 1e9, 2),
               "silhouette_fraction_of_f64_matrix_peak": round(sil_flop / med(t_sil) / 1e9 / F64_MATRIX_PEAK_TFLOPS, 4),
               "silhouette_useful_fraction_of_peak": round(2.0 * n * n * a.d / med(t_sil) / 1e9 / F64_MATRIX_PEAK_TFLOPS, 4),
               "cohesion_tflops_done": round(coh_flop / max(med(t_coh), 1e-6) / 1e9, 2),
               "cohesion_fraction_of_f64_matrix_peak": round(coh_flop / max(med(t_coh), 1e-6) / 1e9 / F64_MATRIX_PEAK_TFLOPS, 4),
               "scratch_bytes": st["scratch_bytes"]}
        print(json.dumps(rec), flush=True)
        if n in a.host:
            from scipy.spatial.distance import pdist
            from sklearn.metrics import silhouette_score
            from threadpoolctl import threadpool_limits
            cpus = min(16, len(os.sched_getaffinity(0)))
            with threadpool_limits(limits=cpus):
                t0 = time.perf_counter()
                host_sil = float(silhouette_score(x, labels))
                t_s = time.perf_counter() - t0
                t0 = time.perf_counter()
                for lab in np.unique(labels):
                    rows = x[labels == lab]
                    if lab >= 0 and len(rows) > 1:
                        dist = pdist(rows, metric="cosine")
                        float(np.mean(dist)), float(np.std(dist))
                t_c = time.perf_counter() - t0
            print(json.dumps({"n": n, "d": a.d, "host_threads": cpus, "sklearn_silhouette_s": round(t_s, 2),
                              "scipy_cohesion_s": round(t_c, 2), "host_silhouette": host_sil,
                              "device_minus_host_silhouette": q["mean"] - host_sil}), flush=True)


if __name__ == "__main__":
    main()
