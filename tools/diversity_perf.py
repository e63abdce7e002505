#!/usr/bin/env python3
"""Developer tool: time anr_index_diversify at the workload's shape (C = 200 candidates of 768 dimensions per query,
50 selected) for B = 1 and 64 queries: the similarity kernels (with their fraction of the f64 matrix peak), the decision
kernel and the whole call by HIP events (anr_diversify_timing), the Python call by wall clock, and beside them the
drop-in's host path (its host loop on a host-built matrix) on the same inputs.  Warm-up, then the median of --reps
calls; one JSON line per B.

  python tools/diversity_perf.py [--reps 9] [--host-queries 4]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-queries", type=int, default=4)
    ap.add_argument("--c", type=int, default=200)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=50)
    a = ap.parse_args()
    from anorag_hip import METRIC_IP, FlatIndex, _lib
    from anorag_hip.diversity import diversify
    from retrieval import diversity_scheduler as ds
    lib = _lib.load()
    Cq, d, K = a.c, a.d, a.k
    rng = np.random.default_rng(1)
    for B in (1, 64):
        common = rng.standard_normal(d)
        centres = rng.standard_normal((40, d))
        x = (common + centres[rng.integers(0, 40, B * Cq)] + 0.9 * rng.standard_normal((B * Cq, d))).astype(np.float32)
        scores = [np.round(rng.uniform(0.0, 0.98, Cq), 6) for _ in range(B)]
        masks = [rng.choice([1, 2, 5, 8, 9, 16, 32], Cq).astype(np.uint32) for _ in range(B)]
        rows = [np.arange(b * Cq, (b + 1) * Cq) for b in range(B)]
        index = FlatIndex(d, METRIC_IP, normalize=False, device=0)
        index.add(x)
        kw = dict(max_candidates=K, similarity_threshold=0.85, quota=True, quotas=[15, 10, 8, 12, 6, 0], balance_factor=0.8)
        ms = (C.c_float * 3)()
        lib.anr_diversify_timing(1, None)
        for _ in range(3):
            out = diversify(index, rows, scores, masks, **kw)
        t_a, t_b, t_call, t_py = [], [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            diversify(index, rows, scores, masks, **kw)
            t_py.append((time.perf_counter() - t0) * 1e3)
            lib.anr_diversify_timing(1, ms)
            t_a.append(ms[0]); t_b.append(ms[1]); t_call.append(ms[2])
        lib.anr_diversify_timing(0, None)
        index.close()
        med = statistics.median
        nb = -(-Cq // 32)
        flops_done = B * (nb * (nb + 1) // 2) * 32 * 32 * 2 * (-(-d // 64) * 64)   # what the upper tiles multiply
        flops_useful = B * Cq * Cq * d                                             # the upper triangle's 2 * C^2 / 2 * d
        # the drop-in's host path on the same inputs: host-built matrix and the host loop
        t_host = []
        for b in range(min(B, a.host_queries)):
            cands = [{"id": f"n{j}", "content": f"w{j}", "score": float(scores[b][j]), "embedding": x[rows[b][j]].tolist(),
                      "source_types": ["vector"] if masks[b][j] & 1 else []} for j in range(Cq)]
            items = ds.DiversityScheduler({})._convert_to_candidate_items(cands)
            t0 = time.perf_counter()
            sim = ds._semantic_matrix(items)
            ds._host_decide(sim, [float(s) for s in scores[b]], masks[b], max_candidates=K, similarity_threshold=0.85,
                            dedup=True, quota=True, quotas=[15, 10, 8, 12, 6, 0] + [0] * 26, balance_factor=0.8)
            t_host.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"B": B, "C": Cq, "d": d, "K": K, "reps": a.reps, "selected": int(len(out[0][1])),
                          "similarity_ms": round(med(t_a), 4), "decision_ms": round(med(t_b), 4),
                          "call_events_ms": round(med(t_call), 4), "python_call_ms": round(med(t_py), 4),
                          "similarity_tflops_done": round(flops_done / med(t_a) / 1e9, 3),
                          "fraction_of_f64_matrix_peak": round(flops_done / med(t_a) / 1e9 / F64_MATRIX_PEAK_TFLOPS, 4),
                          "useful_fraction_of_peak": round(flops_useful / med(t_a) / 1e9 / F64_MATRIX_PEAK_TFLOPS, 4),
                          "host_path_ms_per_query": round(med(t_host), 3), "host_queries": len(t_host),
                          "host_cpus": len(os.sched_getaffinity(0))}), flush=True)


if __name__ == "__main__":
    main()
