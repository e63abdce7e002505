#!/usr/bin/env python3
"""Developer tool: time anr_index_khop_rerank and anr_index_cluster_suppress for B = 1 and 64 queries of C = 64, 256 and
1024 candidates of 768 dimensions: the dot kernel, the rerank kernel, the Gram kernel and the suppression kernel by HIP
events (anr_khop_timing), the two Python calls by wall clock, and beside them the wall time of the plain-Python
restatement (tests/khop_ref.py: rerank on given scores, suppression on a numpy-built cosine matrix) on the same inputs.
Warm-up, then the median of --reps calls; one JSON line per (B, C).  No threshold.

  python tools/khop_perf.py [--reps 9] [--host-queries 2]
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
sys.path[:0] = [os.path.join(ROOT, "ano-rag_amd"), ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-queries", type=int, default=2)
    ap.add_argument("--d", type=int, default=768)
    a = ap.parse_args()
    import khop_ref as kr
    from anorag_hip import METRIC_IP, FlatIndex, _lib
    from anorag_hip.khop_rerank import cluster_suppression, rerank_khop
    lib = _lib.load()
    d = a.d
    rng = np.random.default_rng(1)
    med = statistics.median
    w = dict(kr.FUSION_DEFAULTS, **kr.FEATURE_DEFAULTS)
    for B in (1, 64):
        for Cq in (64, 256, 1024):
            n = B * Cq
            centres = rng.standard_normal((max(8, n // 6), d))
            x = (centres[rng.integers(0, len(centres), n)] + rng.choice([0.1, 0.5, 1.0], (n, 1)) * rng.standard_normal((n, d)))
            x = x.astype(np.float32)
            rows = [np.arange(b * Cq, (b + 1) * Cq) for b in range(B)]
            q, f = rng.standard_normal((B, d)).astype(np.float32), rng.standard_normal((B, d)).astype(np.float32)
            bm25 = [rng.uniform(0, 1, Cq) for _ in range(B)]
            is_prf = [rng.random(Cq) < 0.3 for _ in range(B)]
            psim = [rng.uniform(0, 1, Cq) for _ in range(B)]
            cov = [rng.choice([0.0, 0.5, 1.0], Cq) for _ in range(B)]
            cons = [rng.integers(0, 2, Cq) for _ in range(B)]
            hop = [rng.choice([2, 3], Cq) for _ in range(B)]
            index = FlatIndex(d, METRIC_IP, normalize=False, device=0)
            index.add(x)
            ms = (C.c_float * 6)()
            lib.anr_khop_timing(1, None)

            def both():
                out = rerank_khop(index, rows, bm25, is_prf, psim, cov, cons, hop, query_vecs=q, focus_vecs=f)
                t1 = time.perf_counter()
                kept = cluster_suppression(index, [r[o[3]] for r, o in zip(rows, out)], [o[2][o[3]] for o in out])
                return out, kept, t1

            for _ in range(3):
                out, kept, _ = both()
            t = {k: [] for k in ("dot", "rerank", "rerank_call", "gram", "suppress", "suppress_call", "py_rerank", "py_suppress")}
            for _ in range(a.reps):
                t0 = time.perf_counter()
                _, _, t1 = both()
                t2 = time.perf_counter()
                lib.anr_khop_timing(1, ms)
                for k, v in zip(("dot", "rerank", "rerank_call", "gram", "suppress", "suppress_call"), ms):
                    t[k].append(v)
                t["py_rerank"].append((t1 - t0) * 1e3)
                t["py_suppress"].append((t2 - t1) * 1e3)
            lib.anr_khop_timing(0, None)
            index.close()
            # the restatement on the same inputs (the scores given: it has no encoder to run)
            h_rer, h_sup = [], []
            for b in range(min(B, a.host_queries)):
                dn, fc = [float(v) for v in out[b][0]], [float(v) for v in out[b][1]]
                hp = [int(v) for v in hop[b]]
                t0 = time.perf_counter()
                fin, order = kr.rerank(dn, fc, [float(v) for v in bm25[b]], [bool(v) for v in is_prf[b]],
                                       [float(v) for v in psim[b]], [float(v) for v in cov[b]], [int(v) for v in cons[b]], hp,
                                       [kr.decay_factor(0.85, v) for v in hp], w)
                t1 = time.perf_counter()
                sim = kr.cosine_eps_matrix(x[rows[b][order]])
                kr.suppress(lambda i, j: sim[i, j], [fin[c] for c in order], 0.90, 2)
                t2 = time.perf_counter()
                h_rer.append((t1 - t0) * 1e3)
                h_sup.append((t2 - t1) * 1e3)
            print(json.dumps({"B": B, "C": Cq, "d": d, "reps": a.reps, "kept_first_query": int(len(kept[0])),
                              "dot_ms": round(med(t["dot"]), 4), "rerank_ms": round(med(t["rerank"]), 4),
                              "rerank_call_events_ms": round(med(t["rerank_call"]), 4),
                              "gram_ms": round(med(t["gram"]), 4), "suppress_ms": round(med(t["suppress"]), 4),
                              "suppress_call_events_ms": round(med(t["suppress_call"]), 4),
                              "python_rerank_call_ms": round(med(t["py_rerank"]), 4),
                              "python_suppress_call_ms": round(med(t["py_suppress"]), 4),
                              "restatement_rerank_ms_per_query": round(med(h_rer), 3),
                              "restatement_suppress_ms_per_query": round(med(h_sup), 3), "host_queries": len(h_rer),
                              "host_cpus": len(os.sched_getaffinity(0))}), flush=True)


if __name__ == "__main__":
    main()
