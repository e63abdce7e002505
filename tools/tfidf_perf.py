#!/usr/bin/env python3
"""Developer tool: time the TF-IDF duplicate join (anr_tfidf_*, anorag_hip.note_dedup.TfidfJoin) on two seeded synthetic
corpora of Zipf-distributed words through ``TfidfVectorizer(stop_words='english', max_features=1000)``, the reference's
own call: 5 000 notes of which a fifth are near-duplicates of another note, and 100 000 notes.  Per corpus one JSON line:
host milliseconds of the vectoriser and of building the handle (normalise, relabel, upload, postings), device milliseconds
of the join split into its nominating and deciding stages (HIP events, the median of --reps after a warm-up), wall clock of
the whole ``duplicates`` call, pairs nominated and kept, rows overflowed, and the walk's cost sum(L^2 / 2) over the terms'
posting lengths.  --reference adds the reference's own host expression on the same matrix and host — sklearn's
``cosine_similarity`` and the i < j loop of utils/note_validator.py:379-386 — for corpora of at most --reference-max notes
(the dense matrix takes 8 N^2 bytes: 0.2 GB at 5 000, 3.2 GB at 20 000, 80 GB at 100 000).  Nothing here is asserted anywhere.

  python tools/tfidf_perf.py [--n 5000 100000] [--dup-fraction 0.2 0] [--words 30] [--vocab 20000] [--zipf 1.1]
                             [--shift 20] [--threshold 0.85] [--reps 3] [--reference] [--reference-max 5000]
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


def corpus(n, words, vocab, a, shift, dup_fraction, seed):
    """n texts of about ``words`` words drawn with probability ~ (rank + shift)^-a; a ``dup_fraction`` of them are copies of
    an earlier text with up to three words replaced"""
    rng = np.random.default_rng(seed)
    p = (np.arange(vocab) + 1.0 + shift) ** -a
    p /= p.sum()
    sizes = rng.integers(words // 2, words + words // 2 + 1, size=n)
    draws = rng.choice(vocab, size=int(sizes.sum()), p=p)
    ends = np.cumsum(sizes)
    rows = [draws[e - k:e] for k, e in zip(sizes.tolist(), ends.tolist())]
    for k in np.flatnonzero(rng.random(n) < dup_fraction):
        if k == 0:
            continue
        row = rows[int(rng.integers(0, k))].copy()
        for _ in range(int(rng.integers(0, 4))):
            row[int(rng.integers(len(row)))] = rng.choice(vocab, p=p)
        rows[k] = row
    return [" ".join(f"w{t}" for t in row.tolist()) for row in rows]


def reference_pairs(matrix, threshold):
    from sklearn.metrics.pairwise import cosine_similarity
    t0 = time.perf_counter()
    similarity_matrix = cosine_similarity(matrix)
    t1 = time.perf_counter()
    kept = 0
    n = matrix.shape[0]
    for i in range(n):
        for j in range(i + 1, n):
            if similarity_matrix[i][j] >= threshold:
                kept += 1
    return kept, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[5000, 100000])
    ap.add_argument("--dup-fraction", type=float, nargs="+", default=[0.2, 0.0])
    ap.add_argument("--words", type=int, default=30)
    ap.add_argument("--vocab", type=int, default=20000)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--shift", type=float, default=20.0)
    ap.add_argument("--threshold", type=float, default=0.85)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--reference-max", type=int, default=5000)
    a = ap.parse_args()
    from sklearn.feature_extraction.text import TfidfVectorizer
    from anorag_hip.note_dedup import TfidfJoin

    for k, n in enumerate(a.n):
        dup = a.dup_fraction[min(k, len(a.dup_fraction) - 1)]
        texts = corpus(n, a.words, a.vocab, a.zipf, a.shift, dup, n)
        t0 = time.perf_counter()
        matrix = TfidfVectorizer(stop_words='english', max_features=1000).fit_transform(texts)
        t_vec = time.perf_counter() - t0
        posting = np.bincount(matrix.indices, minlength=matrix.shape[1]).astype(np.float64)
        t0 = time.perf_counter()
        join = TfidfJoin(matrix)
        t_create = time.perf_counter() - t0
        try:
            nominate, decide, wall, stats = [], [], [], None
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                I, J, sim, stats = join.duplicates(a.threshold, return_stats=True)
                if rep or a.reps == 0:
                    wall.append(time.perf_counter() - t0)
                    nominate.append(stats["nominate_us"] / 1e3)
                    decide.append(stats["decide_us"] / 1e3)
            line = {"n": n, "dup_fraction": dup, "terms": int(matrix.shape[1]), "nnz": int(matrix.nnz),
                    "longest_posting": int(posting.max()) if len(posting) else 0,
                    "walk_cost_sum_L2_half": float(np.sum(posting * posting) / 2), "threshold": a.threshold,
                    "vectorise_ms": round(t_vec * 1e3, 1), "create_ms": round(t_create * 1e3, 1),
                    "nominate_ms": round(statistics.median(nominate), 3), "decide_ms": round(statistics.median(decide), 3),
                    "duplicates_wall_ms": round(statistics.median(wall) * 1e3, 3),
                    **{key: stats[key] for key in ("rows", "insertions", "pairs_nominated", "pairs_kept", "rows_overflowed",
                                                   "table_slots")}}
            if a.reference:
                if n <= a.reference_max:
                    kept, t_cos, t_loop = reference_pairs(matrix, a.threshold)
                    line.update(reference_cosine_similarity_ms=round(t_cos, 1), reference_loop_ms=round(t_loop, 1),
                                reference_pairs=kept)
                else:
                    line["reference"] = f"not run: the dense matrix would take {8 * n * n / 1e9:.1f} GB"
            print(json.dumps(line), flush=True)
        finally:
            join.close()


if __name__ == "__main__":
    main()
