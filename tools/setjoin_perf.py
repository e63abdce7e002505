#!/usr/bin/env python3
"""Developer tool: time the set-overlap join (anr_setjoin_*, anorag_hip.note_relations.SetJoin) at N notes whose entities
follow a Zipf law: wall clock of building the handle (upload + postings), of cooccur (count launch, scans, fill launch,
fetch; warm-up, then the median of --reps) and of pair_counts over the pairs cooccur returned, with the stats of DESIGN.md
§5k.  One JSON line per N.  --reference also times the reference's own loop shape (a Python restatement of
relation_extractor.py:418-481 on integer ids) on the same input and host, for N up to --reference-max.  Nothing here is
asserted anywhere.

  python tools/setjoin_perf.py [--n 100000 1000000] [--items-per-note 6] [--vocab 0] [--zipf 1.1] [--shift 50]
                               [--min-common 2] [--reps 3] [--reference]

An entity present in L notes costs L^2 / 2 table insertions (and the reference as many set operations), so the head of the
law decides the time: --shift s draws entity k with probability ~ (k + s)^-zipf; --vocab 0 means N / 4 entities.
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


def zipf_notes(n, per_note, vocab, a, shift, seed):
    rng = np.random.default_rng(seed)
    p = (np.arange(vocab) + 1.0 + shift) ** -a
    p /= p.sum()
    sizes = rng.integers(0, 2 * per_note + 1, size=n)
    draws = rng.choice(vocab, size=int(sizes.sum()), p=p)
    ends = np.cumsum(sizes)
    return [draws[e - k:e].tolist() for k, e in zip(sizes.tolist(), ends.tolist())]


def reference_loop(rows, min_common):
    """the reference's method on integer ids: posting sets, a union per note, one set intersection per candidate pair"""
    from collections import defaultdict
    posting = defaultdict(set)
    sets = []
    for i, row in enumerate(rows):
        sets.append(set(row))
        for e in row:
            posting[e].add(i)
    done, out = set(), 0
    for i, mine in enumerate(sets):
        if not mine:
            continue
        related = set()
        for e in mine:
            related.update(posting[e])
        related.discard(i)
        for j in related:
            pair = (i, j) if i < j else (j, i)
            if pair in done:
                continue
            done.add(pair)
            if len(mine & sets[j]) >= min_common:
                out += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--items-per-note", type=int, default=6)
    ap.add_argument("--vocab", type=int, default=0)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--shift", type=float, default=50.0)
    ap.add_argument("--min-common", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--reference-max", type=int, default=100000)
    a = ap.parse_args()
    from anorag_hip.note_relations import SetJoin

    for n in a.n:
        vocab = a.vocab or max(n // 4, 16)
        rows = zipf_notes(n, a.items_per_note, vocab, a.zipf, a.shift, n)
        t0 = time.perf_counter()
        sj = SetJoin(rows)
        t_create = time.perf_counter() - t0
        try:
            times, out = [], None
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                out = sj.cooccur(a.min_common, return_stats=True)
                if rep:
                    times.append(time.perf_counter() - t0)
            I, J, stats = out[0], out[1], out[6]
            t0 = time.perf_counter()
            sj.pair_counts(I, J)
            t_pairs = time.perf_counter() - t0
            line = {"n": n, "vocab": vocab, "nnz": int(len(sj.ids)), "min_common": a.min_common,
                    "longest_posting": int(np.bincount(sj.ids).max()) if len(sj.ids) else 0,
                    "create_ms": round(t_create * 1e3, 3), "cooccur_ms": round(statistics.median(times) * 1e3, 3),
                    "pair_counts_ms": round(t_pairs * 1e3, 3), **stats}
            if a.reference and n <= a.reference_max:
                t0 = time.perf_counter()
                kept = reference_loop(rows, a.min_common)
                line["reference_loop_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                line["reference_pairs"] = kept
            print(json.dumps(line), flush=True)
        finally:
            sj.close()


if __name__ == "__main__":
    main()
