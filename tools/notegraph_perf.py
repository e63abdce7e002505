#!/usr/bin/env python3
"""Times the note graph (anorag_hip.NoteGraph) on one GPU: graph upload + CSR build, weighted PageRank, and retrieve for
a batch of seed lists, on a random graph (default 1 M nodes, mean degree 20, 64 queries of 20 seeds, cutoff 2.0, weights
0.35-0.85).  Every timed call ends in a device synchronise inside the library, so the clock is a host clock around the
call (warm run first, median of three); the handle exposes no device-event timing.  --networkx N also times the same
two steps of the reference's path (nx.pagerank, 20 x nx.single_source_dijkstra_path_length) on the host at N nodes: a
yardstick on another size, not a like-for-like ratio.  Prints one JSON line; --out writes it to a file too.

  python tools/notegraph_perf.py --out profiles/notegraph_perf.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ano-rag_amd"))


def random_graph(rng, n, mean_degree):
    E = n * mean_degree // 2
    a, b = rng.integers(0, n, E + E // 8), rng.integers(0, n, E + E // 8)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique((lo * n + hi)[lo != hi])
    key = key[rng.permutation(len(key))[:E]]
    return key // n, key % n, rng.uniform(0.35, 0.85, len(key))


def timed(fn, repeats=3):
    fn()  # warm: code objects, workspace
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--degree", type=int, default=20)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--cutoff", type=float, default=2.0)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--networkx", type=int, default=100_000, help="nodes of the host yardstick (0 = skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from anorag_hip import NoteGraph
    rng = np.random.default_rng(7)
    src, dst, w = random_graph(rng, a.nodes, a.degree)
    res = {"nodes": a.nodes, "edges": int(len(w)), "queries": a.queries, "seeds": a.seeds, "cutoff": a.cutoff, "cap": a.cap,
           "clock": "host clock around calls that end in a device synchronise; warm run, then 3 timed"}
    t0 = time.perf_counter()
    g = NoteGraph(a.nodes, src, dst, w)
    res["create_ms"] = (time.perf_counter() - t0) * 1e3
    med, ts, _ = timed(lambda: g.pagerank())
    it = g.last_iterations
    res.update(pagerank_ms=med, pagerank_runs_ms=ts, pagerank_iterations=it, pagerank_ms_per_iteration=med / it,
               pagerank_model_bytes_per_iteration=int(2 * len(w) * 12 + a.nodes * 16),
               pagerank_model_gbps=(2 * len(w) * 12 + a.nodes * 16) * it / (med * 1e-3) / 1e9)
    lists = [rng.integers(0, a.nodes, a.seeds).tolist() for _ in range(a.queries)]
    med, ts, out = timed(lambda: g.retrieve_raw(lists, a.cutoff, a.cap))
    res.update(retrieve_ms=med, retrieve_runs_ms=ts, retrieve_found_mean=float(out[4].mean()),
               retrieve_ms_per_query=med / a.queries)
    one = [lists[0]]
    med, ts, _ = timed(lambda: g.retrieve_raw(one, a.cutoff, a.cap))
    res.update(retrieve_one_query_ms=med, retrieve_one_query_runs_ms=ts)
    g.close()
    if a.networkx:
        import networkx as nx
        s2, d2, w2 = random_graph(rng, a.networkx, a.degree)
        G = nx.Graph()
        G.add_nodes_from(range(a.networkx))
        G.add_weighted_edges_from(zip(s2.tolist(), d2.tolist(), w2.tolist()))
        t0 = time.perf_counter()
        nx.pagerank(G, weight="weight")
        res["networkx_nodes"] = a.networkx
        res["networkx_pagerank_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for s in rng.integers(0, a.networkx, a.seeds).tolist():
            nx.single_source_dijkstra_path_length(G, s, cutoff=a.cutoff, weight="weight")
        res["networkx_one_query_dijkstras_ms"] = (time.perf_counter() - t0) * 1e3
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
