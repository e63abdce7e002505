#!/usr/bin/env python3
"""Times the device graph quality metrics (anorag_hip.NoteGraph.components / hop_histogram / quality_metrics) on one GPU,
on a random graph of --nodes nodes with mean degree --degree (default 100 000 and 16).  Prints the passes, the levels,
the time per call by HIP events (the span of the call's work on the handle's stream; the host reads one count per level
inside it) and by the host clock, and the achieved bytes/s against the model of DESIGN.md §5i: per pass and level
2E * W * 8 bytes of neighbour words gathered plus 3 * n * W * 8 of state.  Warm run first, then the median of three.
--networkx N also times the reference's compute_metrics expression (nx.connected_components and
nx.average_shortest_path_length of the largest component) on the host at N nodes and mean degree 2.2, the shape of
the reference's sparse note graphs: a yardstick on another size, not a like-for-like ratio.  Prints one JSON line;
--out writes it to a file too.

  python tools/graph_quality_perf.py --out profiles/graph_quality_perf.json
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
    E = int(n * mean_degree / 2)
    a, b = rng.integers(0, n, E + E // 8 + 8), rng.integers(0, n, E + E // 8 + 8)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique((lo * n + hi)[lo != hi])
    key = key[rng.permutation(len(key))[:E]]
    return key // n, key % n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--degree", type=float, default=16)
    ap.add_argument("--words", type=int, default=0, help="words per node and pass (0 = the library's default)")
    ap.add_argument("--networkx", type=int, default=0, help="nodes of the host yardstick (0 = skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from anorag_hip import NoteGraph
    rng = np.random.default_rng(11)
    src, dst = random_graph(rng, a.nodes, a.degree)
    E = len(src)
    g = NoteGraph(a.nodes, src, dst, np.ones(E))
    g.set_bfs_words(a.words)
    res = {"nodes": a.nodes, "edges": E}

    def run(fn):
        fn()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), out

    ms, (labels, sizes) = run(g.components)
    res.update(components_host_ms=ms, components=len(sizes), largest=max(sizes))
    roots = np.flatnonzero(labels == np.arange(a.nodes))
    nodes = np.flatnonzero(labels == roots[sizes.index(max(sizes))])
    ev = []

    def hist():
        out = g.hop_histogram(nodes)
        ev.append(g.last_bfs_stats["event_us"] / 1e3)
        return out
    ms, counts = run(hist)
    st = g.last_bfs_stats
    W = st["words"]
    model = st["levels"] * (2 * E * W * 8 + 3 * a.nodes * W * 8)
    ev_ms = statistics.median(ev[1:])
    res.update(words=W, sources_per_pass=st["sources_per_pass"], passes=st["passes"], levels_walked=st["levels"],
               hop_levels=len(counts), scratch_bytes=st["scratch_bytes"], hop_histogram_event_ms=ev_ms,
               hop_histogram_host_ms=ms, model_bytes=model, model_gbps_by_events=model / (ev_ms * 1e-3) / 1e9,
               us_per_level_by_events=ev_ms * 1e3 / st["levels"])
    ms, m = run(g.quality_metrics)
    res.update(quality_metrics_host_ms=ms, average_shortest_path_length=m["average_shortest_path_length"])
    g.close()
    if a.networkx:
        import networkx as nx
        s2, d2 = random_graph(rng, a.networkx, 2.2)
        G = nx.Graph()
        G.add_nodes_from(range(a.networkx))
        G.add_edges_from(zip(s2.tolist(), d2.tolist()))
        t0 = time.perf_counter()
        comp = max(nx.connected_components(G), key=len)
        aspl = nx.average_shortest_path_length(G.subgraph(comp))
        res.update(networkx_nodes=a.networkx, networkx_edges=len(s2), networkx_largest=len(comp),
                   networkx_host_s=time.perf_counter() - t0)
        g2 = NoteGraph(a.networkx, s2, d2, np.ones(len(s2)))
        ms, m2 = run(g2.quality_metrics)
        g2.close()
        assert m2["average_shortest_path_length"] == aspl
        res.update(same_graph_device_host_ms=ms)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
