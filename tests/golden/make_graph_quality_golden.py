#!/usr/bin/env python3
"""Generate the graph-quality golden vectors from the REFERENCE itself (run in the build container only).

  python tests/golden/make_graph_quality_golden.py /path/to/reference

Imports, by file path, the reference's graph/graph_quality.py (networkx is what it runs on) and runs compute_metrics on
the graphs below.  Writes tests/golden/graph_quality_cases.npz — data only:

  names                              JSON list of the cases
  <case>_n, _src, _dst, _loops       node count, the undirected edges without self-loops as node indices (a node's index
                                     is its position in the nx.Graph), and the number of self-loops
  <case>_floats                      average_degree, num_components, largest_component_size,
                                     average_shortest_path_length, as compute_metrics returned them (float64)
  <case>_sizes                       component_sizes, in its order
  <case>_hist                        hist[l] = the (source, node) pairs at hop distance l inside the largest component,
                                     from nx.single_source_shortest_path_length
  named_case                         JSON: node names and edges (by name, self-loops included) of the `named` case
  empty_keys                         JSON: the keys compute_metrics returns for a graph with no nodes

Each case ASSERTS the property it is there for, so that a test cannot pass by accident.
"""
import importlib.util
import json
import os
import random
import sys

import networkx as nx
import numpy as np

if len(sys.argv) != 2:
    sys.exit("usage: make_graph_quality_golden.py /path/to/reference")
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))

spec = importlib.util.spec_from_file_location("ref_graph_quality", os.path.join(REF, "graph", "graph_quality.py"))
gq = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gq)

KEYS = ["average_degree", "num_components", "largest_component_size", "average_shortest_path_length"]


def int_graph(n, pairs):
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(pairs)
    assert list(G) == list(range(n))
    return G


def record(out, name, G):
    order = list(G)
    index = {v: i for i, v in enumerate(order)}
    m = gq.compute_metrics(G)
    assert list(m.keys()) == KEYS + ["component_sizes"]
    assert all(type(m[k]) is float for k in KEYS) and all(type(s) is int for s in m["component_sizes"])
    edges = [(index[u], index[v]) for u, v in G.edges() if u != v]
    loops = sum(1 for u, v in G.edges() if u == v)
    largest = max(nx.connected_components(G), key=len)
    assert len(largest) <= 2600
    sub = G.subgraph(largest)
    hist = {}
    for s in sub:
        for d in nx.single_source_shortest_path_length(sub, s).values():
            hist[d] = hist.get(d, 0) + 1
    hist = np.array([hist[d] for d in range(len(hist))], dtype=np.int64)
    nc = len(largest)
    if nc > 1:  # the histogram is the sum the reference divides
        assert sum(d * int(c) for d, c in enumerate(hist)) / (nc * (nc - 1)) == m["average_shortest_path_length"]
    out[f"{name}_n"] = np.int64(len(order))
    arr = np.array(edges, dtype=np.int64).reshape(-1, 2)
    out[f"{name}_src"], out[f"{name}_dst"] = arr[:, 0].copy(), arr[:, 1].copy()
    out[f"{name}_loops"] = np.int64(loops)
    out[f"{name}_floats"] = np.array([m[k] for k in KEYS], dtype=np.float64)
    out[f"{name}_sizes"] = np.array(m["component_sizes"], dtype=np.int64)
    out[f"{name}_hist"] = hist
    first = min(index[v] for v in largest)
    print(f"{name}: n={len(order)} edges={len(edges)} loops={loops} components={len(m['component_sizes'])} "
          f"largest={nc} (first node {first}) levels={len(hist)} aspl={m['average_shortest_path_length']!r}")
    return m, first


def random_pairs(rng, n, count, lo=0):
    pairs = set()
    while len(pairs) < count:
        a, b = rng.randrange(lo, n), rng.randrange(lo, n)
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    return sorted(pairs)


def main():
    out, names = {}, []
    rng = random.Random(20261017)

    def add(name, G):
        names.append(name)
        return record(out, name, G)

    m, _ = add("one_node", int_graph(1, []))
    assert m["average_shortest_path_length"] == 0.0 and m["component_sizes"] == [1]
    m, _ = add("two_nodes", int_graph(2, [(0, 1)]))
    assert m["average_shortest_path_length"] == 1.0
    m, _ = add("isolated", int_graph(37, []))
    assert m["num_components"] == 37.0 and m["average_shortest_path_length"] == 0.0 and m["average_degree"] == 0.0

    perm = list(range(130))
    rng.shuffle(perm)
    m, _ = add("path130", int_graph(130, [(perm[i], perm[i + 1]) for i in range(129)]))
    assert len(out["path130_hist"]) == 130 and m["num_components"] == 1.0  # 129 levels; sources fill 2 words + 2 bits

    m, _ = add("star1000", int_graph(1000, [(417, v) for v in range(1000) if v != 417]))
    assert m["num_components"] == 1.0 and len(out["star1000_hist"]) == 3

    # two largest components of equal size: a small one with node 0 in front, the two of 40 interleaved over [6, 86) —
    # the even nodes first in node order (node 6) — and a small one behind them
    a_nodes, b_nodes = list(range(6, 86, 2)), list(range(7, 86, 2))
    pairs = [(i, i + 1) for i in range(5)]
    for nodes, step in ((a_nodes, 5), (b_nodes, 3)):  # a spanning path and chords: more of them in the second
        sh = nodes[:]
        rng.shuffle(sh)
        pairs += [(sh[i], sh[i + 1]) for i in range(len(sh) - 1)]
        pairs += [(sh[i], sh[(i * 7 + 3) % len(sh)]) for i in range(0, len(sh), step) if i != (i * 7 + 3) % len(sh)]
    pairs += [(86, 87), (87, 88)]
    pairs = sorted({(min(a, b), max(a, b)) for a, b in pairs})
    m, first = add("equal_largest", int_graph(89, pairs))
    assert m["component_sizes"] == [6, 40, 40, 3] and first == 6
    Gb = int_graph(89, pairs).subgraph(b_nodes)
    assert nx.average_shortest_path_length(Gb) != m["average_shortest_path_length"], "the two candidates must differ"

    # the largest component's smallest node is not 0: isolated nodes and pairs in front of and behind it
    n = 700
    big = list(range(150, 550))
    rng.shuffle(big)
    big = big[:300]
    pairs = [(big[i], big[rng.randrange(0, i)]) for i in range(1, len(big))]   # a random tree over 300 nodes
    pairs += [(big[rng.randrange(300)], big[rng.randrange(300)]) for _ in range(60)]
    rest = [v for v in range(n) if v not in set(big)]
    pairs += [(rest[i], rest[i + 1]) for i in range(0, len(rest) - 1, 3)]      # pairs; every third node isolated
    pairs = sorted({(min(a, b), max(a, b)) for a, b in pairs if a != b})
    m, first = add("root_not_zero", int_graph(n, pairs))
    assert first == min(big) and first > 0 and m["largest_component_size"] == 300.0 and m["num_components"] > 100
    assert 1 in m["component_sizes"] and 2 in m["component_sizes"]

    m, _ = add("random300", int_graph(300, random_pairs(rng, 300, 270)))
    assert 20 <= m["num_components"] <= 120
    m, _ = add("random3000", int_graph(3000, random_pairs(rng, 3000, 3300)))
    assert 200 <= m["num_components"] <= 700 and m["largest_component_size"] > 2000

    # the drop-in's input: string names, self-loops, nodes added by add_edge after the add_node ones
    G = nx.Graph()
    node_names = [f"note-{i:03d}" for i in range(60)]
    for v in node_names[:50]:
        G.add_node(v)
    for a, b in random_pairs(rng, 60, 55):
        G.add_edge(node_names[a], node_names[b])
    for i in (3, 17, 58):
        G.add_edge(node_names[i], node_names[i])
    G.add_node("lonely")
    G.add_edge("lonely", "lonely")
    m, _ = add("named", G)
    assert out["named_loops"] == 4 and m["num_components"] > 3
    assert m["average_degree"] == (2 * len(out["named_src"]) + 8) / 61.0
    out["named_case"] = np.array(json.dumps({"nodes": list(G), "edges": [[u, v] for u, v in G.edges()]}))

    out["empty_keys"] = np.array(json.dumps(gq.compute_metrics(nx.Graph())))
    out["names"] = np.array(json.dumps(names))
    path = os.path.join(HERE, "graph_quality_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
