#!/usr/bin/env python3
"""Generate the note-graph golden vectors from the REFERENCE itself (run in the build container only).

  python tests/golden/make_notegraph_golden.py /path/to/reference

Imports, by file path, the reference's graph/graph_index.py and graph/graph_retriever.py (networkx + scipy are what they
run on; `loguru`, `utils` and `config` are satisfied by stand-in modules, as in make_golden.py) and runs
GraphIndex.build_index (nx.pagerank, graph_index.py:43-49) and GraphRetriever.retrieve (graph_retriever.py:61-92) on
small random note graphs built the way GraphBuilder.build_graph builds them (add_node per note, add_edge per relation).
Writes tests/golden/notegraph_cases.npz — data only:

  <case>_n, _src, _dst, _w          the graph: node count and the undirected edges, as node indices
  <case>_importance                  importance_score per node (1.0 where the note carries none)
  <case>_centrality, _iters          nx.pagerank's values in node order, and the power iterations it made
  <case>_khop                        the retriever's k_hop (a distance cutoff)
  <case>_seed_offs, _seeds           the seed lists (-1 = a note id that is not in the graph)
  <case>_res_offs, _res_ids, _res_dist, _res_score    retrieve()'s output per seed list, in its order
  <case>_tie_offs, _tie_groups       runs of equal graph_score inside a result (start, end), if any
  relations_case                     JSON: notes + relations with a repeated pair, and the nx.Graph's node order / weights

Two properties are ASSERTED so that the tests cannot hide an ordering bug: inside a result no two entries share a
graph_score (otherwise the run is recorded as a tie group, at most 1 % of the entries), and at the stopping iteration the
L1 change is further than a relative 1e-6 from n * tol (an iteration count off by one is then a bug, not rounding).
"""
import importlib.util
import json
import os
import random
import sys
import types

import networkx as nx
import numpy as np

if len(sys.argv) != 2:
    sys.exit("usage: make_notegraph_golden.py /path/to/reference")
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))


def stub_modules():
    lg = types.ModuleType("loguru")

    class _L:
        def __getattr__(self, _):
            return lambda *a, **k: None

    lg.logger = _L()
    sys.modules["loguru"] = lg
    ut = types.ModuleType("utils")
    ut.FileUtils = type("FileUtils", (), {})
    sys.modules["utils"] = ut
    cf = types.ModuleType("config")

    class _C:
        def get(self, key, default=None):
            return default

    cf.config = _C()
    sys.modules["config"] = cf
    pkg = types.ModuleType("graph")
    pkg.__path__ = [os.path.join(REF, "graph")]
    sys.modules["graph"] = pkg


def load(name):
    spec = importlib.util.spec_from_file_location(f"graph.{name}", os.path.join(REF, "graph", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[f"graph.{name}"] = mod
    spec.loader.exec_module(mod)
    return mod


def pagerank_iterations(G, alpha=0.85, max_iter=100, tol=1.0e-6):
    """networkx's _pagerank_scipy step for step (uniform personalisation), to learn what nx.pagerank does not return:
    the iteration it stopped at and the L1 change there"""
    import scipy as sp
    N = len(G)
    nodelist = list(G)
    A = nx.to_scipy_sparse_array(G, nodelist=nodelist, weight="weight", dtype=float)
    S = A.sum(axis=1)
    S[S != 0] = 1.0 / S[S != 0]
    Q = sp.sparse.csr_array(sp.sparse.spdiags(S.T, 0, *A.shape))
    A = Q @ A
    x = np.repeat(1.0 / N, N)
    p = np.repeat(1.0 / N, N)
    is_dangling = np.where(S == 0)[0]
    for it in range(max_iter):
        xlast = x
        x = alpha * (x @ A + sum(x[is_dangling]) * p) + (1 - alpha) * p
        err = np.absolute(x - xlast).sum()
        if err < N * tol:
            return x, it + 1, err
    raise RuntimeError("no convergence")


def make_graph(rng, n, mean_degree, n_isolated, island, importance_share):
    """notes n00000.. in order; the last `island` nodes before the isolated ones form a component of their own"""
    ids = [f"n{i:05d}" for i in range(n)]
    G = nx.Graph()
    imp = np.ones(n)
    for i, nid in enumerate(ids):
        note = {"note_id": nid, "paragraph_idxs": [i % 7]}
        if rng.random() < importance_share:
            imp[i] = round(rng.uniform(0.2, 3.0), 3)
            note["importance_score"] = float(imp[i])
        G.add_node(nid, **note)
    main = n - n_isolated - island
    pairs = set()

    def add(lo, hi, count):
        while count > 0:
            a, b = rng.randrange(lo, hi), rng.randrange(lo, hi)
            if a == b or (min(a, b), max(a, b)) in pairs:
                continue
            pairs.add((min(a, b), max(a, b)))
            G.add_edge(ids[a], ids[b], weight=rng.uniform(0.35, 0.85), relation_type="semantic_similarity")
            count -= 1

    add(0, main, main * mean_degree // 2)
    if island:
        add(main, main + island, island * 2)
    return G, ids, imp


def record(out, name, G, ids, imp, k_hop, seed_lists, gi_mod, gr_mod):
    index = {nid: i for i, nid in enumerate(G)}
    assert list(G) == ids
    n = len(ids)
    gi = gi_mod.GraphIndex()
    gi.build_index(G)
    cent = np.array([gi.node_centrality[nid] for nid in ids], dtype=np.float64)
    x, iters, err = pagerank_iterations(G)
    assert np.array_equal(x, cent), "the step-for-step PageRank differs from nx.pagerank"
    bar = n * 1.0e-6
    assert abs(err - bar) > 1e-6 * bar, f"{name}: the stopping L1 change {err} is too close to n * tol {bar}"
    if iters > 1:  # and one step fewer does not get there
        try:
            nx.pagerank(G, max_iter=iters - 1, weight="weight")
        except nx.PowerIterationFailedConvergence:
            pass
        else:
            raise AssertionError(f"{name}: nx.pagerank converged before iteration {iters}")
    src = np.array([index[u] for u, v in G.edges()], dtype=np.int64)
    dst = np.array([index[v] for u, v in G.edges()], dtype=np.int64)
    w = np.array([G[u][v]["weight"] for u, v in G.edges()], dtype=np.float64)
    out[f"{name}_n"] = np.int64(n)
    out[f"{name}_src"], out[f"{name}_dst"], out[f"{name}_w"] = src, dst, w
    out[f"{name}_importance"] = imp
    out[f"{name}_centrality"] = cent
    out[f"{name}_iters"] = np.int32(iters)
    out[f"{name}_khop"] = np.float64(k_hop)
    retr = gr_mod.GraphRetriever(gi, k_hop=k_hop)
    seed_offs, seeds, res_offs, r_ids, r_dist, r_score, tie_offs, ties = [0], [], [0], [], [], [], [0], []
    for sl in seed_lists:
        res = retr.retrieve(sl)
        seeds += [index.get(s, -1) for s in sl]
        seed_offs.append(len(seeds))
        sc = [r["graph_score"] for r in res]
        assert all(a >= b for a, b in zip(sc, sc[1:]))
        groups, i = [], 0
        while i < len(sc):
            j = i
            while j + 1 < len(sc) and sc[j + 1] == sc[i]:
                j += 1
            if j > i:
                groups.append((i, j + 1))
            i = j + 1
        tied = sum(b - a for a, b in groups)
        assert tied * 100 <= len(sc), f"{name}: {tied} of {len(sc)} entries tie on graph_score"
        ties += groups
        tie_offs.append(len(ties))
        for r in res:
            assert r["centrality"] == cent[index[r["note_id"]]]
            assert r["paragraph_idxs"] == [index[r["note_id"]] % 7]
        r_ids += [index[r["note_id"]] for r in res]
        r_dist += [r["graph_distance"] for r in res]
        r_score += sc
        res_offs.append(len(r_ids))
    out[f"{name}_seed_offs"] = np.array(seed_offs, dtype=np.int64)
    out[f"{name}_seeds"] = np.array(seeds, dtype=np.int64)
    out[f"{name}_res_offs"] = np.array(res_offs, dtype=np.int64)
    out[f"{name}_res_ids"] = np.array(r_ids, dtype=np.int64)
    out[f"{name}_res_dist"] = np.array(r_dist, dtype=np.float64)
    out[f"{name}_res_score"] = np.array(r_score, dtype=np.float64)
    out[f"{name}_tie_offs"] = np.array(tie_offs, dtype=np.int64)
    out[f"{name}_tie_groups"] = np.array(ties, dtype=np.int64).reshape(-1, 2)
    print(f"{name}: n={n} edges={len(w)} iters={iters} err/bar={err / bar:.4f} results={np.diff(res_offs).tolist()} "
          f"tie groups={len(ties)}")


def relations_case():
    """notes and relations with a repeated pair (both directions), an endpoint that is no note, a note without an id —
    through nx.Graph exactly as graph/graph_builder.py:21-35 feeds it"""
    notes = [{"note_id": "a", "importance_score": 2.0}, {"note_id": "b"}, {"content": "no id"}, {"note_id": "c"},
             {"note_id": "d", "paragraph_idxs": [3]}, {"note_id": "b", "importance_score": 0.5}]
    rels = [{"source_id": "a", "target_id": "b", "weight": 0.4, "relation_type": "x"},
            {"source_id": "c", "target_id": "a", "weight": 0.6, "relation_type": "x"},
            {"source_id": "b", "target_id": "a", "weight": 0.7, "relation_type": "y", "metadata": {"k": 1}},
            {"source_id": "d", "target_id": "e", "relation_type": "x"},
            {"source_id": "", "target_id": "a", "weight": 0.9},
            {"source_id": "c", "target_id": "d", "weight": 0.55}]
    G = nx.Graph()
    for note in notes:
        node_id = note.get("note_id")
        if not node_id:
            continue
        G.add_node(node_id, **note)
    for rel in rels:
        src, tgt = rel.get("source_id"), rel.get("target_id")
        if src and tgt:
            G.add_edge(src, tgt, weight=rel.get("weight", 1.0), relation_type=rel.get("relation_type"),
                       **rel.get("metadata", {}))
    order = list(G)
    idx = {v: i for i, v in enumerate(order)}
    edges = sorted([min(idx[u], idx[v]), max(idx[u], idx[v]), G[u][v]["weight"]] for u, v in G.edges())
    return {"notes": notes, "relations": rels, "node_order": order, "edges": edges,
            "importance": [G.nodes[v].get("importance_score", 1.0) for v in order]}


def main():
    stub_modules()
    gi_mod = load("graph_index")
    gr_mod = load("graph_retriever")
    out = {}
    rng = random.Random(20261017)
    # A: isolated nodes (dangling mass), an island component, non-uniform importance; seed lists of every awkward kind
    G, ids, imp = make_graph(rng, 1500, 7, n_isolated=25, island=60, importance_share=0.5)
    main_n = 1500 - 25 - 60
    nbr = list(G[ids[10]])
    lists = [
        [ids[10], nbr[0], nbr[1]],                       # seeds that reach each other
        [ids[3], "ghost", ids[700], ids[3], ids[40]],    # a seed that is no node, a repeated seed
        [],                                              # no seeds
        [ids[main_n + 5], ids[200]],                     # one seed on the island, one on the mainland
        [ids[1499]],                                     # an isolated seed: reaches nothing
        [ids[i] for i in rng.sample(range(main_n), 20)],  # a question's worth of dense hits
        ["ghost"],
    ]
    record(out, "A", G, ids, imp, 2, lists, gi_mod, gr_mod)
    # B: denser and smaller, uniform importance, a tighter cutoff
    G, ids, imp = make_graph(rng, 400, 12, n_isolated=3, island=0, importance_share=0.0)
    lists = [[ids[i] for i in rng.sample(range(390), 8)], [ids[0], ids[1]], [ids[5]]]
    record(out, "B", G, ids, imp, 1, lists, gi_mod, gr_mod)
    out["relations_case"] = np.array(json.dumps(relations_case()))
    path = os.path.join(HERE, "notegraph_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
