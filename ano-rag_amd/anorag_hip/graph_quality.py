"""Drop-in for the reference's ``graph/graph_quality.py``: ``compute_metrics(graph)`` on the device.

``GraphBuilder.build_graph_with_metrics`` (graph/graph_builder.py:39-49) calls ``compute_metrics(G)`` on every graph it
builds; its ``nx.average_shortest_path_length`` is one Python BFS per node.  Here the components and the hop counts come
from ``NoteGraph`` (csrc/notegraph.hip) and only the last division is Python's, so the dict equals the
reference's in every value.  networkx is not imported: any object with ``number_of_nodes()``, ``nodes()`` and ``edges()``
will do, and so will a ``NoteGraph``.
"""
from __future__ import annotations

from typing import Any, Dict, Tuple

import numpy as np

from .note_graph import NoteGraph


def empty_metrics() -> Dict[str, float]:
    """the reference's answer for a graph with no nodes (graph_quality.py:22-28): no ``component_sizes``"""
    return {
        "average_degree": 0.0,
        "num_components": 0.0,
        "largest_component_size": 0.0,
        "average_shortest_path_length": 0.0,
    }


def graph_arrays(graph: Any) -> Tuple[int, np.ndarray, np.ndarray, int]:
    """host half (no device): (n, src, dst, self_loops) of an nx.Graph-like object.  A node's index is its position in
    ``graph.nodes()`` — the order nx.connected_components visits; an edge between the same two nodes is kept once (an
    nx.Graph holds it once), at its first mention; self-loops are counted, not kept."""
    index = {v: i for i, v in enumerate(graph.nodes())}
    pairs: Dict[Tuple[int, int], None] = {}
    loops = 0
    for e in graph.edges():
        a, b = index[e[0]], index[e[1]]
        if a == b:
            loops += 1
        else:
            pairs.setdefault((a, b) if a < b else (b, a))
    arr = np.asarray(list(pairs.keys()), dtype=np.int64).reshape(-1, 2)
    return len(index), arr[:, 0].copy(), arr[:, 1].copy(), loops


def compute_metrics(graph: Any, device: int = 0) -> Dict[str, Any]:
    """graph_quality.compute_metrics: average degree, number of components, size of the largest, the average shortest
    path length (in hops) of the largest — the first of equal sizes in node order — and ``component_sizes``."""
    if isinstance(graph, NoteGraph):
        return graph.quality_metrics()
    if graph.number_of_nodes() == 0:
        return empty_metrics()
    n, src, dst, loops = graph_arrays(graph)
    g = NoteGraph(n, src, dst, np.ones(len(src), dtype=np.float64), device)
    try:
        return g.quality_metrics(self_loops=loops)
    finally:
        g.close()
