"""Loader of tests/golden/graph_quality_cases.npz (made by tests/golden/make_graph_quality_golden.py from the reference's
compute_metrics) for the CPU and GPU graph-quality tests."""
import json
import os
import struct

import numpy as np

KEYS = ["average_degree", "num_components", "largest_component_size", "average_shortest_path_length"]
_Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_quality_cases.npz"))
CASES = json.loads(str(_Z["names"]))
EMPTY = json.loads(str(_Z["empty_keys"]))
NAMED = json.loads(str(_Z["named_case"]))


def load_case(name):
    """(n, src, dst, self_loops, golden dict, golden histogram)"""
    d = {k: float(v) for k, v in zip(KEYS, _Z[f"{name}_floats"])}
    d["component_sizes"] = [int(s) for s in _Z[f"{name}_sizes"]]
    return int(_Z[f"{name}_n"]), _Z[f"{name}_src"], _Z[f"{name}_dst"], int(_Z[f"{name}_loops"]), d, _Z[f"{name}_hist"]


def bits(x):
    return struct.pack("<d", x)


def assert_same_dict(got, want):
    """equal keys in equal order, equal types, floats equal by their bits"""
    assert list(got.keys()) == list(want.keys())
    for k in KEYS:
        assert type(got[k]) is float and bits(got[k]) == bits(want[k]), (k, got[k], want[k])
    if "component_sizes" in want:
        assert type(got["component_sizes"]) is list and all(type(s) is int for s in got["component_sizes"])
        assert got["component_sizes"] == want["component_sizes"]


class NamedGraph:
    """the three methods compute_metrics needs of an nx.Graph, over recorded names (no networkx)"""

    def __init__(self, nodes, edges):
        self._nodes, self._edges = list(nodes), [tuple(e) for e in edges]

    def number_of_nodes(self):
        return len(self._nodes)

    def nodes(self):
        return iter(self._nodes)

    def edges(self):
        return iter(self._edges)
