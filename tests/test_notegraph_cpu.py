"""CPU tests of the note graph (no GPU needed): the numpy restatement (tests/notegraph_ref.py) — the checker the GPU tests
use — against what the reference's own GraphIndex.build_index / GraphRetriever.retrieve produced
(tests/golden/notegraph_cases.npz), the host half of NoteGraph.from_relations against nx.Graph, and the argument checks
of anr_notegraph_create that run before any device work."""
import ctypes as C
import logging

import numpy as np
import pytest

import notegraph_ref as ref
from notegraph_cases import CASES, load_case, max_rel_diff, pagerank_bound, relations_case

log = logging.getLogger(__name__)


def compare_result(got, want, ties):
    """ids, order, graph_distance and graph_score bit for bit; inside a recorded tie group (equal graph_score) the
    entries are compared as a set"""
    ids, dist, score = got
    w_ids, w_dist, w_score = want
    assert len(ids) == len(w_ids)
    assert score.tobytes() == w_score.tobytes()
    free = np.zeros(len(ids), dtype=bool)
    for a, b in ties:
        free[a:b] = True
        assert sorted(zip(ids[a:b].tolist(), dist[a:b].tolist())) == sorted(zip(w_ids[a:b].tolist(), w_dist[a:b].tolist()))
    assert np.array_equal(ids[~free], w_ids[~free])
    assert dist[~free].tobytes() == w_dist[~free].tobytes()


@pytest.mark.parametrize("name", CASES)
def test_restatement_retrieve_equals_the_reference_run(name):
    c = load_case(name)
    rowptr, nbr, wt = ref.build_csr(c["n"], c["src"], c["dst"], c["w"])
    for seeds, want, ties in zip(c["seed_lists"], c["results"], c["ties"]):
        ids, dist, score, _ = ref.retrieve(c["n"], rowptr, nbr, wt, seeds, c["khop"], c["centrality"], c["importance"])
        compare_result((ids, dist, score), want, ties)


@pytest.mark.parametrize("name", CASES)
def test_restatement_pagerank_iterations_and_derived_bound(name):
    """Same iteration count as nx.pagerank (the maker asserts the stopping L1 change is not within a relative 1e-6 of
    n * tol, so the count cannot flip by rounding) and values within notegraph_cases.pagerank_bound — see its docstring
    for the derivation; the observed maximum is logged beside the bound."""
    c = load_case(name)
    rowptr, nbr, wt = ref.build_csr(c["n"], c["src"], c["dst"], c["w"])
    x, iters = ref.pagerank(c["n"], rowptr, nbr, wt)
    assert iters == c["iters"]
    bound = pagerank_bound(c["n"], c["src"], c["dst"], iters)
    seen = max_rel_diff(x, c["centrality"])
    log.info("case %s: max relative difference %.3e, bound %.3e", name, seen, bound)
    print(f"case {name}: n={c['n']} iterations={iters} max relative difference {seen:.3e} bound {bound:.3e}")
    assert seen <= bound
    assert bound < 1e-11          # the bound itself stays a rounding-level statement
    with pytest.raises(RuntimeError):
        ref.pagerank(c["n"], rowptr, nbr, wt, max_iter=iters - 1)


def test_tree_sum_shape():
    assert ref.tree_sum(np.ones(5000)) == 5000.0 and ref.tree_sum(np.zeros(0)) == 0.0
    v = np.random.default_rng(0).random(300_000)
    assert abs(ref.tree_sum(v) - float(np.sum(v))) <= 64 * 2.0 ** -53 * float(np.sum(v))
    # the documented order, spelled out for one chunk: thread t owns t, t + 256, t + 512, t + 768
    w = np.random.default_rng(1).random(1024)
    t = ((w[:256] + w[256:512]) + w[512:768]) + w[768:]
    for s in (128, 64, 32, 16, 8, 4, 2, 1):
        t = t[:s] + t[s:2 * s]
    assert ref.tree_sum(w) == t[0]


def test_from_relations_reproduces_nx_node_order_and_last_edge_wins():
    from anorag_hip import NoteGraph
    rc = relations_case()
    note_ids, nodes, src, dst, w, imp = NoteGraph.edges_from_relations(rc["notes"], rc["relations"])
    assert note_ids == rc["node_order"]
    got = sorted([int(a), int(b), float(x)] for a, b, x in zip(src, dst, w))
    assert got == rc["edges"]
    assert [0, 1, 0.7] in got                         # a-b was related twice: the later weight stays
    assert imp.tolist() == rc["importance"]
    assert nodes[note_ids.index("d")]["paragraph_idxs"] == [3] and nodes[note_ids.index("e")] == {}
    with pytest.raises(ValueError):
        NoteGraph.edges_from_relations([{"note_id": "a"}], [{"source_id": "a", "target_id": "a"}])


def test_create_rejects_bad_graphs_before_any_device_work():
    from anorag_hip import _lib
    lib = _lib.load()

    def create(n, src, dst, w):
        s, d, ww = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(w, np.float64)
        h = C.c_void_p()
        rc = lib.anr_notegraph_create(0, n, len(s), s.ctypes.data, d.ctypes.data, ww.ctypes.data, C.byref(h))
        assert not h.value or rc == 0
        if h.value:
            lib.anr_notegraph_destroy(h)
        return rc, _lib.last_error()

    for args, word in (((4, [0, 2], [1, 2], [0.5, 0.5]), "self-loop"), ((4, [0], [1], [-0.1]), "weight"),
                       ((4, [0], [1], [np.nan]), "weight"), ((4, [0], [1], [np.inf]), "weight"),
                       ((4, [0], [4], [0.5]), "range"), ((4, [-1], [2], [0.5]), "range"), ((0, [], [], []), "n_nodes")):
        rc, msg = create(*args)
        assert rc == -1 and word in msg, (args, rc, msg)


def test_note_graph_fails_loudly_without_a_device():
    from anorag_hip import AnoragError, NoteGraph, _lib
    if _lib.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(AnoragError) as e:
        NoteGraph(3, [0], [1], [0.5])
    assert "no HIP device" in str(e.value)
