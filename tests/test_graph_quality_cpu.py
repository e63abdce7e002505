"""CPU tests of the graph quality metrics: the numpy restatement (tests/graph_quality_ref.py) equals what the reference's
compute_metrics returned (tests/golden/graph_quality_cases.npz) in every value, floats by their bits; it does not depend
on its words per pass; the host half of the drop-in turns an nx-like graph into the recorded indices."""
import numpy as np
import pytest

import graph_quality_ref as ref
from graph_quality_cases import CASES, EMPTY, KEYS, NAMED, NamedGraph, assert_same_dict, load_case


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(name):
    n, src, dst, loops, want, hist = load_case(name)
    got, got_hist = ref.metrics(n, src, dst, loops)
    assert_same_dict(got, want)
    assert got_hist.dtype == np.int64 and np.array_equal(got_hist, hist)


@pytest.mark.parametrize("name", ["path130", "equal_largest", "random300", "named"])
def test_restatement_does_not_depend_on_its_words(name):
    n, src, dst, loops, want, hist = load_case(name)
    for words in (1, 2, 16):
        got, got_hist = ref.metrics(n, src, dst, loops, words=words)
        assert_same_dict(got, want)
        assert np.array_equal(got_hist, hist)


def test_restatement_counts_repeated_sources_apart():
    n, src, dst, _, _, _ = load_case("random300")
    one = ref.hop_histogram(n, src, dst, [5])
    assert ref.hop_histogram(n, src, dst, [5, 5], words=1).tolist() == (2 * one).tolist()


def test_host_conversion_matches_the_recorded_indices():
    from anorag_hip.graph_quality import graph_arrays
    n, src, dst, loops, _, _ = load_case("named")
    gn, gsrc, gdst, gloops = graph_arrays(NamedGraph(NAMED["nodes"], NAMED["edges"]))
    assert (gn, gloops) == (n, loops) and gsrc.dtype == np.int64 and gdst.dtype == np.int64
    assert sorted(zip(np.minimum(gsrc, gdst).tolist(), np.maximum(gsrc, gdst).tolist())) == \
        sorted(zip(np.minimum(src, dst).tolist(), np.maximum(src, dst).tolist()))
    # an edge given in both directions is one edge; a graph without edges gives empty index arrays
    gn, gsrc, gdst, gloops = graph_arrays(NamedGraph("abc", [("a", "b"), ("b", "a"), ("c", "c")]))
    assert (gn, gsrc.tolist(), gdst.tolist(), gloops) == (3, [0], [1], 1)
    gn, gsrc, gdst, gloops = graph_arrays(NamedGraph("ab", []))
    assert gn == 2 and gsrc.shape == (0,) and gdst.shape == (0,) and gloops == 0


def test_no_nodes_dict_needs_no_device():
    from anorag_hip.graph_quality import compute_metrics, empty_metrics
    got = compute_metrics(NamedGraph([], []), device=10 ** 6)  # a device that does not exist: never touched
    assert list(got.keys()) == KEYS == list(EMPTY.keys()) and "component_sizes" not in got
    assert_same_dict(got, EMPTY)
    assert got == empty_metrics()


def test_module_is_exported():
    import anorag_hip
    assert anorag_hip.compute_metrics is anorag_hip.graph_quality.compute_metrics
