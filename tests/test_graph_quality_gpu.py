"""GPU tests of the graph quality metrics (anr_notegraph_components, anr_notegraph_hop_histogram, NoteGraph.quality_metrics,
anorag_hip.graph_quality.compute_metrics): the dict equals what the reference's compute_metrics returned (the goldens),
floats by their bits; labels, sizes and histogram equal the numpy restatement (tests/graph_quality_ref.py); results do
not depend on the words per pass, at every pass boundary; the handle's other state is left as it was."""
import ctypes as C
import functools

import numpy as np
import pytest

import graph_quality_ref as ref
from graph_quality_cases import CASES, NAMED, NamedGraph, assert_same_dict, load_case

pytestmark = pytest.mark.gpu
ANR_EINVAL = -1
OPT_BFS_WORDS = 2


class Handle:
    """the C ABI as it is, without the NoteGraph class"""

    def __init__(self, n, src, dst):
        from anorag_hip import _lib as L
        self.L, self.lib, self.n = L, L.load(), int(n)
        s, d = np.ascontiguousarray(src, np.int64), np.ascontiguousarray(dst, np.int64)
        w = np.ones(len(s), np.float64)
        self.h = C.c_void_p()
        rc = self.lib.anr_notegraph_create(0, self.n, len(s), s.ctypes.data, d.ctypes.data, w.ctypes.data, C.byref(self.h))
        assert rc == 0, L.last_error()

    def words(self, w):
        assert self.lib.anr_notegraph_set_option(self.h, OPT_BFS_WORDS, w) == 0, self.L.last_error()

    def components(self):
        lab = np.full(self.n, -7, np.int32)
        nc = C.c_int64(-7)
        assert self.lib.anr_notegraph_components(self.h, lab.ctypes.data, C.byref(nc)) == 0, self.L.last_error()
        return lab.astype(np.int64), nc.value

    def hist_raw(self, sources, cap):
        counts = np.full(max(cap, 1), -7, np.int64)
        nl = C.c_int64(-7)
        stats = np.full(8, -7, np.int64)
        if sources is None:
            ns, ptr = 0, None
        else:
            sources = np.ascontiguousarray(sources, np.int64)
            ns, ptr = len(sources), sources.ctypes.data
        rc = self.lib.anr_notegraph_hop_histogram(self.h, ns, ptr, cap, counts.ctypes.data, C.byref(nl), stats.ctypes.data)
        return rc, counts, nl.value, stats

    def hist(self, sources=None):
        rc, counts, nl, stats = self.hist_raw(sources, self.n)
        assert rc == 0, self.L.last_error()
        assert (counts[nl:self.n] == 0).all()
        return counts[:nl].copy(), stats

    def close(self):
        if self.h.value:
            assert self.lib.anr_notegraph_destroy(self.h) == 0
            self.h = C.c_void_p()


def largest_nodes(labels, sizes):
    roots = np.flatnonzero(labels == np.arange(len(labels)))
    return np.flatnonzero(labels == roots[sizes.index(max(sizes))])


@pytest.mark.parametrize("name", CASES)
def test_c_abi_equals_golden_and_restatement(name):
    n, src, dst, loops, want, hist = load_case(name)
    rlabels, rsizes = ref.components(n, src, dst)
    h = Handle(n, src, dst)
    try:
        labels, nc = h.components()
        assert np.array_equal(labels, rlabels) and nc == len(rsizes) == int(want["num_components"])
        roots = np.flatnonzero(labels == np.arange(n))
        assert np.bincount(labels, minlength=n)[roots].tolist() == want["component_sizes"]
        got, stats = h.hist(largest_nodes(labels, rsizes))
        assert np.array_equal(got, hist)
        assert stats[0] == 64 * stats[4] and stats[1] == -(-len(largest_nodes(labels, rsizes)) // stats[0])
        assert stats[2] >= len(hist) and stats[3] >= 3 * n * stats[4] * 8
        # every node a source: the pairs inside every component
        all_got, _ = h.hist(None)
        assert np.array_equal(all_got, ref.hop_histogram(n, src, dst))
    finally:
        h.close()


@pytest.mark.parametrize("name", CASES)
def test_notegraph_and_dropin_equal_golden(name):
    from anorag_hip import NoteGraph, compute_metrics
    n, src, dst, loops, want, hist = load_case(name)
    g = NoteGraph(n, src, dst, np.ones(len(src)))
    try:
        assert_same_dict(g.quality_metrics(self_loops=loops), want)
        labels, sizes = g.components()
        assert labels.dtype == np.int64 and sizes == want["component_sizes"]
        got = g.hop_histogram(largest_nodes(labels, sizes))
        assert got.dtype == np.int64 and np.array_equal(got, hist)
        if loops == 0:
            assert_same_dict(compute_metrics(g), want)
    finally:
        g.close()
    if name == "named":
        graph = NamedGraph(NAMED["nodes"], NAMED["edges"])
    else:
        graph = NamedGraph(range(n), zip(src.tolist(), dst.tolist()))
    assert_same_dict(compute_metrics(graph), want)


@functools.lru_cache(maxsize=None)
def ring_case(n_nodes, ring, seed):
    src, dst = ref.ring_with_chords(n_nodes, ring, seed)
    labels, sizes = ref.components(n_nodes, src, dst)
    assert max(sizes) == ring and sizes.count(ring) == 1
    nodes = largest_nodes(labels, sizes)
    return src, dst, nodes, ref.hop_histogram(n_nodes, src, dst, nodes), ref.metrics(n_nodes, src, dst)[0]


@pytest.mark.parametrize("words", [1, 2, 0])
def test_pass_boundaries(words):
    from anorag_hip import NoteGraph
    probe = Handle(2, [0], [1])
    probe.words(words)
    B = int(probe.hist()[1][0])
    probe.close()
    assert B == 64 * (words or 16)
    for ring in (B - 1, B, B + 1, 2 * B + 1):
        n_nodes = ring + 40
        src, dst, nodes, want_hist, want = ring_case(n_nodes, ring, 7)
        h = Handle(n_nodes, src, dst)
        try:
            h.words(words)
            got, stats = h.hist(nodes)
            assert np.array_equal(got, want_hist), (words, ring)
            assert stats[0] == B and stats[1] == -(-ring // B)
        finally:
            h.close()
        g = NoteGraph(n_nodes, src, dst, np.ones(len(src)))
        try:
            g.set_bfs_words(words)
            assert_same_dict(g.quality_metrics(), want)
        finally:
            g.close()


def test_settings_agree_on_one_handle():
    src, dst, nodes, want_hist, _ = ring_case(300, 257, 3)
    h = Handle(300, src, dst)
    try:
        for words in (1, 2, 0, 4, 1):
            h.words(words)
            got, stats = h.hist(nodes)
            assert stats[4] == (words or 16) and np.array_equal(got, want_hist), words
        assert h.lib.anr_notegraph_set_option(h.h, OPT_BFS_WORDS, 3) == ANR_EINVAL
    finally:
        h.close()


@pytest.mark.parametrize("n", [255, 256, 257])
def test_node_counts_at_workgroup_edges(n):
    rng = np.random.default_rng(n)
    pairs = {(min(a, b), max(a, b)) for a, b in rng.integers(0, n, (n, 2)).tolist() if a != b}
    pairs |= {(n - 2, n - 1), (0, n - 1)}
    arr = np.asarray(sorted(pairs), np.int64)
    src, dst = arr[:, 0].copy(), arr[:, 1].copy()
    h = Handle(n, src, dst)
    try:
        labels, nc = h.components()
        rlabels, rsizes = ref.components(n, src, dst)
        assert np.array_equal(labels, rlabels) and nc == len(rsizes)
        for words in (1, 0):
            h.words(words)
            assert np.array_equal(h.hist()[0], ref.hop_histogram(n, src, dst))
        # an explicit list: a subset in scrambled order, with one node given twice
        sources = np.concatenate([rng.permutation(n)[:100], [n - 1, n - 1, 0]])
        h.words(1)
        assert np.array_equal(h.hist(sources)[0], ref.hop_histogram(n, src, dst, sources, words=1))
    finally:
        h.close()


def test_larger_graph():
    n, E = 8192, 24000
    rng = np.random.default_rng(20261017)
    pairs = set()
    while len(pairs) < E:
        ab = rng.integers(0, n, (E, 2))
        pairs |= {(min(a, b), max(a, b)) for a, b in ab.tolist() if a != b}
    arr = np.asarray(sorted(pairs), np.int64)[rng.permutation(len(pairs))[:E]]
    src, dst = arr[:, 0].copy(), arr[:, 1].copy()
    want, want_hist = ref.metrics(n, src, dst)
    from anorag_hip import NoteGraph
    g = NoteGraph(n, src, dst, np.ones(E))
    try:
        assert_same_dict(g.quality_metrics(), want)
        labels, sizes = g.components()
        assert np.array_equal(labels, ref.components(n, src, dst)[0])
        assert np.array_equal(g.hop_histogram(largest_nodes(labels, sizes)), want_hist)
        assert g.last_bfs_stats["passes"] == -(-max(sizes) // 1024)
    finally:
        g.close()


def test_same_handle_state():
    """two calls agree; pagerank and retrieve are the same bits before and after the quality calls"""
    from anorag_hip import NoteGraph
    n, src, dst, loops, want, hist = load_case("random300")
    w = np.random.default_rng(1).uniform(0.3, 0.9, len(src))
    g = NoteGraph(n, src, dst, w)
    try:
        pr0 = g.pagerank()
        seeds = [[3, 50, 120], [7], []]
        r0 = g.retrieve_raw(seeds, 1.5, n)
        m1 = g.quality_metrics()
        m2 = g.quality_metrics()
        assert_same_dict(m1, want)
        assert_same_dict(m2, want)
        g.set_bfs_words(1)
        assert_same_dict(g.quality_metrics(), want)
        r1 = g.retrieve_raw(seeds, 1.5, n)
        for a, b in zip(r0, r1):
            assert a.tobytes() == b.tobytes()
        assert g.pagerank().tobytes() == pr0.tobytes()
        r2 = g.retrieve_raw(seeds, 1.5, n)
        for a, b in zip(r0, r2):
            assert a.tobytes() == b.tobytes()
        assert_same_dict(g.quality_metrics(), want)
    finally:
        g.close()


def test_rejections_leave_the_handle_usable():
    n, src, dst, loops, want, hist = load_case("path130")
    h = Handle(n, src, dst)
    try:
        for bad in ([0, n], [-1], [5, 2 ** 40]):
            rc, counts, nl, _ = h.hist_raw(bad, n)
            assert rc == ANR_EINVAL and (counts == -7).all()
        rc, counts, nl, _ = h.hist_raw(None, 20)  # 130 levels do not fit 20
        assert rc == ANR_EINVAL and nl == 130 and (counts == -7).all()
        rc, counts, nl, _ = h.hist_raw(None, 130)
        assert rc == 0 and nl == 130 and np.array_equal(counts, hist)
        rc, counts, nl, _ = h.hist_raw(np.zeros(1, np.int64)[:0], 4)  # no sources: nothing to count
        assert rc == 0 and nl == 0 and (counts[:4] == 0).all()
        got, _ = h.hist(None)
        assert np.array_equal(got, hist)
    finally:
        h.close()
