"""CPU tests of the graph restatement (tests/graph_ref.py) and of the graph save trailer's pure-Python helpers."""
import io
import struct

import numpy as np

import graph_ref


def test_knn_lists_drop_self_or_the_last_entry():
    I = np.array([[0, 2, 1], [2, 1, 0], [1, 0, -1]])  # row 1: own id in the middle; row 2: own id absent
    assert graph_ref.knn_lists(I, 2).tolist() == [[2, 1], [2, 0], [1, 0]]
    # raw IP, hand-computed: row 1 = (0.1, 0) scores 0.1 with row 0, 0.05 with row 3, 0.01 with itself, 0 with row 2;
    # its top-2 [0, 3] lacks its own id, so the last entry goes
    x = np.array([[1, 0], [0.1, 0], [0, 1], [0.5, 0.5]])
    s = x @ x.T
    I = np.array([sorted(range(4), key=lambda j: (-s[i, j], j))[:2] for i in range(4)])
    assert I[1].tolist() == [0, 3] and graph_ref.knn_lists(I, 1)[1].tolist() == [0]


def test_detour_and_forward_order_known_answer():
    # row 0 lists [1, 2, 3]; 2 is reached through 1 (L_1 = [2, ...] at position 0 < 1) and 3 through 1 and 2
    L = np.array([[1, 2, 3], [2, 3, 0], [3, 0, 1], [0, 1, 2]], dtype=np.int32)
    det = graph_ref.detours(L)
    assert det[0].tolist() == [0, 1, 2]
    assert np.array_equal(det, graph_ref.detours_fast(L))
    assert graph_ref.forward_order(L)[0].tolist() == [1, 2, 3]
    # an entry with fewer detours moves ahead of a closer one; ties keep the rank order
    L2 = np.array([[1, 2, 3, 4], [2, 3, 0, 4], [3, 0, 1, 4], [0, 1, 2, 4], [0, 1, 2, 3]], dtype=np.int32)
    det2 = graph_ref.detours(L2)
    F = graph_ref.forward_order(L2, det2)
    for i in range(5):
        key = [(det2[i, r], r) for r in range(4)]
        assert F[i].tolist() == [int(L2[i, r]) for _, r in sorted(key)]


def test_prune_reverse_edges_duplicates_and_padding():
    # n = 3 <= R: every list is padded with -1
    L = np.array([[1, 2], [0, 2], [1, 0]], dtype=np.int32)
    adj = graph_ref.prune(L, 4)
    assert adj.shape == (3, 4) and (adj[:, 2:] == -1).all()
    assert sorted(adj[0, :2].tolist()) == [1, 2] and -1 not in adj[:, :2]
    # reverse edges: 3 is listed by nobody's first half but lists 0 first; 0 gets 3 as a reverse candidate before
    # the rest of its own list
    # (hand-computed: row 2 has detours [0, 1, 0], so 4 moves ahead of 1; row 3 has [0, 1, 2])
    L = np.array([[1, 2, 4], [0, 2, 4], [0, 1, 4], [0, 1, 2], [0, 1, 2]], dtype=np.int32)
    det = graph_ref.detours(L)
    assert det[2].tolist() == [0, 1, 0] and det[3].tolist() == [0, 1, 2] and det[0].tolist() == [0, 0, 0]
    F = graph_ref.forward_order(L)
    assert F.tolist() == [[1, 2, 4], [0, 2, 4], [0, 4, 1], [0, 1, 2], [0, 1, 2]]
    # R = 2: the first F entry, then the reverse candidates (0 is the first entry of rows 1-4, 1 that of row 0: row 0
    # gets 2 from them), then the rest of F (rows 1-4 have no reverse candidate)
    assert graph_ref.prune(L, 2, F).tolist() == [[1, 2], [0, 2], [0, 4], [0, 1], [0, 1]]
    # R = 4 on the 4-cycle L_i = [i+1, i+2, i+3]: F = L, the reverse candidate i-1 = i+3 completes the list, padding
    L4 = np.array([[(i + d) % 4 for d in (1, 2, 3)] for i in range(4)], dtype=np.int32)
    assert graph_ref.prune(L4, 4).tolist() == [[1, 2, 3, -1], [2, 3, 0, -1], [3, 0, 1, -1], [0, 1, 2, -1]]
    assert graph_ref.prune(L4, 2).tolist() == [[1, 3], [2, 0], [3, 1], [0, 2]]
    # padding inside kNN lists (fewer rows than K + 1) stays out of the graph
    L = np.array([[1, -1, -1], [0, -1, -1]], dtype=np.int32)
    assert graph_ref.prune(L, 2).tolist() == [[1, -1], [0, -1]]


def test_duplicate_rows_and_self_absent_lists_prune_deterministically():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((40, 6)).astype(np.float32)
    x[5] = x[7]                                        # duplicate rows: tie by ascending id
    x[9] *= 0.01                                       # small row: under raw IP its own id is not its best
    s = x.astype(np.float64) @ x.astype(np.float64).T
    I = np.array([sorted(range(40), key=lambda j: (-s[i, j], j))[:9] for i in range(40)])
    assert 9 not in I[9].tolist()
    L = graph_ref.knn_lists(I, 8)
    assert L[9].tolist() == I[9, :8].tolist()
    a = graph_ref.prune(L, 6)
    assert np.array_equal(a, graph_ref.prune(L.copy(), 6))
    assert np.array_equal(graph_ref.detours(L), graph_ref.detours_fast(L))
    for i in range(40):
        row = [v for v in a[i].tolist() if v >= 0]
        assert len(row) == len(set(row)) and i not in row


def test_quantize_is_exact_power_of_two_scaling():
    x = np.array([[0.5, -0.25, 0.0], [0.0, 0.0, 0.0], [3.0, 1e-3, -2.0]], dtype=np.float32)
    c, e = graph_ref.quantize(x)
    assert e.tolist() == [-7, 0, -5] and c[0].tolist() == [64, -32, 0] and c[2, 0] == 96
    d = graph_ref.decode(c, e)
    assert d[0].tolist() == [0.5, -0.25, 0.0] and (d[1] == 0).all()
    c, e = graph_ref.quantize(np.array([[0.99999994]], np.float32))  # rounds to 128: clamped
    assert c[0, 0] == 127


def _toy():
    # a ring of 16 points on the unit circle, each linked to its two neighbours
    ang = np.arange(16) * (2 * np.pi / 16)
    x = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
    adj = np.array([[(i + 1) % 16, (i - 1) % 16] for i in range(16)], dtype=np.int32)
    return x, adj


def test_beam_search_known_answer_entry_and_termination():
    x, adj = _toy()
    img = graph_ref.decode(*graph_ref.quantize(x))
    q = x[5:6] * 2
    D, I, it, scored, capped = graph_ref.search(q, img, x, adj, 3, 1, "ip")
    # n < 4096: the entry sample is all 16 rows (stride 1), every row is scored first; exact answer
    assert I[0].tolist() == [5, 4, 6] and not capped[0] and scored[0] == 16
    assert it[0] == 1  # p = 128 parents per iteration: one iteration expands all 16 and finds nothing new
    Dl, Il, _, _, _ = graph_ref.search(q, img, x, adj, 20, 1, "l2")
    assert Il[0, :3].tolist() == [5, 4, 6] and (Il[0, 16:] == -1).all() and Dl[0, 19] == graph_ref.FLT_MAX


def test_beam_search_walks_a_larger_ring_and_stops():
    n = 5000
    ang = np.arange(n) * (2 * np.pi / n)
    x = np.stack([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
    adj = np.array([[(i + d) % n for d in (1, -1, 2, -2, 16, -16, 128, -128)] for i in range(n)], dtype=np.int32)
    img = graph_ref.decode(*graph_ref.quantize(x))
    q = x[[4500, 4300]]
    D, I, it, scored, capped = graph_ref.search(q, img, x, adj, 5, 64, "ip")
    # the entry sample is rows 0..4095: the beam has to walk to rows beyond it
    # (2-D points: the int8 traversal keys cannot order neighbours a few steps apart, the float64 re-score can)
    assert I[0, 0] == 4500 and all(abs(v - 4500) <= 4 for v in I[0].tolist())
    assert I[1, 0] == 4300 and all(abs(v - 4300) <= 4 for v in I[1].tolist())
    assert not any(capped) and all(i >= 2 for i in it) and all(s > 4096 for s in scored)
    assert np.allclose(D[0], x[I[0]].astype(np.float64) @ x[4500].astype(np.float64))


def test_forgetful_visited_set_gives_the_same_result():
    # more rows than the entry sample (4096): the beam walks, rows leave it and their ids come back as neighbours
    rng = np.random.default_rng(3)
    n, d = 12000, 8
    x = rng.standard_normal((n, d)).astype(np.float32)
    x64 = x.astype(np.float64)
    I = np.concatenate([np.argsort(-(x64[a:a + 2000] @ x64.T), axis=1, kind="stable")[:, :17]
                        for a in range(0, n, 2000)])
    adj = graph_ref.prune(graph_ref.knn_lists(I, 16), 8)
    img = graph_ref.decode(*graph_ref.quantize(x))
    q = rng.standard_normal((8, d)).astype(np.float32)
    rescored = 0
    for metric in ("ip", "l2"):
        D0, I0, it0, sc0, _ = graph_ref.search(q, img, x, adj, 10, 64, metric)
        assert all(i > 1 for i in it0)
        for every in (1, 3):
            D1, I1, it1, sc1, _ = graph_ref.search(q, img, x, adj, 10, 64, metric, forget_every=every)
            assert np.array_equal(I0, I1) and np.array_equal(D0, D1) and it0 == it1
            assert all(a <= b for a, b in zip(sc0, sc1))
            rescored += sum(b - a for a, b in zip(sc0, sc1))
    assert rescored > 0  # forgotten ids did come back (and were dropped again)


def test_graph_trailer_round_trip_and_ivf_reader_skips_it():
    from vector_store.vector_index import read_graph_trailer, read_ivf_trailer, write_graph_trailer, write_ivf_trailer
    adj = np.array([[1, 2, -1, -1], [0, 2, -1, -1], [0, 1, -1, -1]], dtype=np.int32)
    f = io.BytesIO()
    write_graph_trailer(f, adj)
    raw = f.getvalue()
    assert raw[:8] == b"ANRGRPH1" and struct.unpack("<qi", raw[8:20]) == (3, 4) and len(raw) == 20 + 4 * 12
    f.seek(0)
    assert np.array_equal(read_graph_trailer(f, 3), adj)
    f.seek(0)
    assert read_ivf_trailer(f, 4) is None      # an IVF loader meets a graph trailer: no centroids, no error
    assert read_graph_trailer(io.BytesIO(b""), 3) is None
    g = io.BytesIO()
    write_ivf_trailer(g, np.zeros((2, 4), np.float32))
    g.seek(0)
    assert read_graph_trailer(g, 3) is None    # a graph loader ignores another trailer
    g.seek(0)
    assert read_ivf_trailer(g, 4).shape == (2, 4)
    f.seek(0)
    try:
        read_graph_trailer(f, 5)
    except ValueError:
        pass
    else:
        raise AssertionError("a trailer of another row count must be refused")
