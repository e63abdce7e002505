"""GPU tests of the graph index (anr_index_graph_*, anorag_hip.GraphIndex) against tests/graph_ref.py, the float64 exact
top-k and the exact FlatIndex."""
import numpy as np
import pytest

import graph_ref
from oracle import flat_index as orc

pytestmark = pytest.mark.gpu

CONFIGS = [("cos", "ip", True), ("ip", "ip", False), ("l2", "l2", False)]


def _mk(metric, normalize, d, **kw):
    from anorag_hip import GraphIndex, METRIC_IP, METRIC_L2
    return GraphIndex(d, METRIC_L2 if metric == "l2" else METRIC_IP, normalize=normalize, **kw)


def _rank_scores(q, x, metric):
    s = orc.exact_scores(q, x, metric)
    return -s if metric == "l2" else s


def _clustered(rng, n, d, centres, sigma):
    c = rng.standard_normal((centres, d)).astype(np.float32)
    return (c[rng.integers(0, centres, n)] + sigma * rng.standard_normal((n, d))).astype(np.float32)


def test_knn_lists_equal_the_float64_exact_lists():
    rng = np.random.default_rng(5)
    n, d, K = 3000, 64, 32
    x = _clustered(rng, n, d, 40, 0.5)
    g = _mk("ip", True, d, keep_knn=True)
    g.add(x)
    g.build_graph(R=16, build_degree=K)
    L = g.knn_lists()
    xp = graph_ref.prepare(x, True)
    s = orc.exact_scores(xp, xp, "ip")
    _, I = orc.flat_search(xp, xp, K + 1, "ip")
    Lr = graph_ref.knn_lists(I, K)
    np.fill_diagonal(s, np.inf)  # the own id is dropped on both sides
    same = (L == Lr).all(axis=1)
    assert same.mean() >= 0.99
    # rows that differ: only near-ties (within float32 accumulation of 64 terms) around the K-th score
    assert orc.near_tie_equal(L[~same], Lr[~same], s[~same], K + 1, 1e-5)  # K + 1: the own (inf) score counts
    st = g.graph_stats()
    assert st["builds"] == 1 and st["R"] == 16 and st["build_degree"] == K and st["has_graph"] == 1
    g.close()


@pytest.mark.parametrize("name,metric,normalize", CONFIGS)
def test_adjacency_and_search_equal_the_restatement(name, metric, normalize):
    rng = np.random.default_rng({"cos": 1, "ip": 2, "l2": 3}[name])
    n, d, K, R = 10000, 48, 24, 16   # more rows than the entry sample (4096): the beam has to walk
    x = _clustered(rng, n, d, 30, 0.6)
    if name == "ip":
        x *= rng.uniform(0.2, 2.0, (n, 1)).astype(np.float32)  # raw IP: some rows are not their own best match
    g = _mk(metric, normalize, d, keep_knn=True)
    g.add(x)
    g.build_graph(R=R, build_degree=K)
    L = g.knn_lists()
    adj = g.adjacency()
    assert adj.shape == (n, R) and adj.dtype == np.int32
    assert np.array_equal(adj, graph_ref.prune(L, R)), "device adjacency differs from the restated prune"
    # search: the restatement fed the device's graph and decoded traversal image
    img = g.traversal_image(np.arange(n))
    xp = graph_ref.prepare(x, normalize)
    c, e = graph_ref.quantize(xp)
    assert np.array_equal(img, graph_ref.decode(c, e))
    q = _clustered(rng, 100, d, 30, 0.6)
    qp = graph_ref.prepare(q, normalize)
    k, ef = 10, 40
    D, I = g.search(q, k, ef=ef)
    st = g.graph_stats()
    Dr, Ir, it, scored, capped = graph_ref.search(qp, img, xp, adj, k, ef, metric)
    # a query whose device-prepared form may differ in one code from the restated one (a value within 1e-4 of a
    # rounding boundary of the query's int8 codes) is exempt; there are few
    qe = graph_ref.quantize(qp)[1]
    frac = np.abs(np.ldexp(qp, -qe[:, None]) % 1.0 - 0.5)
    exempt = (frac < 1e-4).any(axis=1) if normalize else np.zeros(len(q), bool)
    assert exempt.mean() <= 0.05
    assert np.array_equal(I[~exempt], Ir[~exempt])
    if not exempt.any():
        assert st["last_iterations"] == sum(it) and st["last_capped"] == sum(capped)
        assert st["last_rows_scored"] >= sum(scored)
    assert st["last_nq"] == 100
    # scores are float64 re-scores of the returned rows, rounded to float32
    s = orc.exact_scores(qp, xp, metric)
    assert np.allclose(D, np.take_along_axis(s, I, axis=1).astype(np.float32), rtol=1e-6, atol=1e-6)
    g.close()


def test_recall_at_ef100_on_a_clustered_corpus():
    from anorag_hip import FlatIndex, METRIC_IP
    rng = np.random.default_rng(21)
    n, d = 20000, 256
    c = rng.standard_normal((200, d)).astype(np.float32)
    x = (c[rng.integers(0, 200, n)] + 0.35 * rng.standard_normal((n, d))).astype(np.float32)
    q = (c[rng.integers(0, 200, 200)] + 0.35 * rng.standard_normal((200, d))).astype(np.float32)
    g = _mk("ip", True, d)
    g.add(x)
    D, I = g.search(q, 10, ef=100)       # first search builds R = 64, build_degree = 128
    flat = FlatIndex(d, METRIC_IP, normalize=True)
    flat.add(x)
    _, Ix = flat.search(q, 10)
    recall = np.mean([len(set(I[i]) & set(Ix[i])) / 10 for i in range(len(q))])
    assert recall >= 0.95, recall
    st = g.graph_stats()
    assert st["builds"] == 1 and st["last_rows_scored"] < 0.5 * n * len(q)
    assert st["graph_bytes"] == n * 64 * 4 and st["image_bytes"] == n * (256 + 8)
    g.close()
    flat.close()


def test_tiny_corpus_with_ef_at_least_n_equals_flat_and_pads():
    from anorag_hip import FlatIndex, METRIC_IP
    rng = np.random.default_rng(2)
    n, d = 50, 16
    x = rng.standard_normal((n, d)).astype(np.float32)
    g = _mk("ip", True, d)
    g.add(x)
    g.build_graph(R=8, build_degree=16)
    adj = g.adjacency()
    seen, todo = {0}, [0]
    while todo:
        for v in adj[todo.pop()].tolist():
            if v >= 0 and v not in seen:
                seen.add(v)
                todo.append(v)
    assert len(seen) == n  # connected
    flat = FlatIndex(d, METRIC_IP, normalize=True)
    flat.add(x)
    q = rng.standard_normal((70, d)).astype(np.float32)   # more than 64 queries
    for k in (10, 60):                                     # 60 > ntotal: padding
        D, I = g.search(q, k, ef=64)
        Df, If = flat.search(q, k)
        assert np.array_equal(I, If)
        assert np.allclose(D[:, :n], Df[:, :n], rtol=1e-6, atol=1e-6)
        if k > n:
            assert (I[:, n:] == -1).all() and (D[:, n:] == -np.finfo(np.float32).max).all()
    g.close()
    flat.close()


def test_device_queries_and_an_add_after_a_build():
    import torch
    rng = np.random.default_rng(9)
    n, d = 4000, 32
    x = rng.standard_normal((n, d)).astype(np.float32)
    g = _mk("ip", True, d, R=16, build_degree=32)
    g.add(x)
    q = rng.standard_normal((80, d)).astype(np.float32)
    D, I = g.search(q, 10, ef=64)
    qt = torch.from_numpy(q).to("cuda:0")
    torch.cuda.synchronize()
    D2, I2 = g.search_device_queries(qt.data_ptr(), len(q), 10, ef=64)
    assert np.array_equal(I, I2) and np.array_equal(D, D2)
    assert g.graph_stats()["builds"] == 1
    new = rng.standard_normal((50, d)).astype(np.float32)
    g.add(new)
    assert g.graph_stats()["stale"] == 1
    D3, I3 = g.search(new, 1, ef=64)
    assert (I3[:, 0] == np.arange(n, n + 50)).all()      # every new row finds itself
    st = g.graph_stats()
    assert st["builds"] == 2 and st["stale"] == 0
    g.search(new, 1, ef=64)
    assert g.graph_stats()["builds"] == 2
    g.close()


def test_knn_lists_after_reset_or_add_follow_the_rows():
    from anorag_hip import AnoragError
    rng = np.random.default_rng(4)
    x = rng.standard_normal((3000, 32)).astype(np.float32)
    g = _mk("ip", True, 32, R=8, build_degree=16)
    g.add(x)
    g.build_graph()
    with pytest.raises(AnoragError):           # not kept by default: no n * build_degree host copy
        g.knn_lists()
    g.keep_knn = True
    g.build_graph()
    assert g.knn_lists().shape == (3000, 16) and g.graph_stats()["builds"] == 2
    g.reset()                                  # zero rows: the stale graph is rebuilt over nothing
    assert g.knn_lists().shape == (0, 16) and g.adjacency().shape == (0, 8)
    g.add(x[:1000])
    L = g.knn_lists()                          # rebuilt for the 1000 rows now stored
    assert L.shape == (1000, 16) and L.min() >= 0 and L.max() < 1000 and g.graph_stats()["builds"] == 4
    # the C entry points check the caller's buffer shape
    out = np.zeros((10, 16), np.int32)
    assert g._lib.anr_index_graph_knn(g._h, out.ctypes.data, 10, 16) == -1
    assert g._lib.anr_index_graph_get(g._h, out.ctypes.data, 10, 16) == -1
    assert (out == 0).all()
    D, I = g.search(x[:5], 300)                # k beyond the beam: the exact scan answers
    Dx, Ix = g.exact_search(x[:5], 300)
    assert np.array_equal(I, Ix) and (I[:, 1000:] == -1).all()
    g.close()


@pytest.fixture
def cfg(tmp_path):
    from anorag_hip.compat import config
    config.reset()
    config.set("storage.vector_index_path", str(tmp_path / "vidx"))
    config.set("vector_store.index_type", "HNSW")
    yield config
    config.reset()


def test_facade_graph_key_remove_save_and_load(cfg):
    from anorag_hip import FlatIndex, GraphIndex
    from vector_store import VectorIndex
    rng = np.random.default_rng(71)
    c = rng.standard_normal((50, 64)).astype(np.float32)
    x = (c[rng.integers(0, 50, 6000)] + 0.4 * rng.standard_normal((6000, 64))).astype(np.float32)
    q = (c[rng.integers(0, 50, 16)] + 0.4 * rng.standard_normal((16, 64))).astype(np.float32)
    plain = VectorIndex(64)
    assert plain.create_index() and isinstance(plain.index, FlatIndex) and not isinstance(plain.index, GraphIndex)
    assert plain.add_vectors(x) and "ef_search" not in plain.get_index_stats()
    exact = plain.search(q, top_k=10)
    plain.cleanup()
    cfg.set("anorag_hip.graph", True)
    vi = VectorIndex(64)
    assert vi.create_index() and isinstance(vi.index, GraphIndex)
    assert vi.add_vectors(x) and vi.get_index_stats()["ef_search"] == 100
    hits = vi.search(q, top_k=10)
    rec = np.mean([len({h["index"] for h in a} & {h["index"] for h in b}) / 10 for a, b in zip(hits, exact)])
    assert rec >= 0.95 and vi.index.graph_stats()["builds"] == 1
    assert vi.remove_vectors(np.array([3, 7, 11]))          # renumbered as the exact HNSW path does
    assert isinstance(vi.index, GraphIndex) and vi.index.ntotal == 5997
    before = vi.search(q, top_k=10)
    assert vi.index.graph_stats()["builds"] == 1             # the new handle's first build
    path = vi.save_index()
    assert path
    assert vi.index.graph_stats()["builds"] == 1            # saving a fresh graph does not build
    adj = vi.index.adjacency()
    vi2 = VectorIndex(64)
    assert vi2.load_index(path.split("/")[-1]) and isinstance(vi2.index, GraphIndex)
    assert np.array_equal(vi2.index.adjacency(), adj) and vi2.index.graph_stats()["builds"] == 0
    assert vi2.search(q, top_k=10) == before and vi2.index.graph_stats()["builds"] == 0
    cfg.set("anorag_hip.graph", False)
    vi3 = VectorIndex(64)
    assert vi3.load_index(path.split("/")[-1]) and not isinstance(vi3.index, GraphIndex) and vi3.index.ntotal == 5997
    cfg.set("anorag_hip.ivf", True)
    vi4 = VectorIndex(64)
    assert vi4.load_index(path.split("/")[-1]) and vi4.index.ntotal == 5997
    for v in (vi, vi2, vi3, vi4):
        v.cleanup()
