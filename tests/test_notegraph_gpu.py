"""GPU tests of the note graph through the C ABI (anr_notegraph_*): weighted PageRank bit-equal to the numpy
restatement (tests/notegraph_ref.py) and within the derived bound of the networkx fixture; retrieve bit-equal to what the
reference's GraphRetriever.retrieve produced, per query, batched and with the workspace forced to one slot; the cap; the
rejections; the device hand-off into anr_fuse_dense against anr_fuse_lists; a 200 k-node run of the sub-batching."""
import ctypes as C

import numpy as np
import pytest

import notegraph_ref as ref
from notegraph_cases import CASES, load_case, max_rel_diff, pagerank_bound
from test_notegraph_cpu import compare_result

pytestmark = pytest.mark.gpu
ANR_EINVAL, ANR_ENOCONV = -1, -5


def _lib():
    from anorag_hip import _lib as L
    return L, L.load()


class Handle:
    def __init__(self, n, src, dst, w):
        L, lib = _lib()
        self.L, self.lib, self.n = L, lib, int(n)
        s, d, ww = (np.ascontiguousarray(src, np.int64), np.ascontiguousarray(dst, np.int64),
                    np.ascontiguousarray(w, np.float64))
        self.h = C.c_void_p()
        self.rc = lib.anr_notegraph_create(0, self.n, len(s), s.ctypes.data, d.ctypes.data, ww.ctypes.data, C.byref(self.h))

    def ok(self):
        assert self.rc == 0, self.L.last_error()
        return self

    def pagerank(self, alpha=0.85, max_iter=100, tol=1e-6):
        out = np.full(self.n, -1.0)
        it = C.c_int32(-1)
        rc = self.lib.anr_notegraph_pagerank(self.h, alpha, max_iter, tol, out.ctypes.data, C.byref(it))
        return rc, out, it.value

    def set(self, centrality=None, importance=None):
        if centrality is not None:
            c = np.ascontiguousarray(centrality, np.float64)
            assert self.lib.anr_notegraph_set_centrality(self.h, c.ctypes.data) == 0
        if importance is not None:
            c = np.ascontiguousarray(importance, np.float64)
            assert self.lib.anr_notegraph_set_importance(self.h, c.ctypes.data) == 0

    def centrality(self):
        out = np.empty(self.n)
        assert self.lib.anr_notegraph_get_centrality(self.h, out.ctypes.data) == 0
        return out

    def max_slots(self, v):
        assert self.lib.anr_notegraph_set_option(self.h, 1, v) == 0

    @staticmethod
    def pack(seed_lists):
        offs = np.zeros(len(seed_lists) + 1, np.int64)
        offs[1:] = np.cumsum([len(s) for s in seed_lists])
        seeds = np.concatenate([np.asarray(s, np.int64) for s in seed_lists] + [np.zeros(0, np.int64)])
        return offs, np.ascontiguousarray(seeds)

    def retrieve(self, seed_lists, cutoff, cap):
        nq = len(seed_lists)
        offs, seeds = self.pack(seed_lists)
        ids = np.full((nq, cap), -7, np.int64)
        dist, score = np.zeros((nq, cap)), np.zeros((nq, cap))
        pos, cnt = np.full((nq, cap), -7, np.int32), np.full(nq, -7, np.int32)
        rc = self.lib.anr_notegraph_retrieve(self.h, nq, offs.ctypes.data, seeds.ctypes.data, cutoff, cap, ids.ctypes.data,
                                             dist.ctypes.data, score.ctypes.data, pos.ctypes.data, cnt.ctypes.data)
        assert rc == 0, self.L.last_error()
        return ids, dist, score, pos, cnt

    def close(self):
        if self.h.value:
            assert self.lib.anr_notegraph_destroy(self.h) == 0
            self.h = C.c_void_p()


def rows_of(out, q):
    ids, dist, score, pos, cnt = out
    m = min(int(cnt[q]), ids.shape[1])
    assert (ids[q, m:] == -1).all() and (pos[q, m:] == -1).all()
    assert np.isnan(dist[q, m:]).all() and np.isnan(score[q, m:]).all()
    return ids[q, :m], dist[q, :m], score[q, :m]


@pytest.mark.parametrize("name", CASES)
def test_pagerank_bit_equal_to_restatement_and_within_bound_of_networkx(name):
    c = load_case(name)
    g = Handle(c["n"], c["src"], c["dst"], c["w"]).ok()
    rc, x, iters = g.pagerank()
    assert rc == 0, g.L.last_error()
    rowptr, nbr, wt = ref.build_csr(c["n"], c["src"], c["dst"], c["w"])
    xr, itr = ref.pagerank(c["n"], rowptr, nbr, wt)
    assert iters == itr == c["iters"]
    assert x.tobytes() == xr.tobytes()
    assert g.centrality().tobytes() == x.tobytes()          # the result is the handle's centrality
    bound = pagerank_bound(c["n"], c["src"], c["dst"], iters)
    seen = max_rel_diff(x, c["centrality"])
    print(f"case {name}: max relative difference to networkx {seen:.3e}, bound {bound:.3e}")
    assert seen <= bound
    # other parameters, and a second run gives the same bits
    for alpha, tol in ((0.5, 1e-9), (0.95, 1e-8)):
        rc, x2, it2 = g.pagerank(alpha, 300, tol)
        xr2, itr2 = ref.pagerank(c["n"], rowptr, nbr, wt, alpha, 300, tol)
        assert rc == 0 and it2 == itr2 and x2.tobytes() == xr2.tobytes()
    assert g.pagerank()[1].tobytes() == x.tobytes()
    g.close()


def test_pagerank_without_convergence_has_its_own_status():
    c = load_case("B")
    g = Handle(c["n"], c["src"], c["dst"], c["w"]).ok()
    before = np.arange(c["n"], dtype=np.float64)
    g.set(centrality=before)
    rc, _, iters = g.pagerank(max_iter=1)
    assert rc == ANR_ENOCONV and rc != ANR_EINVAL and iters == 1
    assert b"converge" in g.lib.anr_last_error()
    assert np.array_equal(g.centrality(), before)           # a failed run leaves the centrality alone
    g.close()


@pytest.mark.parametrize("name", CASES)
def test_retrieve_equals_the_reference_run_per_query_batched_and_one_slot(name):
    c = load_case(name)
    g = Handle(c["n"], c["src"], c["dst"], c["w"]).ok()
    g.set(c["centrality"], c["importance"])
    lists = [s.tolist() for s in c["seed_lists"]]
    if name == "A":
        lists[1] = [x if x >= 0 else c["n"] + 5 for x in lists[1]]      # "not in the graph" from the other side too
    cap = c["n"]
    batch = g.retrieve(lists, c["khop"], cap)
    single = [g.retrieve([s], c["khop"], cap) for s in lists]
    g.max_slots(1)
    one_slot = g.retrieve(lists, c["khop"], cap)
    g.max_slots(0)
    for q, (want, ties) in enumerate(zip(c["results"], c["ties"])):
        assert batch[4][q] == len(want[0])
        compare_result(rows_of(batch, q), want, ties)
        for other in (rows_of(single[q], 0), rows_of(one_slot, q)):
            for a, b in zip(rows_of(batch, q), other):
                assert a.tobytes() == b.tobytes()
        assert single[q][4][0] == one_slot[4][q] == batch[4][q]
        assert np.array_equal(batch[3][q], one_slot[3][q])
    # seed positions: every node comes from the first seed in list order that reaches it
    rowptr, nbr, wt = ref.build_csr(c["n"], c["src"], c["dst"], c["w"])
    for q, s in enumerate(lists):
        r = ref.retrieve(c["n"], rowptr, nbr, wt, s, c["khop"], c["centrality"], c["importance"])
        assert np.array_equal(batch[3][q, :len(r[3])], r[3])
    g.close()


def test_cap_keeps_the_best_and_reports_the_full_count():
    c = load_case("A")
    g = Handle(c["n"], c["src"], c["dst"], c["w"]).ok()
    g.set(c["centrality"], c["importance"])
    lists = [s.tolist() for s in c["seed_lists"]]
    out = g.retrieve(lists, c["khop"], 100)
    for q, want in enumerate(c["results"]):
        assert out[4][q] == len(want[0])
        ids, dist, score = rows_of(out, q)
        m = min(100, len(want[0]))
        assert np.array_equal(ids, want[0][:m]) and dist.tobytes() == want[1][:m].tobytes()
        assert score.tobytes() == want[2][:m].tobytes()
    g.close()


def test_rejections_set_einval_and_a_message():
    L, lib = _lib()
    for src, dst, w, word in (([0, 2], [1, 2], [0.5, 0.5], "self-loop"), ([0, 1, 2], [1, 2, 1], [0.5, 0.5, 0.5], "more than once"),
                              ([0, 0], [1, 1], [0.5, 0.6], "more than once"), ([0], [1], [-0.5], "weight"),
                              ([0], [1], [float("nan")], "weight"), ([0], [7], [0.5], "range")):
        g = Handle(5, src, dst, w)
        assert g.rc == ANR_EINVAL and not g.h.value, (src, dst, w)
        assert word in L.last_error()
    g = Handle(5, [0, 1], [1, 2], [0.5, 0.25]).ok()
    offs, seeds = np.array([0, 1], np.int64), np.array([0], np.int64)
    ids, cnt = np.zeros(4, np.int64), np.zeros(1, np.int32)
    for cutoff, cap in ((float("nan"), 4), (-1.0, 4), (2.0, 0)):
        assert lib.anr_notegraph_retrieve(g.h, 1, offs.ctypes.data, seeds.ctypes.data, cutoff, cap, ids.ctypes.data, None,
                                          None, None, cnt.ctypes.data) == ANR_EINVAL
    # optional outputs may be NULL; zero-weight edges are legal; node 3 and 4 are isolated
    assert lib.anr_notegraph_retrieve(g.h, 1, offs.ctypes.data, seeds.ctypes.data, 2.0, 4, ids.ctypes.data, None, None, None,
                                      cnt.ctypes.data) == 0
    assert cnt[0] == 2 and sorted(ids[:2].tolist()) == [1, 2] and (ids[2:] == -1).all()
    g.close()


def test_device_rows_fuse_as_the_graph_source_like_the_lists():
    """anr_notegraph_retrieve_dev -> anr_notegraph_rows_to_array_dev -> anr_fuse_dense (linear, with a dense short list)
    equals anr_fuse_lists on the equivalent lists bit for bit — including a note the expansion did not reach staying ABSENT
    from `graph` (NaN in out_src, no candidate) instead of present with 0.0"""
    from anorag_hip.fusion import DeviceArray, SparseRows, fuse_dense
    L, lib = _lib()
    c = load_case("A")
    n = c["n"]
    g = Handle(n, c["src"], c["dst"], c["w"]).ok()
    g.set(c["centrality"], c["importance"])
    lists = [s.tolist() for s in c["seed_lists"]]
    nq, cap, pool = len(lists), 4096, 100
    host = g.retrieve(lists, c["khop"], cap)
    offs, seeds = g.pack(lists)
    rows = SparseRows(nq, n, cap)
    found = np.zeros(nq, np.int32)
    assert lib.anr_notegraph_retrieve_dev(g.h, nq, offs.ctypes.data, seeds.ctypes.data, c["khop"], cap, C.c_void_p(rows.ids_ptr),
                                          C.c_void_p(rows.scores_ptr), C.c_void_p(rows.count_ptr), found.ctypes.data) == 0
    assert np.array_equal(found, host[4])
    back = rows.numpy()
    for q in range(nq):                                   # rows ascending by id, the same (id, score) pairs
        ids, _, score = rows_of(host, q)
        order = np.argsort(ids)
        assert np.array_equal(back[q][0], ids[order]) and back[q][1].tobytes() == score[order].tobytes()
    arr = DeviceArray(nq, n)
    assert lib.anr_notegraph_rows_to_array_dev(g.h, nq, cap, C.c_void_p(rows.ids_ptr), C.c_void_p(rows.scores_ptr),
                                               C.c_void_p(rows.count_ptr), C.c_void_p(arr.ptr)) == 0
    a = arr.numpy()
    for q in range(nq):
        assert np.isnan(a[q]).sum() == n - found[q]
    rng = np.random.default_rng(5)
    dense = []
    for q in range(nq):
        ids = rows_of(host, q)[0]
        pick = list(rng.choice(ids, size=min(30, len(ids)), replace=False)) + list(rng.integers(0, n, 40))
        pick = list(dict.fromkeys(int(x) for x in pick))[:60]
        dense.append((np.asarray(pick, np.int64), np.sort(rng.random(len(pick)))[::-1].copy()))
    w = {"dense": 1.0, "bm25": 0.5, "graph": 0.5, "path": 0.1}
    got = fuse_dense("linear", w, 60.0, pool, nq, {"dense": dense, "graph": arr})
    # the same through anr_fuse_lists: per query dense, bm25 (none), graph (best first), path (none)
    all_ids, all_sc, o5 = [], [], np.zeros((nq, 5), np.int64)
    for q in range(nq):
        gi, _, gs = rows_of(host, q)
        o5[q, 0] = len(all_ids)
        all_ids += dense[q][0].tolist(); all_sc += dense[q][1].tolist()
        o5[q, 1] = o5[q, 2] = len(all_ids)
        all_ids += gi.tolist(); all_sc += gs.tolist()
        o5[q, 3] = o5[q, 4] = len(all_ids)
    ids64, sc64 = np.asarray(all_ids, np.int64), np.asarray(all_sc, np.float64)
    wv = np.asarray([w[k] for k in ("dense", "bm25", "graph", "path")])
    e_ids, e_fin = np.empty((nq, pool), np.int64), np.empty((nq, pool))
    e_src, e_cnt = np.empty((nq, pool, 4)), np.empty(nq, np.int32)
    assert lib.anr_fuse_lists(0, 0, nq, ids64.ctypes.data, sc64.ctypes.data, o5.ctypes.data, wv.ctypes.data, 60.0, pool,
                              e_ids.ctypes.data, e_fin.ctypes.data, e_src.ctypes.data, e_cnt.ctypes.data) == 0, L.last_error()
    assert np.array_equal(got[3], e_cnt)
    assert (e_cnt[[2, 4, 6]] == [len(d[0]) for d in (dense[2], dense[4], dense[6])]).all()   # no graph result: only the dense ids
    absent_seen = False
    for q in range(nq):
        m = e_cnt[q]
        assert np.array_equal(got[0][q, :m], e_ids[q, :m])
        assert got[1][q, :m].tobytes() == e_fin[q, :m].tobytes()
        assert np.array_equal(got[2][q, :m], e_src[q, :m], equal_nan=True)
        absent_seen |= bool(found[q] > 0 and np.isnan(e_src[q, :m, 2]).any())
    assert absent_seen                                    # a candidate of a query with graph results is absent from `graph`
    arr.free()
    rows.free()
    g.close()


def test_200k_nodes_64_queries_of_20_seeds_run_and_match_the_restatement():
    """a size check of the sub-batching (1280 searches of a graph whose every search reaches most of the 200 k nodes), not
    a timing: 4 sampled queries are compared with the restatement, the rest must be well-formed"""
    rng = np.random.default_rng(20)
    n, E = 200_000, 1_600_000
    a, b = rng.integers(0, n, 2 * E), rng.integers(0, n, 2 * E)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique((lo * n + hi)[lo != hi])[:E]
    key = key[rng.permutation(len(key))]
    src, dst = key // n, key % n
    w = rng.uniform(0.35, 0.85, len(key))
    g = Handle(n, src, dst, w).ok()
    rc, cent, _ = g.pagerank()
    assert rc == 0
    imp = rng.uniform(0.5, 2.0, n)
    g.set(importance=imp)
    lists = [rng.integers(0, n, 20).tolist() for _ in range(64)]
    cap = 2048
    out = g.retrieve(lists, 2.0, cap)
    assert (out[4] > cap).all() and (out[4] <= n).all()
    assert (np.diff(out[2], axis=1) <= 0).all() and (out[0] >= 0).all() and (out[0] < n).all()
    rowptr, nbr, wt = ref.build_csr(n, src, dst, w)
    for q in (0, 21, 42, 63):
        ids, dist, score, pos = ref.retrieve(n, rowptr, nbr, wt, lists[q], 2.0, cent, imp)
        assert out[4][q] == len(ids)
        assert np.array_equal(out[0][q], ids[:cap]) and out[1][q].tobytes() == dist[:cap].tobytes()
        assert out[2][q].tobytes() == score[:cap].tobytes() and np.array_equal(out[3][q], pos[:cap])
    g.close()
