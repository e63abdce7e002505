"""GPU tests of the related-notes pass (anr_index_related_notes, anorag_hip.related_notes): the device equals the
reference's own output (tests/golden/related_notes_cases.json) and the brute-force restatement (tests/related_ref.py) at
the smallest shapes that reach every edge of the 32-row tile and the 256-row block pair: n in {1, 2, 31, 33, 255, 257, 300}
(off-diagonal block pairs from 257, a partial last block at 300), d in {8, 40, 96} (padding of the f16 image)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import related_ref as ref

pytestmark = pytest.mark.gpu
CASES = ref.load_cases()
IDS = [c["name"] for c in CASES]
SHAPES = [(n, d) for n in (1, 2, 31, 33, 255, 257, 300) for d in (8, 40, 96)]
KW = {"threshold": "threshold", "w": "entity_weight", "min_shared": "min_shared", "exclude_same_cluster": "exclude_same_cluster",
      "bonus": "cluster_bonus", "M": "max_related"}
ARRAYS = ("nbr", "n_nbr", "combined", "base", "inter", "uni")


def device_run(emb, ents, clusters, p):
    """(result of related_pairs with stats, the index's stored rows)"""
    from anorag_hip import METRIC_IP, FlatIndex, related_pairs
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    index = FlatIndex(emb.shape[1], METRIC_IP, normalize=True)
    try:
        if len(emb):
            index.add(emb)
        x = index.reconstruct_n(0, len(emb))
        res = related_pairs(index, ents, clusters, return_stats=True, **{KW[k]: v for k, v in p.items()})
    finally:
        index.close()
    return res, x


def stored(emb):
    """the rows a cosine index stores, read back from the device (a copy: nothing of the pass under test runs)"""
    from anorag_hip import METRIC_IP, FlatIndex
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    index = FlatIndex(emb.shape[1], METRIC_IP, normalize=True)
    try:
        index.add(emb)
        return index.reconstruct_n(0, len(emb))
    finally:
        index.close()


def assert_same_lists(res, rel):
    assert res["n_nbr"].tolist() == [len(r) for r in rel]
    for i, row in enumerate(rel):
        assert res["nbr"][i, :len(row)].tolist() == [e[0] for e in row], i
        assert (res["nbr"][i, len(row):] == -1).all()
        assert res["inter"][i, :len(row)].tolist() == [e[4] for e in row] and res["uni"][i, :len(row)].tolist() == [e[5] for e in row]


def assert_values(res, base, ents, clusters, p, d):
    """every base within 2 (d + 8) 2^-53 of the correctly rounded dot product (eight partial sums of d / 8 exact products and
    three joining additions, on products whose absolute sum is at most 1); combined bit-equal to the host's expression"""
    bound = 2 * (d + 8) * ref.U
    lens = [len(set(e)) for e in ents]
    for i in range(len(base)):
        for t in range(int(res["n_nbr"][i])):
            j = int(res["nbr"][i, t])
            b = float(res["base"][i, t])
            assert abs(b - base[i, j]) <= bound, (i, j, b, base[i, j])
            ent = ref.ent_sim(int(res["inter"][i, t]), int(res["uni"][i, t]), lens[i], lens[j], p["min_shared"])
            assert ref.combine(b, ent, clusters[i], clusters[j], p) == float(res["combined"][i, t]), (i, j)


@functools.lru_cache(maxsize=None)
def shape_input(n, d):
    emb, ents, clusters = ref.clustered(n, d, seed=1000 * n + d)
    return emb, ents, clusters


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_goldens(case):
    from anorag_hip import NoteSimilarityCalculator
    notes, config, emb = case["notes"], case["config"], case["embeddings"]
    valid = ref.valid_positions(notes, config)
    full = np.zeros((len(notes), case["dim"]), np.float32)
    full[valid] = emb
    calc = NoteSimilarityCalculator(dict(config))
    out = calc.find_related_notes([dict(n) for n in notes], embeddings=full)
    ref.same_related(out, case["expected"])
    assert calc.last_stats["kept"] * 2 >= sum(len(n["related_notes"]) for n in out) > 0
    # the device base against the exact cosine: within twice what the reference's own float32 cosine deviates
    vn = [notes[k] for k in valid]
    res, _ = device_run(emb, [n.get('entities', []) for n in vn], [n.get('cluster_id', -1) for n in vn],
                        ref.params_of_config(config))
    exact = ref.exact_cosine(emb)
    worst = max((abs(float(res["base"][i, t]) - exact[i, int(res["nbr"][i, t])])
                 for i in range(len(vn)) for t in range(int(res["n_nbr"][i]))), default=0.0)
    print(f"{case['name']}: device base vs exact cosine {worst:.3g}, reference {case['base_dev']:.3g}")
    assert worst <= 2 * case["base_dev"]


@pytest.mark.parametrize("n,d", SHAPES)
def test_decisions_and_values_at_every_tile_edge(n, d):
    emb, ents, clusters = shape_input(n, d)
    base = ref.base_matrix(stored(emb))
    for p in (ref.params(threshold=0.7), ref.params(threshold=0.8, exclude_same_cluster=False, min_shared=2, w=0.2)):
        m = ref.margins(base, ents, clusters, p)
        print(f"n={n} d={d} margins={m}")
        assert min(m["threshold"], m["order"], m["bonus"]) > 2 * (d + 8) * ref.U      # asserted before the device is asked
        rel = ref.related(base, ents, clusters, p)
        res, _ = device_run(emb, ents, clusters, p)
        assert_same_lists(res, rel)
        assert_values(res, base, ents, clusters, p, d)
        if n >= 31:
            assert sum(len(r) for r in rel) > 0
        st = res["stats"]
        assert st["kept"] * 2 >= int(res["n_nbr"].sum()) and st["scored"] >= st["kept"] and st["strips"] == 1


def test_exact_ties_come_in_column_order():
    rng = np.random.default_rng(5)
    n, d = 40, 8
    emb = rng.standard_normal((n, d)).astype(np.float32)
    centre = rng.standard_normal(d)
    emb[3] = centre + 0.1 * rng.standard_normal(d)
    dup = [30, 7, 22, 11, 35]
    emb[dup] = (centre + 0.1 * rng.standard_normal(d)).astype(np.float32)
    ents = [["a", "b"] if k in dup or k == 3 else [f"x{k}"] for k in range(n)]
    clusters = [-1] * n
    p = ref.params(threshold=0.7, M=4)
    base = ref.base_matrix(stored(emb))
    res, x = device_run(emb, ents, clusters, p)
    assert all(np.array_equal(x[k], x[dup[0]]) for k in dup)
    assert res["nbr"][3].tolist() == sorted(dup)[:4]
    assert len({float(c).hex() for c in res["combined"][3]}) == 1 and len({float(b).hex() for b in res["base"][3]}) == 1
    rel = ref.related(base, ents, clusters, p)
    assert ref.margins(base, ents, clusters, p)["order"] == 0.0       # the restatement sees the ties too
    assert_same_lists(res, rel)
    # a duplicate's own list: the other duplicates (combined exactly equal among them) in column order
    row = res["nbr"][7, :int(res["n_nbr"][7])].tolist()
    assert row == [e[0] for e in rel[7]] and set(row[:4]) <= set(dup) | {3}


def test_threshold_is_strict():
    n, d = 255, 40                                      # M = 64 holds every row whole: no entry moves up when one leaves
    emb, ents, clusters = shape_input(n, d)
    p0 = ref.params(threshold=0.7, M=64)
    res0, _ = device_run(emb, ents, clusters, p0)
    rows = [i for i in range(n) if res0["n_nbr"][i] >= 2]
    i = rows[0]
    j, c = int(res0["nbr"][i, 1]), float(res0["combined"][i, 1])
    at, _ = device_run(emb, ents, clusters, ref.params(threshold=c, M=64))
    below, _ = device_run(emb, ents, clusters, ref.params(threshold=math.nextafter(c, -math.inf), M=64))

    def lists(res):
        return {(a, int(res["nbr"][a, t])): float(res["combined"][a, t]) for a in range(n) for t in range(int(res["n_nbr"][a]))}
    la, lb = lists(at), lists(below)
    assert (i, j) not in la and (j, i) not in la and lb[(i, j)] == c == lb[(j, i)]
    gone = {k for k in lb if k not in la}
    assert gone == {k for k, v in lb.items() if v == c} and all(la[k] == lb[k] for k in la)
    assert all(v > c for v in la.values())


def test_band_loses_no_passing_pair():
    """cosines within 1e-6 of the smallest base that can pass, on both sides: far inside what the f16 image can tell"""
    n, d, thr = 48, 8, 0.8
    emb = np.zeros((n, d), np.float32)
    emb[0, 0] = 1.0
    deltas = np.concatenate([np.linspace(-1e-6, -1e-7, (n - 1) // 2), np.linspace(1e-7, 1e-6, n - 1 - (n - 1) // 2)])
    for k, dl in enumerate(deltas, start=1):
        c = thr + dl
        emb[k, 0], emb[k, 1 + k % 7] = c, math.sqrt(1 - c * c)     # the rows 1.. are far from each other
    ents, clusters = [[] for _ in range(n)], [-1] * n
    p = ref.params(threshold=thr, w=0.0, M=64)
    base = ref.base_matrix(stored(emb))
    near = base[0, 1:]
    assert (np.abs(near - thr) < 2e-6).all() and (near > thr).sum() >= 5 and (near < thr).sum() >= 5
    assert ref.margins(base, ents, clusters, p)["threshold"] > 2 * (d + 8) * ref.U
    res, _ = device_run(emb, ents, clusters, p)
    assert_same_lists(res, ref.related(base, ents, clusters, p))
    assert int(res["n_nbr"][0]) == int((near > thr).sum())
    assert res["stats"]["band_resolved"] >= n - 1 and res["stats"]["nominated"] >= n - 1


@pytest.mark.parametrize("which", ["entity_weight_1", "threshold_minus_1"])
def test_degenerate_weights_make_every_pair_a_candidate(which):
    n, d = 70, 8
    emb, ents, clusters = ref.clustered(n, d, seed=77)
    ents = [e + [99] for e in ents]                     # one shared entity: every ent is at least 0.1 + 1 / uni
    p = ref.params(w=1.0, threshold=0.05, exclude_same_cluster=False) if which == "entity_weight_1" else \
        ref.params(threshold=-1.0, exclude_same_cluster=False)
    base = ref.base_matrix(stored(emb))
    res, _ = device_run(emb, ents, clusters, p)
    assert res["stats"]["nominated"] == n * (n - 1) // 2 == res["stats"]["kept"]
    assert (res["n_nbr"] == p["M"]).all()
    assert_same_lists(res, ref.related(base, ents, clusters, p))
    assert_values(res, base, ents, clusters, p, d)


def test_capacity_independence_and_determinism():
    from anorag_hip.related_notes import set_pair_capacity
    n, d = 300, 8
    emb, ents, clusters = shape_input(n, d)
    p = ref.params(threshold=0.6, M=5)
    a, _ = device_run(emb, ents, clusters, p)
    b, _ = device_run(emb, ents, clusters, p)
    set_pair_capacity(64)
    try:
        c, _ = device_run(emb, ents, clusters, p)
    finally:
        set_pair_capacity(0)
    for k in ARRAYS:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
    assert a["stats"]["strips"] == 1 and c["stats"]["strips"] > 1 and c["stats"]["pair_capacity"] == n
    assert c["stats"]["kept"] == a["stats"]["kept"] > 0 and c["stats"]["scored"] == a["stats"]["scored"]
    assert a["stats"] == b["stats"]


@pytest.mark.parametrize("M", [1, 5, 64])
def test_max_related(M):
    n, d = 257, 8
    emb, ents, clusters = shape_input(n, d)
    p = ref.params(threshold=0.5, M=M)
    base = ref.base_matrix(stored(emb))
    rel = ref.related(base, ents, clusters, p)
    res, _ = device_run(emb, ents, clusters, p)
    assert_same_lists(res, rel)
    assert max(len(r) for r in rel) == M or M == 64


def test_limits_are_refused():
    from anorag_hip import METRIC_IP, METRIC_L2, AnoragError, FlatIndex, _lib, related_pairs
    x = np.random.default_rng(0).standard_normal((10, 8)).astype(np.float32)
    ents = [[] for _ in range(10)]
    for metric, norm in ((METRIC_L2, False), (METRIC_IP, False)):
        idx = FlatIndex(8, metric, normalize=norm)
        idx.add(x)
        with pytest.raises(AnoragError, match=r"code -1"):
            related_pairs(idx, ents, None)
        idx.close()
    idx = FlatIndex(8, METRIC_IP, normalize=True)
    out = related_pairs(idx, [], None, return_stats=True)             # an empty index: an empty result
    assert out["nbr"].shape == (0, 5) and out["n_nbr"].shape == (0,) and out["stats"]["strips"] == 0
    idx.add(x)
    for M in (0, 65):
        with pytest.raises(AnoragError, match=r"code -1"):
            related_pairs(idx, ents, None, max_related=M)
    with pytest.raises(AnoragError, match=r"code -1"):
        related_pairs(idx, ents, None, threshold=float("nan"))
    lib = _lib.load()
    params = _lib.RelatedParams(0.75, 0.3, 0.1, 1, 1, 5, 0)
    nbr, cnt = np.zeros(50, np.int32), np.zeros(10, np.int32)

    def raw(indptr, ids):
        indptr, ids = np.asarray(indptr, np.int64), np.asarray(ids, np.int32)
        return lib.anr_index_related_notes(idx._h, C.byref(params), None, indptr.ctypes.data, ids.ctypes.data, nbr.ctypes.data,
                                           cnt.ctypes.data, None, None, None, None, None)
    flat = [0, 2, 4] + [4] * 8
    assert raw(flat, [1, 5, 0, 3]) == 0
    assert raw(flat, [5, 1, 0, 3]) == -1 and b"ascending" in lib.anr_last_error()      # unsorted
    assert raw(flat, [1, 1, 0, 3]) == -1                                               # repeated
    assert raw(flat, [-2, 1, 0, 3]) == -1                                              # out of range
    assert raw([0, 2, 1] + [4] * 8, [1, 5, 0, 3]) == -1                                # indptr descends
    idx.close()
