"""GPU tests of the IVF-Flat index (anr_ivf_*, anorag_hip.IVFIndex) against tests/ivf_ref.py and the exact FlatIndex."""
import numpy as np
import pytest

import ivf_ref
from oracle import flat_index as orc

pytestmark = pytest.mark.gpu

METRICS = [("ip", False), ("cos", True), ("l2", False)]


def _mk(d, nlist, metric, normalize):
    from anorag_hip import IVFIndex, METRIC_IP, METRIC_L2
    return IVFIndex(d, nlist, METRIC_L2 if metric == "l2" else METRIC_IP, normalize=normalize)


def _prep(x, normalize):
    # the device's normalisation (divide by the float32 of the float64 norm), so that near-identical rows keep their order
    return ivf_ref.normalize_rows(np.asarray(x, np.float32)) if normalize else np.ascontiguousarray(x, dtype=np.float32)


def _m(metric):
    return "l2" if metric == "l2" else "ip"


def _rank_scores(q, x, metric):
    s = orc.exact_scores(q, x, _m(metric))
    return -s if metric == "l2" else s  # larger is better for near_tie_equal


@pytest.mark.parametrize("metric,normalize", METRICS)
def test_all_lists_probed_equals_the_flat_index(metric, normalize):
    from anorag_hip import FlatIndex, METRIC_IP, METRIC_L2
    rng = np.random.default_rng(11)
    d, n, nlist = 96, 20_000, 64
    x = rng.standard_normal((n, d), dtype=np.float32)
    ivf = _mk(d, nlist, metric, normalize)
    ivf.train(x, niter=8, seed=5)
    ivf.add(x)
    flat = FlatIndex(d, METRIC_L2 if metric == "l2" else METRIC_IP, normalize=normalize)
    flat.add(x)
    assert ivf.ntotal == n and int(ivf.list_sizes().sum()) == n
    qa = rng.standard_normal((200, d), dtype=np.float32)
    for nq in (1, 7, 64, 200):
        q = qa[:nq]
        s = _rank_scores(_prep(q, normalize), _prep(x, normalize), metric)
        for k in (1, 10, 100):
            D, I = ivf.search(q, k, nprobe=nlist)
            Df, If = flat.search(q, k)
            assert orc.near_tie_equal(I, If, s, k, 1e-6), (nq, k)
            assert float(np.max(np.abs(D - Df))) <= 1e-4, (nq, k)
    ivf.close()
    flat.close()


def _probed_case(x, q, metric, normalize, nlist, nprobe, ks, seed):
    rng = np.random.default_rng(seed)
    xp, qp = _prep(x, normalize), _prep(q, normalize)
    cent = xp[rng.choice(len(x), nlist, replace=False)].copy()
    ivf = _mk(x.shape[1], nlist, metric, normalize)
    ivf.set_centroids(cent)
    ivf.add(x)
    lists = ivf_ref.assign(xp, cent, _m(metric))
    assert np.array_equal(ivf.list_sizes(), np.bincount(lists, minlength=nlist))
    ids = np.arange(len(x), dtype=np.int64)
    ok = ivf_ref.probe_margin(qp, cent, nprobe, _m(metric)) > 1e-5
    skipped = int((~ok).sum())
    assert skipped <= len(q) // 4
    s = _rank_scores(qp, xp, metric)
    P = ivf_ref.probed(qp, cent, nprobe, _m(metric))
    for k in ks:
        D, I = ivf.search(q, k, nprobe=nprobe)
        Dr, Ir = ivf_ref.search(qp, xp, ids, lists, cent, k, nprobe, _m(metric))
        for i in np.flatnonzero(ok):
            si = np.where(np.isin(lists, P[i]), s[i], -np.inf)[None, :]
            assert orc.near_tie_equal(I[i:i + 1], Ir[i:i + 1], si, k, 1e-6), (k, i)
            assert np.array_equal(I[i] < 0, Ir[i] < 0), (k, i)
            assert float(np.max(np.abs(D[i] - Dr[i]))) <= 1e-4, (k, i)
    ivf.close()
    return skipped


@pytest.mark.parametrize("metric,normalize", METRICS)
def test_probed_lists_gaussian_and_clustered(metric, normalize, record_property):
    rng = np.random.default_rng(21)
    d = 64
    x = rng.standard_normal((12_000, d), dtype=np.float32)
    q = rng.standard_normal((64, d), dtype=np.float32)
    skipped = _probed_case(x, q, metric, normalize, 48, 5, (1, 10, 100), 1)
    centres = rng.standard_normal((1024, d), dtype=np.float32)
    xc = centres[rng.integers(0, 1024, 12_000)] + 0.3 * rng.standard_normal((12_000, d), dtype=np.float32)
    qc = centres[rng.integers(0, 1024, 200)] + 0.3 * rng.standard_normal((200, d), dtype=np.float32)
    skipped_c = _probed_case(xc, qc, metric, normalize, 64, 3, (10, 100), 2)
    # queries whose nprobe-th and (nprobe+1)-th centroid keys are within 1e-5 are not compared: counted here
    record_property("near_tie_queries_skipped", f"gaussian {skipped}/64, clustered {skipped_c}/200")
    print(f"near-tie queries skipped: gaussian {skipped}/64, clustered {skipped_c}/200")


def test_lists_shorter_than_k_pad_with_minus_one():
    rng = np.random.default_rng(31)
    x = rng.standard_normal((640, 32), dtype=np.float32)
    q = rng.standard_normal((7, 32), dtype=np.float32)
    for metric, normalize in METRICS:
        _probed_case(x, q, metric, normalize, 64, 1, (100,), 3)
    ivf = _mk(32, 64, "l2", False)
    ivf.set_centroids(x[:64])
    ivf.add(x)
    D, I = ivf.search(q, 100, nprobe=1)
    assert (I == -1).any() and np.all(D[I == -1] == np.finfo(np.float32).max)


def _planted(groups, per, d, sep, sigma, seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((groups, d)).astype(np.float32)
    centres *= sep / np.linalg.norm(centres, axis=1, keepdims=True)
    x = np.repeat(centres, per, axis=0) + sigma * rng.standard_normal((groups * per, d), dtype=np.float32)
    return x.astype(np.float32), np.repeat(np.arange(groups), per)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_training_is_deterministic_and_matches_lloyd(metric):
    rng = np.random.default_rng(41)
    d, n, nlist = 32, 5000, 40
    x = rng.standard_normal((n, d), dtype=np.float32)
    a, b = _mk(d, nlist, metric, False), _mk(d, nlist, metric, False)
    a.train(x, niter=10, seed=7)
    b.train(x, niter=10, seed=7)
    ca, cb = a.centroids, b.centroids
    assert ca.tobytes() == cb.tobytes()
    # each row's list is the best centroid (within 1e-5)
    a.add(x)
    kk = ivf_ref.keys(x, ca, metric)
    best = kk.max(axis=1)
    got = a.assignments(np.arange(n)).astype(np.int64)
    assert np.all(kk[np.arange(n), got] >= best - 1e-5)  # row by row
    assert np.array_equal(a.list_sizes(), np.bincount(got, minlength=nlist))
    # from given centroids the device runs the same Lloyd iterations as the restatement, and each centroid is the f64
    # mean of its rows
    init = x[rng.choice(n, nlist, replace=False)].copy()
    c = _mk(d, nlist, metric, False)
    c.set_centroids(init)
    c.train_from(x, 6)
    ref = ivf_ref.lloyd(x, init, 6, metric)
    assert float(np.max(np.abs(c.centroids - ref))) <= 1e-5
    c5 = ivf_ref.lloyd(x, init, 5, metric)
    last = ivf_ref.assign(x, c5, metric)
    for l in range(nlist):
        if (last == l).any():
            assert np.allclose(c.centroids[l], x[last == l].astype(np.float64).mean(0), atol=1e-5)
    # spherical k-means (what the facade uses for inner product): normalised means
    if metric == "ip":
        sp = _mk(d, nlist, metric, False)
        sp.set_spherical(True)
        sp.set_centroids(init)
        sp.train_from(x, 6)
        ref = ivf_ref.lloyd(x, init, 6, metric, spherical=True)
        assert float(np.max(np.abs(sp.centroids - ref))) <= 1e-5
        assert np.allclose(np.linalg.norm(sp.centroids.astype(np.float64), axis=1), 1.0, atol=1e-6)
        sp.close()
    for h in (a, b, c):
        h.close()


def test_planted_partition_and_empty_list_split():
    x, g = _planted(8, 50, 32, 10.0, 0.1, 51)
    ivf = _mk(32, 8, "l2", False)
    ivf.set_centroids(x[::50] + 0.05)
    ivf.train_from(x, 5)
    ivf.add(x)
    assert ivf.list_sizes().tolist() == [50] * 8
    for grp in range(8):
        _, I = ivf.search(x[grp * 50:grp * 50 + 1], 50, nprobe=1)
        assert sorted(I[0].tolist()) == list(range(grp * 50, grp * 50 + 50))
    ivf.close()
    # one centroid far from every row: its list is empty after the first assignment and takes half of the largest
    x4, _ = _planted(4, 50, 16, 10.0, 0.1, 52)
    init = np.stack([x4[0], x4[50], x4[100], np.full(16, 1000.0, np.float32)])
    ivf = _mk(16, 4, "l2", False)
    ivf.set_centroids(init)
    ivf.train_from(x4, 4)
    ref = ivf_ref.lloyd(x4, init, 4, "l2")
    assert float(np.max(np.abs(ivf.centroids - ref))) <= 1e-5
    ivf.add(x4)
    sizes = ivf.list_sizes()
    assert (sizes > 0).all() and sizes.sum() == 200
    ivf.close()


def test_chunked_add_and_remove_ids():
    rng = np.random.default_rng(61)
    d, n, nlist = 48, 9000, 32
    x = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((64, d), dtype=np.float32)
    one = _mk(d, nlist, "ip", True)
    one.train(x, niter=5, seed=3)
    cent = one.centroids
    one.add(x)
    three = _mk(d, nlist, "ip", True)
    three.set_centroids(cent)
    for s in (0, 2000, 6500):
        three.add(x[s:{0: 2000, 2000: 6500, 6500: n}[s]])
    for k, nprobe in ((10, 4), (100, 9)):
        D1, I1 = one.search(q, k, nprobe=nprobe)
        D3, I3 = three.search(q, k, nprobe=nprobe)
        assert np.array_equal(I1, I3) and np.array_equal(D1, D3)
    assert np.array_equal(one.reconstruct([5, 8999]), three.reconstruct([5, 8999]))
    gone = rng.choice(n, 3000, replace=False)
    assert three.remove_ids(gone) == 3000 and three.ntotal == n - 3000
    assert np.array_equal(three.centroids, cent)
    keep = np.setdiff1d(np.arange(n), gone)
    xp, qp = orc.preprocess_vectors(x), orc.preprocess_vectors(q)
    lists = ivf_ref.assign(xp[keep], cent, "ip")
    ok = ivf_ref.probe_margin(qp, cent, 6, "ip") > 1e-5
    D, I = three.search(q, 50, nprobe=6)
    Dr, Ir = ivf_ref.search(qp, xp[keep], keep.astype(np.int64), lists, cent, 50, 6, "ip")
    assert np.array_equal(I[ok], Ir[ok]) and float(np.max(np.abs(D[ok] - Dr[ok]))) <= 1e-4
    with pytest.raises(Exception):
        three.reconstruct([int(gone[0])])
    one.close()
    three.close()


@pytest.fixture
def cfg(tmp_path):
    from anorag_hip.compat import config
    config.reset()
    config.set("storage.vector_index_path", str(tmp_path / "vidx"))
    config.set("vector_store.index_type", "IVFFlat")
    config.set("vector_store.nlist", 20)
    config.set("vector_store.nprobe", 10)
    yield config
    config.reset()


def test_facade_ivf_save_load_and_nprobe_sweep(cfg):
    from anorag_hip import FlatIndex, IVFIndex
    from vector_store import VectorIndex
    rng = np.random.default_rng(71)
    x = rng.standard_normal((4000, 64), dtype=np.float32)
    q = rng.standard_normal((16, 64), dtype=np.float32)
    plain = VectorIndex(64)
    assert plain.create_index() and isinstance(plain.index, FlatIndex)  # the key is off by default
    plain.cleanup()
    cfg.set("anorag_hip.ivf", True)
    vi = VectorIndex(64)
    assert vi.create_index() and isinstance(vi.index, IVFIndex)
    assert vi.add_vectors(x) and vi.is_trained and vi.index.ntotal == 4000
    assert vi.remove_vectors(np.array([3, 7, 11]))
    before = vi.search(q, top_k=10)
    assert all(h["index"] not in (3, 7, 11) for hits in before for h in hits)
    path = vi.save_index()
    assert path
    vi2 = VectorIndex(64)
    assert vi2.load_index(path.split("/")[-1]) and isinstance(vi2.index, IVFIndex)
    assert np.array_equal(vi2.index.centroids, vi.index.centroids)
    assert vi2.search(q, top_k=10) == before
    st = vi2.get_index_stats()
    assert {"nlist", "nprobe", "ntotal"} <= set(st) and st["ntotal"] == 3997
    cfg.set("anorag_hip.ivf", False)
    vi3 = VectorIndex(64)
    assert vi3.load_index(path.split("/")[-1]) and isinstance(vi3.index, FlatIndex) and vi3.index.ntotal == 3997
    # nprobe sweep: recall grows with nprobe and is 1.0 when every list is probed
    xp = orc.preprocess_vectors(x)
    keep = np.setdiff1d(np.arange(4000), [3, 7, 11])
    _, Ir = orc.flat_search(orc.preprocess_vectors(q), xp[keep], 10, "ip")
    truth = keep[Ir]
    recalls = []
    for nprobe in (1, 5, 10, 20):
        vi.nprobe = nprobe
        recalls.append(vi._calculate_recall(vi.search(q, top_k=10), truth))
    assert recalls == sorted(recalls) and recalls[-1] == 1.0 and recalls[0] < 1.0
    best = vi.optimize_search_params(q, truth, target_recall=1.0)
    assert best["recall"] == 1.0 and vi.nprobe == best["nprobe"] <= 20
    for v in (vi, vi2, vi3):
        v.cleanup()


def _check_against_ref(ivf, q, xp, qp, cent, metric, k, nprobe, ids=None):
    ids = np.arange(len(xp), dtype=np.int64) if ids is None else ids
    lists = ivf_ref.assign(xp, cent, _m(metric))
    D, I = ivf.search(q, k, nprobe=nprobe)
    Dr, Ir = ivf_ref.search(qp, xp, ids, lists, cent, k, nprobe, _m(metric))
    assert np.array_equal(I, Ir)
    assert float(np.max(np.abs(D - Dr) / np.maximum(1.0, np.abs(Dr)))) <= 1e-5
    return ivf.last_search_stats()


@pytest.mark.parametrize("metric,normalize", METRICS)
def test_certificate_failures_take_the_exact_rescan(metric, normalize):
    """More identical rows at the query than K' (and than the 2048 candidates k_ivf_select can hold) make the
    certificate fail; so do thousands of near-duplicates within the f16 error of each other (several chunks of the exact
    re-scan).  The results must still be the exact top-k of the probed rows, ties by ascending id."""
    rng = np.random.default_rng(81)
    d, nlist = 64, 8
    base = rng.standard_normal((4000, d), dtype=np.float32)
    v = rng.standard_normal(d).astype(np.float32)
    dup = np.repeat(v[None, :], 3000, axis=0)
    near = v[None, :] + 1e-4 * rng.standard_normal((5000, d), dtype=np.float32)
    x = np.concatenate([base, dup, near]).astype(np.float32)
    perm = rng.permutation(len(x))
    x = x[perm]  # duplicates spread over the ids
    q = np.stack([v + 1e-3 * rng.standard_normal(d).astype(np.float32) for _ in range(7)])
    xp, qp = _prep(x, normalize), _prep(q, normalize)
    # list 0 is centred on the duplicated row, the others on rows of the Gaussian part: every duplicate is in list 0
    cent = np.concatenate([_prep(v[None, :], normalize), _prep(base[rng.choice(4000, nlist - 1, replace=False)], normalize)])
    ivf = _mk(d, nlist, metric, normalize)
    ivf.set_centroids(cent)
    ivf.add(x)
    for k in (10, 100):
        st = _check_against_ref(ivf, q, xp, qp, cent, metric, k, 2)
        assert st["n_queries"] == 7 and st["n_exact_rescan"] == 7, st
    ivf.close()
    # the query IS the duplicated row: 3000 approximate keys equal the threshold, more than k_ivf_select can hold
    x2 = np.concatenate([base, dup])[rng.permutation(7000)]
    x2p = _prep(x2, normalize)
    q2 = np.stack([v, v])
    ivf = _mk(d, nlist, metric, normalize)
    ivf.set_centroids(cent)
    ivf.add(x2)
    for k in (10, 100):
        st = _check_against_ref(ivf, q2, x2p, _prep(q2, normalize), cent, metric, k, 2)
        assert st["n_exact_rescan"] == 2, st
    ivf.close()


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_rows_beyond_the_f16_range_are_scored_exactly(metric):
    """A row of norm >= 60000 cannot be held by the f16 image: every query takes the exact re-scan, and the big row is
    still found (its f16 key is inf / NaN)."""
    rng = np.random.default_rng(91)
    d, nlist = 32, 8
    x = rng.standard_normal((3000, d), dtype=np.float32)
    x[123] = 0.0
    x[123, :4] = 70000.0  # beyond the f16 range: its f16 key overflows
    q = rng.standard_normal((7, d), dtype=np.float32)
    q[0] = np.abs(q[0]) if metric == "ip" else x[123] * 0.99
    cent = x[rng.choice(3000, nlist, replace=False)].copy()
    cent[0] = x[123]
    ivf = _mk(d, nlist, metric, False)
    ivf.set_centroids(cent)
    ivf.add(x)
    st = _check_against_ref(ivf, q, x, q, cent, metric, 10, 3)
    assert st["n_exact_rescan"] == 7
    D, I = ivf.search(q[:1], 10, nprobe=nlist)
    assert I[0, 0] == 123
    ivf.close()


def test_facade_failed_add_leaves_the_id_map_unchanged(cfg):
    from vector_store import VectorIndex
    cfg.set("anorag_hip.ivf", True)
    rng = np.random.default_rng(101)
    x = rng.standard_normal((600, 32), dtype=np.float32)
    vi = VectorIndex(32)
    assert vi.create_index()
    assert vi.add_vectors(x[:300], ids=np.arange(1000, 1300))
    assert not vi.add_vectors(rng.standard_normal((50, 16), dtype=np.float32), ids=np.arange(50))  # wrong dimension
    assert not vi.add_vectors(x[300:310], ids=np.arange(3))  # ids of the wrong length
    assert vi.add_vectors(x[300:], ids=np.arange(5000, 5300))
    assert len(vi._ids) == 600 and vi.index.ntotal == 600
    vi.nprobe = vi.nlist
    hits = vi.search(x[[5, 400]], top_k=1)
    assert hits[0][0]["index"] == 1005 and hits[1][0]["index"] == 5100
    path = vi.save_index()
    assert path
    vi2 = VectorIndex(32)
    assert vi2.load_index(path.split("/")[-1])
    vi2.nprobe = vi2.nlist
    assert vi2.search(x[[5, 400]], top_k=1) == hits
    vi.cleanup()
    vi2.cleanup()
