"""GPU tests of the IVF-PQ mode of anr_ivf (anr_ivf_create_pq, anorag_hip.IVFIndex(pq_m=...)) against
tests/ivfpq_ref.py, and of the VectorIndex facade's IVFPQ type with anorag_hip.ivf + anorag_hip.ivf_pq.

Error bound of the ADC keys (ivfpq_ref.key_bounds).  Let u = 2^-24 and g = (dsub + m + 2) u / (1 - (dsub + m + 2) u).
  IP: each LUT entry is a float32 sum of dsub products (error <= gamma_dsub sum_d |q_d||cb_d|), the m entries are
      summed in float32 (error <= gamma_m sum_j |LUT_j|), and the float64 coarse score q.c plus that sum is rounded once
      to float32 (u |key|).  So |key - exact| <= g sum_d |q_d||cb_d| + u |key|.
  L2: a = fl(q - c) and e = fl(a - cb) differ from v = q - c - cb by at most eta = u (1.01 |q - c| + |v|) per value;
      e^2 - v^2 <= eta (2 |v| + eta), and the float32 sums (dsub per entry, m entries) add g sum (|v| + eta)^2.
The comparisons below use twice the largest bound of a query's probed rows: two keys closer than that may come out in
either order."""
import numpy as np
import pytest

import ivf_ref
import ivfpq_ref

pytestmark = pytest.mark.gpu

METRICS = [("ip", False), ("cos", True), ("l2", False)]


def _m(metric):
    return "l2" if metric == "l2" else "ip"


def _prep(x, normalize):
    return ivf_ref.normalize_rows(np.asarray(x, np.float32)) if normalize else np.ascontiguousarray(x, dtype=np.float32)


def _mk(d, nlist, metric, normalize, m):
    from anorag_hip import IVFIndex, METRIC_IP, METRIC_L2
    return IVFIndex(d, nlist, METRIC_L2 if metric == "l2" else METRIC_IP, normalize=normalize, pq_m=m)


def _books(res, m, rng):
    """initial codebooks: the sub-vectors of 256 random residual rows"""
    pick = res[rng.choice(len(res), 256, replace=False)]
    return np.ascontiguousarray(ivfpq_ref.sub(pick, m).transpose(1, 0, 2))


def _given(x, metric, normalize, nlist, m, seed):
    """a PQ handle with given centroids and codebooks holding x, and the restated lists / codes"""
    rng = np.random.default_rng(seed)
    xp = _prep(x, normalize)
    cent = xp[rng.choice(len(x), nlist, replace=False)].copy()
    lists = ivf_ref.assign(xp, cent, _m(metric))
    res = ivfpq_ref.residuals(xp, cent, lists)
    cb = _books(res, m, rng)
    h = _mk(x.shape[1], nlist, metric, normalize, m)
    h.set_centroids(cent)
    h.set_codebooks(cb)
    h.add(x)
    return h, xp, cent, cb, lists, ivfpq_ref.encode(res, cb)


def _check_search(h, q, qp, cent, cb, lists, codes, ids, k, nprobe, metric):
    """ids equal the restated ADC top-k except among keys within the bound; D within the bound; returns (D, I)"""
    mt = _m(metric)
    D, I = h.search(q, k, nprobe=nprobe)
    Dr, Ir, S = ivfpq_ref.search(qp, lists, codes, ids, cent, cb, k, nprobe, mt)
    B = ivfpq_ref.key_bounds(qp, lists, codes, cent, cb, mt)
    ok = ivf_ref.probe_margin(qp, cent, nprobe, mt) > 1e-9
    assert int((~ok).sum()) <= len(q) // 8
    P = ivf_ref.probed(qp, cent, nprobe, mt)
    pos = {int(v): i for i, v in enumerate(ids)}
    for i in np.flatnonzero(ok):
        sel = np.isin(lists, P[i])
        tol = 2.0 * float(B[i, sel].max()) if sel.any() else 0.0
        assert np.array_equal(I[i] < 0, Ir[i] < 0), (i, k, nprobe)
        a, b = set(I[i][I[i] >= 0].tolist()), set(Ir[i][Ir[i] >= 0].tolist())
        if a != b:
            kth = float(np.sort(S[i, sel])[::-1][min(k, int(sel.sum())) - 1])
            for v in a ^ b:
                assert abs(S[i, pos[v]] - kth) <= tol, (i, k, nprobe, v)
        valid = Ir[i] >= 0
        assert float(np.max(np.abs(D[i][valid].astype(np.float64) - Dr[i][valid]), initial=0.0)) <= tol, (i, k, nprobe)
        if (~valid).any():
            assert np.all(D[i][~valid] == (ivfpq_ref.FLT_MAX if metric == "l2" else -ivfpq_ref.FLT_MAX))
        # each D is the key of its own id
        got = I[i][I[i] >= 0]
        kd = S[i, [pos[v] for v in got]]
        assert float(np.max(np.abs(D[i][:len(got)] - (kd if mt == "ip" else -kd)), initial=0.0)) <= tol / 2, (i, k)
    return D, I


@pytest.mark.parametrize("metric,normalize", METRICS)
def test_codes_equal_the_restated_encoding(metric, normalize):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((20_000, 128), dtype=np.float32)
    h, xp, cent, cb, lists, codes = _given(x, metric, normalize, 40, 16, 4)
    ids = np.arange(len(x))
    gl, gc = h.codes(ids)
    assert np.array_equal(gl, lists)
    assert np.array_equal(gc, codes)
    assert np.array_equal(h.assignments(ids), lists)
    assert np.array_equal(h.reconstruct(ids[:100]), xp[:100])  # the float32 rows, from the host copy
    assert np.array_equal(h.decode(ids[:500]), ivfpq_ref.decode(lists[:500], codes[:500], cent, cb))
    h.close()


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_codes_on_exact_and_near_ties(metric):
    """dyadic data: the float32 tile pass sees exact ties (equal entries, equidistant residuals) and near ties (2^-17
    apart), all settled in float64 as the restatement settles them"""
    rng = np.random.default_rng(8)
    d, m, nlist = 64, 8, 2
    cent = np.zeros((nlist, d), dtype=np.float32)
    cent[1] = 64.0
    cb = rng.integers(-4, 5, (m, 256, d // m)).astype(np.float32)
    cb[:, 17] = cb[:, 3]  # duplicated entries: the lower code wins
    x = rng.integers(-5, 6, (3000, d)).astype(np.float32)
    # residuals halfway between entries 5 and 9 of every sub-space, and nudged 2^-17 towards either
    mid = ((cb[:, 5] + cb[:, 9]) / 2).reshape(-1)
    step = (cb[:, 9] - cb[:, 5]).reshape(-1) * np.float32(2.0 ** -17)
    x[:100] = mid
    x[100:200] = mid + step
    x[200:300] = mid - step
    h = _mk(d, nlist, metric, False, m)
    h.set_centroids(cent)
    h.set_codebooks(cb)
    h.add(x)
    lists = ivf_ref.assign(x, cent, metric)
    codes = ivfpq_ref.encode(ivfpq_ref.residuals(x, cent, lists), cb)
    gl, gc = h.codes(np.arange(len(x)))
    assert np.array_equal(gl, lists) and np.array_equal(gc, codes)
    assert not np.any(gc == 17)
    h.close()


@pytest.mark.parametrize("metric,normalize", METRICS)
def test_pq_training_matches_lloyd_and_is_deterministic(metric, normalize):
    from anorag_hip import AnoragError
    rng = np.random.default_rng(21)
    d, m, nlist = 64, 8, 16
    x = rng.standard_normal((6000, d), dtype=np.float32)
    xp = _prep(x, normalize)
    cent = xp[rng.choice(len(x), nlist, replace=False)].copy()
    lists = ivf_ref.assign(xp, cent, _m(metric))
    res = ivfpq_ref.residuals(xp, cent, lists)
    init = _books(res, m, rng)
    h = _mk(d, nlist, metric, normalize, m)
    h.set_centroids(cent)
    h.set_codebooks(init)
    h.pq_train_from(x, 6)
    ref = ivfpq_ref.train(res, init, 6)
    assert h.codebooks.tobytes() == ref.tobytes()
    h.close()
    a, b = _mk(d, nlist, metric, normalize, m), _mk(d, nlist, metric, normalize, m)
    a.train(x, niter=5, seed=7)
    b.train(x, niter=5, seed=7)
    assert a.centroids.tobytes() == b.centroids.tobytes()
    assert a.codebooks.tobytes() == b.codebooks.tobytes()
    assert a.is_trained
    c = _mk(d, 4, metric, normalize, m)
    with pytest.raises(AnoragError):
        c.train(x[:255], niter=5, seed=7)
    assert not c.is_trained
    for v in (a, b, c):
        v.close()


@pytest.mark.parametrize("metric,normalize", METRICS)
def test_search_equals_the_restated_adc(metric, normalize):
    rng = np.random.default_rng(31)
    x = rng.standard_normal((30_000, 96), dtype=np.float32)
    h, xp, cent, cb, lists, codes = _given(x, metric, normalize, 48, 12, 32)
    q = rng.standard_normal((48, 96), dtype=np.float32)
    qp = _prep(q, normalize)
    ids = np.arange(len(x), dtype=np.int64)
    for nprobe in (1, 5, 48):
        for k in (1, 10, 100):
            D, I = _check_search(h, q, qp, cent, cb, lists, codes, ids, k, nprobe, metric)
    # D is the key of q against decode(id)
    dec = h.decode(I[I >= 0])
    qq = np.repeat(qp.astype(np.float64), (I >= 0).sum(axis=1), axis=0)
    want = (qq * dec).sum(1) if _m(metric) == "ip" else ((qq - dec) ** 2).sum(1)
    bnd = ivfpq_ref.key_bounds(qp, lists, codes, cent, cb, _m(metric))
    rows = np.repeat(np.arange(len(q)), (I >= 0).sum(axis=1))
    # decode() rounds c + cb to float32 (rho <= u |decode| per value), which moves the key by at most
    # sum |q| rho (IP) or sum rho (2 |q - decode| + rho) (L2)
    rho = 2.0 ** -24 * np.abs(dec.astype(np.float64))
    extra = (np.abs(qq) * rho).sum(1) if _m(metric) == "ip" else (rho * (2 * np.abs(qq - dec) + rho)).sum(1)
    assert np.all(np.abs(D[I >= 0] - want) <= bnd[rows, I[I >= 0]] + extra)
    assert h.last_search_stats() == {"n_queries": 48, "n_exact_rescan": 0}
    h.close()


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_duplicates_come_back_by_ascending_id_and_short_lists_pad(metric):
    rng = np.random.default_rng(5)
    base = rng.standard_normal((300, 64), dtype=np.float32)
    x = np.concatenate([base, base[:50], base[:50], base[:50]])  # rows i, 300 + i, 350 + i, 400 + i are equal
    h, xp, cent, cb, lists, codes = _given(x, metric, False, 8, 8, 6)
    D, I = h.search(base[:50], 10, nprobe=1)
    for i in range(50):
        dup = [v for v in I[i] if v % 50 == i % 50 and (v == i or v >= 300)]
        assert dup == sorted(dup) and len(dup) == 4, (i, I[i])
        run = I[i][np.flatnonzero(D[i] == D[i][list(I[i]).index(i)])]
        assert list(run) == sorted(run)
    h.close()
    # lists shorter than k: padded with -1 and -FLT_MAX / +FLT_MAX
    small = x[:40]
    h, xp, cent, cb, lists, codes = _given(np.concatenate([small] * 8), metric, False, 8, 8, 7)
    q = small[:4]
    D, I = h.search(q, 400, nprobe=1)
    P = ivf_ref.probed(q, cent, 1, _m(metric))
    for i in range(4):
        n_in = int((lists == P[i][0]).sum())
        assert (I[i] >= 0).sum() == n_in and np.all(I[i][n_in:] == -1)
        assert np.all(D[i][n_in:] == (ivfpq_ref.FLT_MAX if metric == "l2" else -ivfpq_ref.FLT_MAX))
    h.close()


@pytest.mark.parametrize("metric,normalize", METRICS)
def test_chunked_add_remove_and_add_device(metric, normalize):
    import torch
    rng = np.random.default_rng(13)
    x = rng.standard_normal((12_000, 64), dtype=np.float32)
    q = rng.standard_normal((20, 64), dtype=np.float32)
    a, xp, cent, cb, lists, codes = _given(x, metric, normalize, 24, 16, 9)
    b = _mk(64, 24, metric, normalize, 16)
    b.set_centroids(cent)
    b.set_codebooks(cb)
    for s in range(0, len(x), 3001):
        b.add(x[s:s + 3001])
    c = _mk(64, 24, metric, normalize, 16)
    c.set_centroids(cent)
    c.set_codebooks(cb)
    xd = torch.from_numpy(x).cuda()
    c.add_device(xd.data_ptr(), len(x))
    torch.cuda.synchronize()
    ids = np.arange(len(x))
    Da, Ia = a.search(q, 50, nprobe=6)
    for o in (b, c):
        assert all(np.array_equal(u, v) for u, v in zip(a.codes(ids), o.codes(ids)))
        Do, Io = o.search(q, 50, nprobe=6)
        assert np.array_equal(Io, Ia) and Do.tobytes() == Da.tobytes()
    gone = np.arange(0, len(x), 7)
    assert a.remove_ids(gone) == len(gone) and a.ntotal == len(x) - len(gone)
    keep = np.setdiff1d(ids, gone)
    qp = _prep(q, normalize)
    D, I = _check_search(a, q, qp, cent, cb, lists[keep], codes[keep], keep.astype(np.int64), 50, 6, metric)
    assert not np.isin(I, gone).any()
    assert int(a.list_sizes().sum()) == len(keep)
    for o in (a, b, c):
        o.close()


def test_memory_is_codes_and_ids():
    from anorag_hip import IVFIndex, METRIC_IP
    rng = np.random.default_rng(17)
    d, n, nlist, m = 128, 50_000, 64, 8
    x = rng.standard_normal((n, d), dtype=np.float32)
    pq = _mk(d, nlist, "ip", True, m)
    pq.train(x[:20_000], niter=4, seed=3)
    pq.add(x)
    flat = IVFIndex(d, nlist, METRIC_IP, normalize=True)
    flat.set_centroids(pq.centroids)
    flat.add(x)
    mp, mf = pq.memory(), flat.memory()
    dsub = d // m
    bound = (n + 64 * nlist) * (m + 8) + nlist * (4 * d + 8) + 256 * m * (4 * dsub + 8) + 4 * m
    assert mp["device_bytes"] <= bound
    assert mp["device_bytes"] * 10 <= mf["device_bytes"]
    assert mp["host_bytes"] >= n * d * 4  # the float32 rows live on the host
    pq.close()
    flat.close()


@pytest.fixture
def cfg(tmp_path):
    from anorag_hip.compat import config
    config.reset()
    config.set("storage.vector_index_path", str(tmp_path / "vidx"))
    config.set("vector_store.index_type", "IVFPQ")
    config.set("vector_store.nlist", 16)
    config.set("vector_store.nprobe", 4)
    config.set("vector_store.pq_m", 8)
    yield config
    config.reset()


def test_facade_ivfpq(cfg):
    from anorag_hip import FlatIndex, IVFIndex
    from vector_store import VectorIndex
    rng = np.random.default_rng(71)
    x = rng.standard_normal((5000, 64), dtype=np.float32)
    q = rng.standard_normal((12, 64), dtype=np.float32)
    cfg.set("anorag_hip.ivf", True)
    cfg.set("anorag_hip.ivf_pq", True)
    vi = VectorIndex(64)
    assert vi.create_index() and isinstance(vi.index, IVFIndex) and vi.index.pq_m == 8
    assert vi.add_vectors(x) and vi.is_trained and vi.index.ntotal == 5000
    hits = vi.search(q, top_k=10)
    # the same handle built by hand: spherical coarse k-means for inner product, 10 iterations, seed 1234
    h = IVFIndex(64, 16, 0, normalize=True, spherical=True, pq_m=8)
    h.train(vi._preprocess_vectors(x), niter=10, seed=1234)  # what train_index hands the index
    h.add(x)
    D, I = h.search(q, 10, nprobe=4)
    assert [[r["index"] for r in row] for row in hits] == I.tolist()
    assert [[r["score"] for r in row] for row in hits] == D.tolist()
    h.close()
    path = vi.save_index()
    assert path
    name = path.split("/")[-1]
    vi2 = VectorIndex(64)
    assert vi2.load_index(name) and isinstance(vi2.index, IVFIndex) and vi2.index.pq_m == 8
    assert vi2.index.codebooks.tobytes() == vi.index.codebooks.tobytes()
    ids = np.arange(5000)
    assert all(np.array_equal(u, v) for u, v in zip(vi.index.codes(ids), vi2.index.codes(ids)))
    assert vi2.search(q, top_k=10) == hits
    cfg.set("anorag_hip.ivf_pq", False)
    vi3 = VectorIndex(64)
    assert vi3.load_index(name) and isinstance(vi3.index, IVFIndex) and vi3.index.pq_m is None
    assert vi3.index.ntotal == 5000 and np.array_equal(vi3.index.centroids, vi.index.centroids)
    cfg.set("anorag_hip.ivf", False)
    vi4 = VectorIndex(64)
    assert vi4.load_index(name) and isinstance(vi4.index, FlatIndex) and vi4.index.ntotal == 5000
    for v in (vi, vi2, vi3, vi4):
        v.cleanup()


def test_facade_ivfpq_key_leaves_the_other_types_alone(cfg):
    from anorag_hip import FlatIndex, IVFIndex
    from vector_store import VectorIndex
    x = np.random.default_rng(2).standard_normal((100, 64), dtype=np.float32)
    cfg.set("anorag_hip.ivf_pq", True)  # without anorag_hip.ivf: no effect
    vi = VectorIndex(64)
    assert vi.create_index() and isinstance(vi.index, FlatIndex)
    cfg.set("anorag_hip.ivf", True)
    vi = VectorIndex(64)
    assert vi.create_index("IVFFlat") and isinstance(vi.index, IVFIndex) and vi.index.pq_m is None
    assert vi.create_index("Flat") and isinstance(vi.index, FlatIndex)
    assert vi.create_index("IVFPQ") and vi.index.pq_m == 8
    few = VectorIndex(64)
    assert few.create_index() and few.index.pq_m == 8
    assert not few.train_index(x)  # 100 rows cannot train 256 codes per sub-space
    few.cleanup()
    cfg.set("vector_store.pq_m", 7)  # 64 does not split into 7 sub-spaces
    bad = VectorIndex(64)
    assert not bad.create_index()
    cfg.set("vector_store.pq_m", 8)
    cfg.set("anorag_hip.ivf_pq", False)
    vi2 = VectorIndex(64)
    assert vi2.create_index("IVFPQ") and isinstance(vi2.index, IVFIndex) and vi2.index.pq_m is None
    vi.cleanup()
    vi2.cleanup()
