"""GPU tests of the in-place edits of the flat index (anr_index_remove / anr_index_update): after an edit the float32 rows,
every scan image, the certificate statistics and the search results are those of an index freshly built from the edited
matrix.

Shapes: 3 017 rows (94 full tiles and a ragged one), d = 768 and d = 100 (one padded k-block group).  The raw
inner-product case carries rows 0..39 scaled by 10^3, the float16 edge values in row 40 and an all-zero group in row 41,
as the image tests do; its queries are scaled by 10^-3 so that scores stay at unit scale, where the absolute 1e-4 of the
search bar is far above a float32 spacing (at 10^4 one spacing is 1e-3, and no float32 result could meet it)."""
import numpy as np
import pytest

import index_edit_ref as ref
from oracle import flat_index as orc

pytestmark = pytest.mark.gpu

N = 3017
K = 10
SCORE_TOL = 1e-4
EXTRA = 100          # rows added after a removal: the ragged tile then has both writers

# (d, mode, scan bits, option set before the adds?) — every d, mode and image width, three cases each way
CONFIGS = [(768, "cos", 12, True), (768, "raw", 8, False), (768, "l2", 16, True),
           (100, "cos", 8, True), (100, "raw", 16, False), (100, "l2", 12, False)]
MODES = {"cos": ("ip", True), "raw": ("ip", False), "l2": ("l2", False)}

_data_cache = {}


def _data(d, mode):
    key = (d, mode)
    if key not in _data_cache:
        rng = np.random.default_rng(1000 + d + len(mode) * 7 + ord(mode[0]))
        x = rng.standard_normal((N + EXTRA, d)).astype(np.float32)
        q = rng.standard_normal((8, d)).astype(np.float32)
        if mode == "raw":
            x[:40] *= 1.0e3
            x[40, :8] = [65504.0, -65504.0, 65500.0, 65472.0, -65488.0, 6.1e-5, -5.9e-8, 0.0]   # the float16 edges
            x[41, :32] = 0.0                                                                        # an all-zero group
            q *= 1.0e-3
        _data_cache[key] = (x, q)
    return _data_cache[key]


def _build(d, mode, bits, before, rows, raw=False, cls=None, **kw):
    """an index of `rows`; raw: the rows are stored ones (ANR_OPT_ADD_RAW)"""
    from anorag_hip import FlatIndex, METRIC_IP, METRIC_L2
    from anorag_hip._lib import OPT_ADD_RAW, OPT_SCAN_BITS
    metric, normalize = MODES[mode]
    idx = (cls or FlatIndex)(d, METRIC_L2 if metric == "l2" else METRIC_IP, normalize=normalize, **kw)
    if before:
        idx.reserve(N + 2 * EXTRA)            # storage exists, so the option allocates its image and k_add fills it
        idx.set_option(OPT_SCAN_BITS, bits)
    if raw:
        idx.set_option(OPT_ADD_RAW, 1)
    if len(rows):
        idx.add(rows)
    if raw:
        idx.set_option(OPT_ADD_RAW, 0)
    if not before:
        if not len(rows):
            idx.reserve(EXTRA)                # (an index without storage would put the image off until a batch wants it)
        idx.set_option(OPT_SCAN_BITS, bits)   # k_build12 / k_build8 over the stored rows
    return idx


def _check_stats(idx, stored, bits):
    st = idx.scan_image_stats()
    widths = (16,) if bits == 16 else (16, bits)
    true = ref.true_stats(stored, widths)
    print("stats", {k: (true[k], st[k]) for k in true})
    for key, t in true.items():
        assert t <= st[key] <= t * 1.0003 + 1e-12, (key, t, st[key])
    return st


def _check_images(idx, stored, bits):
    n = len(stored)
    assert idx.ntotal == n
    assert idx.reconstruct_n(0, n).tobytes() == stored.tobytes()
    for b in ((16,) if bits == 16 else (16, bits)):
        assert idx.reconstruct_scan_image(b, 0, n).tobytes() == ref.image(stored, b).tobytes(), b


def _check_search(idx, stored, q, mode):
    """stored: what the index holds (already preprocessed); near-tie-aware id sets, scores within 1e-4, best first"""
    from anorag_hip._lib import OPT_FORCE_EXACT, OPT_TINY
    metric, normalize = MODES[mode]
    n = len(stored)
    qm = orc.preprocess_vectors(q, "cosine" if normalize else "raw")
    if n == 0:
        D, I = idx.search(q, K)
        assert np.all(I == -1)
        return
    Dr, Ir = orc.flat_search(qm, stored, K, metric)
    s64 = orc.exact_scores(qm, stored, metric)
    valid = Ir >= 0
    for opt, value, qs in ((OPT_TINY, 0, slice(0, 3)), (OPT_TINY, 1, slice(0, 3)), (OPT_TINY, 1, slice(0, 8)),
                           (OPT_FORCE_EXACT, 1, slice(0, 8))):
        idx.set_option(opt, value)
        D, I = idx.search(q[qs], K)
        idx.set_option(OPT_FORCE_EXACT, 0)
        idx.set_option(OPT_TINY, 1)
        assert I.max() < n, "an id at or beyond ntotal came back"
        assert np.array_equal(I >= 0, valid[qs])
        assert orc.near_tie_equal(I, Ir[qs], s64[qs], K, 1e-6), ("top-k id sets differ beyond near-ties", opt, value)
        err = np.max(np.abs(D[valid[qs]] - Dr[qs][valid[qs]]), initial=0.0)
        print("search", opt, value, "max |D - Dr|", err)
        assert err <= SCORE_TOL, (opt, value, err)
        sign = -1.0 if metric == "ip" else 1.0
        assert np.all(sign * np.diff(D, axis=1)[valid[qs][:, 1:]] >= 0)


def _patterns():
    rng = np.random.default_rng(9)
    tenth = rng.choice(N, N // 10, replace=False)
    return {
        "row0": ([0], 0),
        "last": ([N - 1], 0),
        "tile": (list(range(64, 96)), 0),
        "middle_chunk64": ([1500], 64),     # a shift of one across dozens of chunks: sources overlap destinations
        # (unsorted, with a few repeats and rows outside mixed in: they are ignored)
        "random_tenth": (np.concatenate([tenth, tenth[:7], [-1, N, N + 64]]).tolist(), 0),
        "every_second": (list(range(0, N, 2)), 0),
        "all_but_1500": ([i for i in range(N) if i != 1500], 0),
        "all": (list(range(N)), 0),
        "nothing_valid": ([-1, -1, N, N, N + 5, -7, 10 ** 12], 0),
    }


PATTERNS = _patterns()


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("d,mode,bits,before", CONFIGS)
def test_remove_equals_a_fresh_build(d, mode, bits, before, pattern):
    from anorag_hip._lib import OPT_EDIT_CHUNK_ROWS
    x, q = _data(d, mode)
    rows, chunk = PATTERNS[pattern]
    idx = _build(d, mode, bits, before, x[:N])
    stored_before = idx.reconstruct_n(0, N)
    images_before = {b: idx.reconstruct_scan_image(b, 0, N) for b in {16, bits}}
    stats_before = idx.scan_image_stats()
    gone = ref.valid_gone(rows, N)
    idx.set_option(OPT_EDIT_CHUNK_ROWS, chunk)
    assert idx.remove_rows(rows) == len(gone)
    survivors = np.delete(stored_before, gone, axis=0)
    assert np.array_equal(survivors, stored_before[ref.source_map(N, gone)])
    assert idx.ntotal == N - len(gone)
    _check_images(idx, survivors, bits)
    if len(gone) == 0:      # every byte as it was
        for b, img in images_before.items():
            assert idx.reconstruct_scan_image(b, 0, N).tobytes() == img.tobytes()
    st = _check_stats(idx, survivors, bits)
    if mode == "raw" and len(survivors) and np.array_equal(gone[:41], np.arange(41)):   # the 10^3 rows and the edges went
        assert st["max_norm"] < 0.01 * stats_before["max_norm"]
    _check_search(idx, survivors, q, mode)
    # 100 further rows: equal to a fresh index of the survivors plus the new rows
    idx.add(x[N:])
    fresh = _build(d, mode, bits, before, survivors, raw=True)
    fresh.add(x[N:])
    n2 = len(survivors) + EXTRA
    stored2 = fresh.reconstruct_n(0, n2)
    assert stored2[:len(survivors)].tobytes() == survivors.tobytes()
    _check_images(idx, stored2, bits)
    _check_images(fresh, stored2, bits)
    _check_stats(idx, stored2, bits)
    _check_search(idx, stored2, q, mode)
    idx.close()
    fresh.close()


def test_removing_the_large_rows_tightens_the_certificate_statistics():
    """rows 0..40 of the raw case hold the largest norms (10^3 scale, the float16 edges) and with them the largest image
    errors: once they are gone every statistic is the survivors' own, not the maximum ever seen"""
    d, mode, bits = 768, "raw", 12
    x, q = _data(d, mode)
    idx = _build(d, mode, bits, False, x[:N])
    before = idx.scan_image_stats()
    stored = idx.reconstruct_n(0, N)
    assert idx.remove_rows(np.arange(41)) == 41
    st = _check_stats(idx, stored[41:], bits)
    print(before, st)
    assert st["max_norm"] < 0.01 * before["max_norm"]
    assert st["max_err16"] < 0.01 * before["max_err16"] and st["max_err12"] < 0.01 * before["max_err12"]
    _check_search(idx, stored[41:], q, mode)
    idx.close()


@pytest.mark.parametrize("d,mode,bits,before", [(768, "cos", 12, True), (100, "l2", 8, False)])
def test_compaction_chunk_size_does_not_change_a_byte(d, mode, bits, before):
    from anorag_hip._lib import OPT_EDIT_CHUNK_ROWS
    x, q = _data(d, mode)
    rows = np.random.default_rng(4).choice(N, N // 10, replace=False)
    out = []
    for chunk in (32, 96, 0):
        idx = _build(d, mode, bits, before, x[:N])
        idx.set_option(OPT_EDIT_CHUNK_ROWS, chunk)
        assert idx.remove_rows(rows) == len(rows)
        n = idx.ntotal
        D, I = idx.search(q, K)     # (L2: the moved row biases enter the scores)
        out.append((idx.reconstruct_n(0, n).tobytes(), idx.reconstruct_scan_image(16, 0, n).tobytes(),
                    idx.reconstruct_scan_image(bits, 0, n).tobytes(), D.tobytes(), I.tobytes()))
        idx.close()
    assert out[0] == out[1] == out[2]
    stored = np.frombuffer(out[0][0], dtype=np.float32).reshape(-1, d)
    base = _build(d, mode, bits, before, x[:N])
    assert stored.tobytes() == np.delete(base.reconstruct_n(0, N), rows, axis=0).tobytes()
    base.close()


@pytest.mark.parametrize("d,mode,bits,before", [(768, "cos", 8, False), (100, "raw", 12, True), (768, "l2", 12, True),
                                                (100, "cos", 16, False)])
def test_update_equals_a_fresh_build_of_the_edited_matrix(d, mode, bits, before):
    from anorag_hip._lib import AnoragError
    x, q = _data(d, mode)
    rng = np.random.default_rng(21)
    rows = np.concatenate([[0, 31, 32, 33, N - 1], np.arange(60, 71), rng.choice(np.arange(100, N - 1), 200, replace=False)])
    if mode == "raw":
        rows = np.concatenate([rows, np.arange(1, 42)])      # the large rows become ordinary ones: the maxima must drop
    rows = rng.permutation(np.unique(rows))
    new = rng.standard_normal((len(rows), d)).astype(np.float32)
    edited = x[:N].copy()
    edited[rows] = new
    # one row listed twice: the last entry wins
    twice = int(rows[5])
    rows_arg = np.concatenate([[twice], rows])
    new_arg = np.concatenate([rng.standard_normal((1, d)).astype(np.float32), new])
    idx = _build(d, mode, bits, before, x[:N])
    before_stats = idx.scan_image_stats()
    idx.update_rows(rows_arg, new_arg)
    fresh = _build(d, mode, bits, before, edited)
    stored = fresh.reconstruct_n(0, N)
    _check_images(fresh, stored, bits)
    _check_images(idx, stored, bits)
    st = _check_stats(idx, stored, bits)
    if mode == "raw":
        assert st["max_norm"] < 0.01 * before_stats["max_norm"]
    _check_search(idx, stored, q, mode)
    # a row outside the index: an error, and nothing changed
    with pytest.raises(AnoragError):
        idx.update_rows([5, N], new[:2])
    with pytest.raises(AnoragError):
        idx.update_rows([-1], new[:1])
    assert idx.reconstruct_n(0, N).tobytes() == stored.tobytes()
    idx.update_rows([], np.zeros((0, d), np.float32))
    assert idx.reconstruct_n(0, N).tobytes() == stored.tobytes()
    idx.close()
    fresh.close()


def test_a_batch_in_flight_answers_from_the_rows_before_the_edit():
    import torch
    d, mode, bits = 768, "cos", 16
    x, _ = _data(d, mode)
    dev = torch.device("cuda", 0)
    nq = 64
    qh = np.random.default_rng(8).standard_normal((nq, d)).astype(np.float32)
    qd = torch.from_numpy(qh).to(dev)
    D = torch.empty((nq, K), device=dev)
    I = torch.empty((nq, K), device=dev, dtype=torch.int64)
    torch.cuda.synchronize()
    idx = _build(d, mode, bits, False, x[:N])
    stored = idx.reconstruct_n(0, N)
    gone = np.arange(0, N, 3)
    idx.search_device_async(qd.data_ptr(), nq, K, D.data_ptr(), I.data_ptr(), 0)
    assert idx.remove_rows(gone) == len(gone)
    idx.wait(0)
    torch.cuda.synchronize()
    qm = orc.preprocess_vectors(qh)
    for got_D, got_I, rows in ((D.cpu().numpy(), I.cpu().numpy(), stored), (*idx.search(qh, K), np.delete(stored, gone, 0))):
        Dr, Ir = orc.flat_search(qm, rows, K, "ip")
        assert orc.near_tie_equal(got_I, Ir, orc.exact_scores(qm, rows, "ip"), K, 1e-6)
        assert np.max(np.abs(got_D - Dr)) <= SCORE_TOL
    idx.close()


def test_score_rows_and_self_join_see_the_new_numbering():
    d, mode, bits = 100, "cos", 16
    x, q = _data(d, mode)
    idx = _build(d, mode, bits, False, x[:N])
    stored = idx.reconstruct_n(0, N)
    gone = np.random.default_rng(12).choice(N, 700, replace=False)
    assert idx.remove_rows(gone) == 700
    s = np.delete(stored, gone, axis=0)
    n = len(s)
    ids = np.random.default_rng(13).integers(0, n, size=(len(q), 9))
    ids[0, 0] = n                                                  # one past the new end: no row any more
    got = idx.score_rows(q, ids)
    qn = orc.preprocess_vectors(q)
    want = np.einsum("qd,qjd->qj", qn.astype(np.float64), s[np.clip(ids, 0, n - 1)].astype(np.float64))
    assert np.isnan(got[0, 0])
    ok = np.ones(ids.shape, dtype=bool)
    ok[0, 0] = False
    assert np.max(np.abs(got[ok] - want[ok])) <= 1e-6
    s64 = s.astype(np.float64) @ s.astype(np.float64).T
    thr = 0.3
    I, J, S = idx.self_join(thr)
    assert np.all(I < J) and J.max() < n
    gotm = np.zeros((n, n), dtype=bool)
    gotm[I, J] = True
    assert gotm.sum() == len(I) > 100
    near = np.abs(s64 - thr) <= 1e-6
    assert not ((gotm != np.triu(s64 >= thr, 1)) & ~near).any()
    assert np.max(np.abs(S - s64[I, J])) <= 1e-6
    idx.close()


def test_a_graph_index_is_rebuilt_after_an_edit():
    """an update keeps ntotal, so only the stale mark tells the graph that its rows changed: the row rewritten to a copy
    of the query must come back first, which the graph built before the edit (and its traversal image) cannot deliver"""
    from anorag_hip import GraphIndex
    d, mode = 100, "cos"
    x, q = _data(d, mode)
    idx = _build(d, mode, 16, False, x[:N], cls=GraphIndex, R=32, build_degree=64, ef_search=128)
    idx.search(q, K)
    assert idx.has_fresh_graph()
    target = 2222
    idx.update_rows([target], q[:1])
    assert not idx.has_fresh_graph()
    D, I = idx.search(q[:1], K)
    assert I[0, 0] == target and abs(D[0, 0] - 1.0) <= 1e-5
    assert idx.has_fresh_graph()
    # a removal in front of it renumbers it: the rebuilt graph answers with the new number
    assert idx.remove_rows([5, 6, 7, target + 1]) == 4
    assert not idx.has_fresh_graph()
    D, I = idx.search(q[:1], K)
    assert I[0, 0] == target - 3 and I.max() < N - 4
    idx.close()
