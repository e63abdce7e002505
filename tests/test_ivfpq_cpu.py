"""CPU tests of the IVF-PQ restatement (tests/ivfpq_ref.py) and of the PQ save trailer's pure-Python helpers."""
import io
import struct

import numpy as np
import pytest

import ivf_ref
import ivfpq_ref


def _books():
    # m = 2 sub-spaces of 2 values; entries 0..3 hand-made, the rest far away
    cb = np.full((2, 256, 2), 100.0, dtype=np.float32)
    cb[0, :4] = [[0, 0], [1, 0], [1, 0], [0, 1]]  # entries 1 and 2 are equal: 1 wins
    cb[1, :4] = [[0, 0], [2, 0], [0, 2], [-2, 0]]
    return cb


def test_encode_known_answers_and_ties():
    cb = _books()
    res = np.array([[1, 0, 2, 0],        # exact matches
                    [0.5, 0, 1, 0],      # midway between 0 and 1 (and 2) / between 0 and 1: lower code
                    [0, 0.9, -1.2, 0],   # 3 / 3
                    [0.5, 0.5, 1, 1]],   # 0, 1, 2, 3 all at 0.5 / 0, 1, 2 at 2: lowest
                   dtype=np.float32)
    assert ivfpq_ref.encode(res, cb).tolist() == [[1, 1], [0, 0], [3, 3], [0, 0]]


def test_residuals_decode_and_adc_keys():
    cb = _books()
    cent = np.array([[10, 0, 0, 0], [0, 0, 0, 10]], dtype=np.float32)
    x = np.array([[11, 0, 2, 0], [0, 1, -2, 10]], dtype=np.float32)
    lists = ivf_ref.assign(x, cent, "l2")
    assert lists.tolist() == [0, 1]
    r = ivfpq_ref.residuals(x, cent, lists)
    assert r.tolist() == [[1, 0, 2, 0], [0, 1, -2, 0]]
    codes = ivfpq_ref.encode(r, cb)
    assert codes.tolist() == [[1, 1], [3, 3]]
    dec = ivfpq_ref.decode(lists, codes, cent, cb)
    assert np.array_equal(dec, x)  # every residual is an entry: decoding is exact
    q = np.array([[1, 2, 3, 4]], dtype=np.float32)
    kip = ivfpq_ref.adc_keys(q, lists, codes, cent, cb, "ip")
    kl2 = ivfpq_ref.adc_keys(q, lists, codes, cent, cb, "l2")
    assert np.allclose(kip, q.astype(np.float64) @ dec.T.astype(np.float64))
    assert np.allclose(kl2, -((q.astype(np.float64) - dec) ** 2).sum(1)[None, :])


def test_search_ties_to_the_lower_id_and_padding():
    cb = _books()
    cent = np.array([[0, 0, 0, 0], [-50, -50, -50, -50]], dtype=np.float32)
    lists = np.array([0, 0, 0, 1], dtype=np.int64)
    codes = np.array([[1, 1], [2, 1], [0, 0], [0, 0]], dtype=np.uint8)  # rows 0 and 1 decode to the same vector
    ids = np.array([7, 3, 5, 9], dtype=np.int64)
    q = np.array([[1, 0, 1, 0]], dtype=np.float32)
    D, I, _ = ivfpq_ref.search(q, lists, codes, ids, cent, cb, 5, 1, "ip")
    assert I.tolist() == [[3, 7, 5, -1, -1]]  # 3 and 7 tie: lower id first
    assert D[0, :3].tolist() == [3, 3, 0] and D[0, 3] == -ivfpq_ref.FLT_MAX
    D, I, _ = ivfpq_ref.search(q, lists, codes, ids, cent, cb, 5, 2, "l2")
    assert I[0, :4].tolist() == [3, 7, 5, 9] and I[0, 4] == -1 and D[0, 4] == ivfpq_ref.FLT_MAX
    assert D[0, :3].tolist() == [1, 1, 2]


def test_train_is_lloyd_per_sub_space():
    rng = np.random.default_rng(5)
    res = rng.standard_normal((600, 8)).astype(np.float32)
    init = np.ascontiguousarray(ivfpq_ref.sub(res[:256], 2).transpose(1, 0, 2))
    cb = ivfpq_ref.train(res, init, 3)
    assert cb.shape == (2, 256, 4)
    for j in range(2):
        assert np.array_equal(cb[j], ivf_ref.lloyd(np.ascontiguousarray(res[:, 4 * j:4 * j + 4]), init[j], 3, "l2"))
    # encoding with the trained books does not increase the distortion of encoding with the initial ones
    def distortion(b):
        return float(((res - ivfpq_ref.decode(np.zeros(600, np.int64), ivfpq_ref.encode(res, b),
                                              np.zeros((1, 8), np.float32), b)) ** 2).sum())
    assert distortion(cb) <= distortion(init)


def test_key_bounds_cover_float32_sums():
    rng = np.random.default_rng(9)
    d, m = 32, 4
    cent = rng.standard_normal((3, d)).astype(np.float32)
    cb = rng.standard_normal((m, 256, d // m)).astype(np.float32)
    lists = rng.integers(0, 3, 50)
    codes = rng.integers(0, 256, (50, m)).astype(np.uint8)
    q = rng.standard_normal((4, d)).astype(np.float32)
    for metric in ("ip", "l2"):
        exact = ivfpq_ref.adc_keys(q, lists, codes, cent, cb, metric)
        b = ivfpq_ref.key_bounds(q, lists, codes, cent, cb, metric)
        # the device's arithmetic, restated in float32: LUT entries (ascending d), then the sum over j
        rt = cb[np.arange(m)[None, :], codes.astype(np.int64)]
        for i in range(4):
            for r in range(50):
                acc = np.float32(0)
                for j in range(m):
                    sl = slice(j * (d // m), (j + 1) * (d // m))
                    t = np.float32(0)
                    for dd in range(d // m):
                        if metric == "ip":
                            t = np.float32(t + np.float32(q[i, sl][dd] * rt[r, j, dd]))
                        else:
                            a = np.float32(q[i, sl][dd] - cent[lists[r], sl][dd])
                            e = np.float32(a - rt[r, j, dd])
                            t = np.float32(t + np.float32(e * e))
                    acc = np.float32(acc + t)
                key = float(np.float32(float(q[i].astype(np.float64) @ cent[lists[r]].astype(np.float64)) + float(acc))) \
                    if metric == "ip" else -float(acc)
                assert abs(key - exact[i, r]) <= b[i, r]


def test_pq_trailer_layout_round_trip_and_errors():
    from vector_store.vector_index import read_ivf_trailer, read_pq_trailer, write_ivf_trailer, write_pq_trailer
    cent = np.arange(8, dtype=np.float32).reshape(2, 4)
    cb = (np.arange(2 * 256 * 2, dtype=np.float32) / 3).reshape(2, 256, 2)
    f = io.BytesIO()
    write_ivf_trailer(f, cent)
    at = f.tell()
    write_pq_trailer(f, cb)
    raw = f.getvalue()
    assert raw[at:at + 8] == b"ANRPQ001" and struct.unpack("<iii", raw[at + 8:at + 20]) == (2, 8, 2)
    assert len(raw) == at + 20 + 4 * cb.size
    assert np.array_equal(np.frombuffer(raw[at + 20:], dtype="<f4").reshape(2, 256, 2), cb)
    f.seek(0)
    assert np.array_equal(read_ivf_trailer(f, 4), cent)  # the IVF reader stops after the centroids
    assert np.array_equal(read_pq_trailer(f, 4), cb)
    # an IVF-Flat file ends after the centroids
    g = io.BytesIO()
    write_ivf_trailer(g, cent)
    g.seek(0)
    read_ivf_trailer(g, 4)
    assert read_pq_trailer(g, 4) is None
    with pytest.raises(ValueError):  # dim mismatch
        read_pq_trailer(io.BytesIO(raw[at:]), 6)
    with pytest.raises(ValueError):  # truncated codebooks
        read_pq_trailer(io.BytesIO(raw[at:-4]), 4)
    with pytest.raises(ValueError):  # unknown magic
        read_pq_trailer(io.BytesIO(b"XXXXXXXX" + raw[at + 8:]), 4)
    bad = bytearray(raw[at:])
    bad[12:16] = struct.pack("<i", 4)  # nbits 4
    with pytest.raises(ValueError):
        read_pq_trailer(io.BytesIO(bytes(bad)), 4)
