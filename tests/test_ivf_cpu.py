"""CPU tests of the IVF restatement (tests/ivf_ref.py) and of the IVF save trailer's pure-Python helpers."""
import io
import struct

import numpy as np
import pytest

import ivf_ref


def test_assign_known_answers_and_ties():
    cent = np.array([[1, 0], [0, 1], [1, 0]], dtype=np.float32)  # lists 0 and 2 are equal: 0 wins
    x = np.array([[2, 0], [0, 3], [1, 1]], dtype=np.float32)
    assert ivf_ref.assign(x, cent, "ip").tolist() == [0, 1, 0]  # [1, 1]: a tie of all three -> 0
    assert ivf_ref.assign(x, cent, "l2").tolist() == [0, 1, 0]


def test_probed_lists_order_and_ties():
    cent = np.array([[3, 0], [1, 0], [2, 0], [2, 0]], dtype=np.float32)
    q = np.array([[1, 0]], dtype=np.float32)
    assert ivf_ref.probed(q, cent, 3, "ip").tolist() == [[0, 2, 3]]
    assert ivf_ref.probed(q, cent, 2, "l2").tolist() == [[1, 2]]
    assert ivf_ref.probe_margin(q, cent, 2, "ip")[0] == 0.0
    assert ivf_ref.probe_margin(q, cent, 4, "ip")[0] == np.inf


def test_search_known_answer_short_lists_and_padding():
    cent = np.array([[1, 0], [-1, 0]], dtype=np.float32)
    x = np.array([[1, 0], [2, 0], [-1, 0], [2, 0]], dtype=np.float32)
    ids = np.array([10, 11, 12, 13], dtype=np.int64)
    lists = ivf_ref.assign(x, cent, "ip")
    assert lists.tolist() == [0, 0, 1, 0]
    q = np.array([[1, 0]], dtype=np.float32)
    D, I = ivf_ref.search(q, x, ids, lists, cent, 5, 1, "ip")
    assert I.tolist() == [[11, 13, 10, -1, -1]]  # 11 and 13 tie: lower id first
    assert D[0, :3].tolist() == [2, 2, 1] and D[0, 3] == -ivf_ref.FLT_MAX
    D, I = ivf_ref.search(q, x, ids, lists, cent, 5, 2, "l2")
    assert I.tolist() == [[10, 11, 13, 12, -1]] and D[0, 4] == ivf_ref.FLT_MAX
    assert D[0, :4].tolist() == [0, 1, 1, 4]


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_lloyd_invariants(metric):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((600, 16)).astype(np.float32)
    c = x[rng.choice(600, 12, replace=False)].copy()
    prev = ivf_ref.inertia(x, c, "l2")
    for _ in range(6):
        a = ivf_ref.assign(x, c, metric)
        c = ivf_ref.means(x, a, c)
        if metric == "l2":  # Lloyd never increases the L2 inertia
            cur = ivf_ref.inertia(x, c, "l2")
            assert cur <= prev + 1e-6 * abs(prev)
            prev = cur
    a = ivf_ref.assign(x, c, metric)
    c2 = ivf_ref.means(x, a, c)
    for l in range(12):
        m = a == l
        if m.any():
            assert np.allclose(c2[l], x[m].astype(np.float64).mean(0), atol=1e-6)


def test_empty_list_takes_half_of_the_largest():
    x = np.array([[0, 0], [1, 0], [2, 0], [3, 0], [10, 0]], dtype=np.float32)
    cent = np.array([[1, 0], [100, 100], [10, 0]], dtype=np.float32)  # list 1 gets no rows
    a = ivf_ref.assign(x, cent, "l2")
    assert a.tolist() == [0, 0, 0, 0, 2]
    c = ivf_ref.means(x, a, cent)
    assert c[0].tolist() == [0.5, 0] and c[1].tolist() == [2.5, 0] and c[2].tolist() == [10, 0]


def test_ivf_trailer_layout_round_trip():
    from vector_store.vector_index import read_ivf_trailer, write_ivf_trailer
    c = np.arange(12, dtype=np.float32).reshape(3, 4) / 7
    f = io.BytesIO()
    write_ivf_trailer(f, c)
    raw = f.getvalue()
    assert raw[:8] == b"ANRIVF01" and struct.unpack("<ii", raw[8:16]) == (3, 4) and len(raw) == 16 + 48
    assert np.array_equal(np.frombuffer(raw[16:], dtype="<f4").reshape(3, 4), c)
    f.seek(0)
    assert np.array_equal(read_ivf_trailer(f, 4), c)
    assert read_ivf_trailer(io.BytesIO(b""), 4) is None  # an exact index's file ends after its rows
    with pytest.raises(ValueError):
        read_ivf_trailer(io.BytesIO(raw), 5)
    with pytest.raises(ValueError):
        read_ivf_trailer(io.BytesIO(raw[:-4]), 4)
