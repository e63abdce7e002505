"""ANR_OPT_SCAN_BITS 8 on the device: the 8-bit image k_add / k_build8 write equals the numpy restatement
(tests/scan_image8.py) bit for bit, its tracked error norm bounds the true one, and searches through it stay the exact
top-k of the float32 rows."""
import numpy as np
import pytest

import scan_image8 as s8
from oracle import flat_index as orc

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-4


def _check(index, x, q, k, metric_name, normalize):
    D, I = index.search(q, k)
    xm = orc.preprocess_vectors(x, "cosine" if normalize else "raw")
    qm = orc.preprocess_vectors(q, "cosine" if normalize else "raw")
    Dr, Ir = orc.flat_search(qm, xm, k, metric_name)
    s64 = orc.exact_scores(qm, xm, metric_name)
    assert orc.near_tie_equal(I, Ir, s64, k, 1e-6), "top-k id sets differ beyond near-ties"
    valid = Ir >= 0
    assert np.max(np.abs(D[valid] - Dr[valid]), initial=0.0) <= SCORE_TOL
    return D, I


@pytest.mark.parametrize("d,normalize", [(768, True), (200, False)])
def test_the_eight_bit_image_equals_the_restatement(d, normalize):
    from anorag_hip import FlatIndex, METRIC_IP
    from anorag_hip._lib import AnoragError, OPT_SCAN_BITS
    rng = np.random.default_rng(5)
    n = 5_000
    x = rng.standard_normal((n, d)).astype(np.float32)
    if not normalize:
        x[:40] *= 1.0e3
        x[40, :8] = [65504.0, -65504.0, 65500.0, 65472.0, -65488.0, 6.1e-5, -5.9e-8, 0.0]   # the float16 edges
        x[41, :32] = 0.0                                                                        # an all-zero group
    idx = FlatIndex(d, METRIC_IP, normalize=normalize)
    idx.add(x[:10])
    with pytest.raises(AnoragError):
        idx.reconstruct_scan_image(8, 0, 10)       # no 8-bit image yet
    idx.add(x[10:2990])
    idx.set_option(OPT_SCAN_BITS, 8)               # k_build8 for the rows stored so far
    idx.add(x[2990:])                              # k_add for the rest (the tile at 2976..3007 gets both writers)
    stored = idx.reconstruct_n(0, n)
    img = idx.reconstruct_scan_image(8, 0, n)
    ref = s8.decode(stored)
    assert img.tobytes() == ref.tobytes()
    part = idx.reconstruct_scan_image(8, 2970, 45)
    assert part.tobytes() == ref[2970:3015].tobytes()
    st = idx.scan_image_stats()
    assert st["bits"] == 8
    true = s8.error_norm(stored)
    assert true <= st["max_err8"] <= true * 1.0003 + 1e-12, (true, st["max_err8"])
    idx.set_option(OPT_SCAN_BITS, 16)              # only the image in use is kept
    with pytest.raises(AnoragError):
        idx.reconstruct_scan_image(8, 0, 10)
    idx.close()


@pytest.mark.parametrize("when", ["before_add", "after_add"])
def test_eight_bit_scan_image_gives_the_exact_top_k(when):
    """cosine / raw inner product / L2, a ragged row count, the option set before the rows arrive (k_add) and on a filled
    index (k_build8), adds after the switch"""
    from anorag_hip import FlatIndex, METRIC_IP, METRIC_L2
    from anorag_hip._lib import OPT_SCAN_BITS
    rng = np.random.default_rng(77)
    n, d, nq, k = 200_001, 768, 64, 100
    x = rng.standard_normal((n, d), dtype=np.float32)
    q = np.random.default_rng(78).standard_normal((nq, d), dtype=np.float32)
    tiles = -(-n // 32)
    for metric, name, normalize in ((METRIC_IP, "ip", True), (METRIC_IP, "ip", False), (METRIC_L2, "l2", False)):
        idx = FlatIndex(d, metric, normalize=normalize)
        if when == "before_add":
            idx.set_option(OPT_SCAN_BITS, 8)
        idx.add(x[:150_000])
        if when == "after_add":
            idx.set_option(OPT_SCAN_BITS, 8)
        idx.add(x[150_000:])
        D, I = _check(idx, x, q, k, name, normalize)
        st = idx.last_stats()
        assert st["sample_rows"] > 0 and st["n_dense_exact"] == 0, st
        assert st["scan_bytes"] == tiles * 32 * 768 * 17 // 16, st      # 1.0625 bytes per stored value
        if name == "ip" and normalize:
            idx.set_option(OPT_SCAN_BITS, 16)
            D16, I16 = idx.search(q, k)
            assert np.array_equal(I16, I) and np.array_equal(D16, D)
        idx.close()


def test_eight_bit_scan_on_tight_clusters_recovers_or_hands_over_to_f16():
    from anorag_hip import FlatIndex, METRIC_IP
    from anorag_hip._lib import OPT_SCAN_BITS
    rng = np.random.default_rng(11)
    n, d, nq, k = 200_000, 256, 64, 50
    cent = rng.standard_normal((300, d)).astype(np.float32)
    x = (cent[rng.integers(0, 300, n)] + 0.02 * rng.standard_normal((n, d))).astype(np.float32)
    q = (cent[rng.integers(0, 300, nq)] + 0.02 * rng.standard_normal((nq, d))).astype(np.float32)
    idx = FlatIndex(d, METRIC_IP, normalize=True)
    idx.add(x)
    idx.set_option(OPT_SCAN_BITS, 8)
    seen = []
    for _ in range(14):
        _check(idx, x, q, k, "ip", True)
        st = idx.last_stats()
        seen.append((st["scan_bytes"], st["n_fallback"]))
    tiles = -(-n // 32)
    b8, b16 = tiles * 32 * 256 * 17 // 16, tiles * 32 * 256 * 2
    # every answer above was exact; the index either found a K' at which most certificates hold on the 8-bit image, or
    # went back to the f16 image after two batches that failed at the top of the ladder
    assert seen[0][0] == b8 and seen[-1][0] in (b8, b16), seen
    assert seen[-1][0] == b16 or seen[-1][1] < nq // 2, seen
    idx.close()


def test_eight_bit_scan_pipelined_batches_equal_the_sixteen_bit_ones():
    import torch
    from anorag_hip import FlatIndex, METRIC_IP
    from anorag_hip._lib import OPT_SCAN_BITS
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    n, d, nb, B, k = 400_000, 768, 9, 64, 100
    idx = FlatIndex(d, METRIC_IP, normalize=True)
    idx.reserve(n)
    for _ in range(4):
        xb = torch.randn((n // 4, d), generator=g, device=dev)
        torch.cuda.synchronize()
        idx.add_device(xb.data_ptr(), xb.shape[0])
    Q = torch.randn((nb, B, d), generator=g, device=dev)
    out = {}
    for bits in (16, 8):
        idx.set_option(OPT_SCAN_BITS, bits)
        D = torch.empty((nb, B, k), device=dev)
        I = torch.empty((nb, B, k), device=dev, dtype=torch.int64)
        torch.cuda.synchronize()
        for b in range(nb):
            idx.search_device_async(Q[b].data_ptr(), B, k, D[b].data_ptr(), I[b].data_ptr(), 0)
        idx.sync()
        torch.cuda.synchronize()
        out[bits] = (D.cpu().numpy(), I.cpu().numpy())
    assert np.array_equal(out[8][1], out[16][1])
    assert np.array_equal(out[8][0], out[16][0])
    idx.close()
