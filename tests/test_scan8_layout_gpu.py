"""The 8-bit scan image's tile layout (granules of eight k-blocks: codes, then their scales; csrc/index_kernels.hpp at
kX8TileBytesPerKb): whatever k_add / k_build8 write and k_image_rows / k_scan8 read must agree on where a row's codes and
scales sit.  The image decoded through reconstruct_scan_image equals the numpy restatement (tests/scan_image8.py) bit for bit
at every row count, width and writer, with scales that tell a wrong row, granule or half apart; searches through the
8-bit image return the ids and scores of the f16 image position by position."""
import numpy as np
import pytest

import scan_image8 as s8

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 31, 32, 33, 1000)
GROW_BY = 1100          # storage starts at 1024 rows: any of ROW_COUNTS + 1100 needs a larger one


def _rows(rng, n, d):
    """Gaussian rows whose 32-dimension groups differ in magnitude by row and by group, so no two scales of a tile agree"""
    x = rng.standard_normal((n, d)).astype(np.float32)
    g = np.arange(d) // 32
    x *= np.exp2(((g[None, :] * 3 + np.arange(n)[:, None] * 5) % 13) - 6).astype(np.float32)
    return x


def _check_image(idx, x):
    n = x.shape[0]
    assert idx.ntotal == n
    stored = idx.reconstruct_n(0, n)
    assert stored.tobytes() == x.tobytes()
    img = idx.reconstruct_scan_image(8, 0, n)
    ref = s8.decode(stored)
    assert img.tobytes() == ref.tobytes()
    st = idx.scan_image_stats()
    assert st["bits"] == 8
    true = s8.error_norm(stored)
    assert true <= st["max_err8"] <= true * 1.0003 + 1e-12, (true, st["max_err8"])


def _filled(x, writer):
    """an index holding x with its 8-bit image written by `writer`"""
    from anorag_hip import FlatIndex, METRIC_IP
    from anorag_hip._lib import OPT_SCAN_BITS
    idx = FlatIndex(x.shape[1], METRIC_IP, normalize=False)
    if writer == "build8":
        idx.add(x)
        idx.set_option(OPT_SCAN_BITS, 8)          # k_build8 over the stored rows
        return idx
    idx.reserve(1)
    idx.set_option(OPT_SCAN_BITS, 8)              # the image exists before the rows: k_add writes it
    if writer == "appends":                       # 7 + 30 + the rest: continue inside a partly filled tile, cross its edge
        at = 0
        for m in (7, 30, x.shape[0]):
            m = min(m, x.shape[0] - at)
            if m > 0:
                idx.add(x[at:at + m])
            at += m
    else:
        idx.add(x)
    return idx


@pytest.mark.parametrize("writer", ["one_add", "appends", "build8", "grow"])
@pytest.mark.parametrize("d", [32, 100, 128, 136, 768])          # kb = 8, 8, 8, 16, 48; 100 and 136 pad their last group
def test_the_image_equals_the_restatement_at_every_row_count(d, writer):
    rng = np.random.default_rng(1000 + d)
    x = _rows(rng, max(ROW_COUNTS) + GROW_BY, d)
    for n in ROW_COUNTS:
        idx = _filled(x[:n], "one_add" if writer == "grow" else writer)
        _check_image(idx, x[:n])
        if writer == "grow":
            idx.add(x[n:n + GROW_BY])             # a larger storage: the tiles so far are copied, the add continues in them
            _check_image(idx, x[:n + GROW_BY])
        idx.close()


def _distinct_scale_rows(n, d, rng):
    """row r's group g has absmax 2^((g + 7 r) mod 24 - 8) exactly: every scale of a row differs from the row's others by a
    power of two, and from the same group's scale in the rows before and after"""
    groups = -(-d // 32)
    e = (np.arange(groups)[None, :] + 7 * np.arange(n)[:, None]) % 24 - 8
    x = rng.uniform(-1.0, 1.0, (n, groups, 32)).astype(np.float32)
    x[:, :, 5] = 1.0
    x *= np.exp2(e).astype(np.float32)[:, :, None]
    return np.ascontiguousarray(x.reshape(n, groups * 32)[:, :d])


@pytest.mark.parametrize("writer", ["one_add", "appends", "build8"])
@pytest.mark.parametrize("d", [768, 128, 136])
def test_a_scale_from_the_wrong_row_granule_or_half_shows(d, writer):
    rng = np.random.default_rng(7)
    n = 100                                        # three full tiles and a ragged one
    x = _distinct_scale_rows(n, d, rng)
    s = s8.scales(x).astype(np.float32)
    full = d // 32                                 # groups that hold dimension 5 of their 32
    for r in range(n):
        assert len(set(s[r, :full].tolist())) == full
        if r:
            assert (s[r, :full] != s[r - 1, :full]).all()
    ratio = s[:, 1:full] / s[:, :full - 1]
    assert ((ratio >= 1.99) | (ratio <= 0.51)).all()
    idx = _filled(x, writer)
    _check_image(idx, x)
    idx.close()


def _corpus(n, d, duplicate):
    rng = np.random.default_rng(40_000 + d + (1 if duplicate else 0))
    x = rng.standard_normal((n, d), dtype=np.float32)
    q = rng.standard_normal((4, 64, d), dtype=np.float32)
    if duplicate:
        x[n // 2 + 17] = x[123]                    # an exact duplicate pair ...
        q[:, 0] = x[123] + 0.05 * q[:, 0]          # ... that leads query 0 of every batch
    return x, q


def _search_all(idx, q, nq, k):
    """three pipelined batches and one synchronous one: (scores [4, nq, k], ids [4, nq, k], scan_bytes of the last)"""
    import torch
    dev = torch.device("cuda", 0)
    Q = torch.from_numpy(np.ascontiguousarray(q[:3, :nq])).to(dev)
    D = torch.empty((3, nq, k), device=dev)
    I = torch.empty((3, nq, k), device=dev, dtype=torch.int64)
    torch.cuda.synchronize()
    for b in range(3):
        idx.search_device_async(Q[b].data_ptr(), nq, k, D[b].data_ptr(), I[b].data_ptr(), 0)
    idx.sync()
    torch.cuda.synchronize()
    Ds, Is = idx.search(q[3, :nq], k)
    st = idx.last_stats()
    return (np.concatenate([D.cpu().numpy(), Ds[None]]), np.concatenate([I.cpu().numpy(), Is[None]]), st["scan_bytes"])


def _bits8_equals_bits16(n, d, duplicate, first, expect_x8_scanned):
    from anorag_hip import FlatIndex, METRIC_IP
    from anorag_hip._lib import OPT_SCAN_BITS
    x, q = _corpus(n, d, duplicate)
    idx = FlatIndex(d, METRIC_IP, normalize=True)
    idx.reserve(n)
    out = {}
    order = (8, 16) if first == 8 else (16, 8)     # 8 first: k_add writes the image; 16 first: k_build8 does
    idx.set_option(OPT_SCAN_BITS, order[0])
    idx.add(x)
    for bits in order:
        idx.set_option(OPT_SCAN_BITS, bits)
        out[bits] = {(nq, k): _search_all(idx, q, nq, k) for nq in (64, 3) for k in (10, 100)}
    idx.close()
    tiles, dimp = -(-n // 32), -(-d // 128) * 128
    for key in out[16]:
        D16, I16, b16 = out[16][key]
        D8, I8, b8 = out[8][key]
        assert np.array_equal(I8, I16), key
        assert np.array_equal(D8, D16), key
        if expect_x8_scanned and key[0] == 64:     # (a batch of a few queries may take a path without a streaming pass)
            assert b16 == tiles * 32 * dimp * 2, (key, b16)
            assert b8 == tiles * 32 * dimp * 17 // 16, (key, b8)   # 1.0625 bytes per stored value: the 8-bit image
    if duplicate:
        I = out[8][(64, 10)][1]
        assert sorted(I[0, 0, :2].tolist()) == [123, n // 2 + 17]


@pytest.mark.parametrize("d,duplicate", [(768, False), (136, False), (768, True)])
def test_search_through_the_eight_bit_image_equals_the_f16_one(d, duplicate):
    """40 000 rows: 64 and 3 queries, k = 10 and 100, three pipelined batches and a synchronous one per combination.  (At
    this size a batch forced to 8 bits may still run from the f16 image — a corpus of fewer than eight samples does — so the
    test below repeats the comparison where the 8-bit image is the one scanned.)"""
    _bits8_equals_bits16(40_000, d, duplicate, first=16, expect_x8_scanned=False)


@pytest.mark.parametrize("d,first", [(768, 8), (136, 16), (320, 8), (100, 16)])
def test_search_streams_the_eight_bit_image_and_equals_the_f16_one(d, first):
    """164 000 rows is the smallest corpus whose k = 100 batches stream the 8-bit image (5 120 full tiles = eight samples
    of 2 K' = 640 tiles); kb = 48 and 16 take chunks of eight k-blocks (three loop rounds, and one: only the hand-over to
    the next tile), kb = 24 and 8 chunks of four (two per granule)"""
    _bits8_equals_bits16(164_000, d, d == 768, first=first, expect_x8_scanned=True)
