"""The exact flat index on the device against the oracle, away from unit-scale Gaussian data: the magnitude sweep of
tests/magnitude_cases.py through every scan image (16, 12, 8 bits) and every search path, held to the scale-free bar of
magnitude_cases.check_exact (ids position by position, scores to one float32 spacing; the excuse caps are conditions on the
inputs that tests/test_index_magnitudes_cpu.py checks from the oracle alone).  Path assertions come from last_stats(), not
from timing; the share of failed certificates and the K' reached are recorded per case (record_property), not asserted."""
import numpy as np
import pytest

import magnitude_cases as mc
import scan_image8 as s8
from oracle import flat_index as orc

pytestmark = pytest.mark.gpu

BITS = (16, 12, 8)


def _index(name, bits=None, n_rows=0, options=()):
    from anorag_hip import FlatIndex, METRIC_IP, METRIC_L2
    from anorag_hip._lib import OPT_SCAN_BITS
    x, q, metric, normalize, k = mc.case(name)
    if n_rows:
        x = x[:n_rows]
    idx = FlatIndex(x.shape[1], METRIC_IP if metric == "ip" else METRIC_L2, normalize=normalize)
    for opt, value in options:
        idx.set_option(opt, value)
    if bits is not None:
        idx.set_option(OPT_SCAN_BITS, bits)      # before the add: k_add writes the image
    idx.add(x)
    return idx, x, q, k


def _assert_path(name, st, nq, out_of_range_queries):
    if name in mc.ROWS_OUT_OF_RANGE:
        # a stored value beyond +-65504: no image is trusted, every query is answered by the exact path
        assert st["n_fallback"] == nq and st["n_dense_exact"] == nq, st
        assert st["sample_rows"] == 0 and st["scan_bytes"] == 0 and st["n_candidates"] == 0, st
    else:
        assert st["scan_bytes"] > 0, st          # the scan ran
        if name in mc.QUERIES_OUT_OF_RANGE:
            # the dense exact path answers the queries whose f16 image is not finite (eps = inf or NaN, hence no theta),
            # and on this Gaussian corpus no other
            assert st["n_dense_exact"] == out_of_range_queries and st["n_overflow"] == 0, st
            assert st["n_fallback"] >= out_of_range_queries, st


def _record(record_property, st, nq):
    record_property("failed_certificates", f"{st['n_fallback']}/{nq}")
    record_property("overfetch", st["overfetch"])
    record_property("n_dense_exact", st["n_dense_exact"])
    print(f"failed certificates {st['n_fallback']}/{nq}, K' {st['overfetch']}, dense exact {st['n_dense_exact']}, "
          f"from lists {st['n_from_lists']}")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", mc.NAMES)
def test_every_scan_image_gives_the_exact_top_k(name, bits, record_property):
    from anorag_hip._lib import OPT_TINY
    idx, x, q, k = _index(name, bits, options=((OPT_TINY, 0),))
    D, I = idx.search(q, k)
    st = idx.last_stats()
    _record(record_property, st, len(q))
    if mc.case(name)[3] and bits == 16:          # cosine: the stored rows are the ones the oracle ranks, bit for bit
        assert idx.reconstruct_n(0, 4096).tobytes() == mc.preprocess(x[:4096], True).tobytes()
    record_property("excused_queries", mc.check_case(name, D, I))
    _assert_path(name, st, len(q), len(mc.OUT_OF_RANGE_QUERIES) if name in mc.QUERIES_OUT_OF_RANGE else 0)
    if name not in mc.ROWS_OUT_OF_RANGE and bits != 16:
        dimp = -(-x.shape[1] // 128) * 128
        per_value = {12: 1.5, 8: 1.0625}[bits]
        assert st["scan_bytes"] in (-(-len(x) // 32) * 32 * dimp * per_value, -(-len(x) // 32) * 32 * dimp * 2), st
    D2, I2 = idx.search(q, k)                     # a second batch (K' may have adapted): the same bits
    assert np.array_equal(I2, I) and np.array_equal(D2, D)
    idx.close()


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_default_image_and_the_other_search_paths(name, record_property):
    """the image the index picks by itself (12 bits from 262 144 rows on), the three-launch post-processing
    (ANR_OPT_FUSED_POST 0: k_finalize instead of k_post, identical bits), the single-launch path (ANR_OPT_TINY 2, 4 queries,
    on the first 20 000 rows) and k = 2000 on those rows (the device sort)"""
    from anorag_hip._lib import OPT_FUSED_POST, OPT_TINY
    idx, x, q, k = _index(name, options=((OPT_TINY, 0), (OPT_FUSED_POST, 2)))
    D, I = idx.search(q, k)
    st = idx.last_stats()
    _record(record_property, st, len(q))
    mc.check_case(name, D, I)
    if len(x) >= 262_144 and name not in mc.ROWS_OUT_OF_RANGE:
        assert st["scan_bytes"] == len(x) * 128 * 3 // 2, st     # the 12-bit image by default
    idx.set_option(OPT_FUSED_POST, 0)
    D0, I0 = idx.search(q, k)
    st0 = idx.last_stats()
    assert np.array_equal(I0, I) and np.array_equal(D0, D)
    assert st0["n_dense_exact"] == st["n_dense_exact"], (st0, st)
    idx.close()
    idx, x, q, k = _index(name, n_rows=20_000, options=((OPT_TINY, 0),))
    Dp, Ip = idx.search(q[:4], k)
    idx.set_option(OPT_TINY, 2)
    Dt, It = idx.search(q[:4], k)
    stt = idx.last_stats()
    assert stt["n_dense_exact"] == 4 and stt["n_candidates"] == 0, stt     # the single-launch path ran
    mc.check_case(name, Dt, It, n_rows=20_000, queries=slice(0, 4))
    assert np.array_equal(It, Ip) and np.array_equal(Dt, Dp)
    Dk, Ik = idx.search(q, 2000)
    assert idx.last_stats()["n_dense_exact"] == len(q)
    # (the excuse caps are stated for the best k + 1 = 11 scores; among 2000 neighbours float32 near-ties are ordinary, so
    # here the excuse is bounded by check_exact's two-spacing rule alone, and counted)
    ref = mc.oracle(x, q, 2000, *mc.case(name)[2:4])
    record_property("excused_queries_k2000", mc.check_exact(Dk, Ik, x, q, 2000, *mc.case(name)[2:4], ref=ref))
    idx.close()


@pytest.mark.parametrize("name,bits", [("row_norms_1e-3_to_1e3-ip", 16), ("row_norms_1e-3_to_1e3-l2", 12),
                                       ("tight_band_scaled_2^8-ip", 8), ("tight_band_scaled_2^-10-l2", 16)])
def test_pipelined_batches_whose_certificates_fail_in_bulk(name, bits, record_property):
    """eight batches of 64 in flight on three streams (search_device_async), on corpora where one long row inflates every
    query's eps or where hundreds of rows sit inside it: the recoveries run beside the pipeline and leave the bits of the
    one-batch-at-a-time search, which are the oracle's"""
    import torch
    from anorag_hip._lib import OPT_OVERFETCH
    idx, x, q, k = _index(name, bits, options=((OPT_OVERFETCH, 64),))     # a fixed K': no adaptation between batches
    nb, B = 8, len(q)
    order = [np.roll(np.arange(B), 5 * b) for b in range(nb)]
    dev = torch.device("cuda", 0)
    Q = torch.from_numpy(np.stack([q[o] for o in order])).to(dev)
    ref = []
    for b in range(nb):
        D = torch.empty((B, k), device=dev)
        I = torch.empty((B, k), device=dev, dtype=torch.int64)
        idx.search_device(Q[b].data_ptr(), B, k, D.data_ptr(), I.data_ptr())
        torch.cuda.synchronize()
        ref.append((D.cpu().numpy(), I.cpu().numpy()))
        inv = np.argsort(order[b])
        mc.check_case(name, ref[b][0][inv], ref[b][1][inv])
    idx.reset_stats()
    S = [torch.cuda.Stream() for _ in range(3)]
    Ds = [torch.empty((B, k), device=dev) for _ in range(nb)]
    Is = [torch.empty((B, k), device=dev, dtype=torch.int64) for _ in range(nb)]
    torch.cuda.synchronize()
    for b in range(nb):
        idx.search_device_async(Q[b].data_ptr(), B, k, Ds[b].data_ptr(), Is[b].data_ptr(), S[b % 3].cuda_stream)
    idx.sync()
    torch.cuda.synchronize()
    for b in range(nb):
        assert np.array_equal(Is[b].cpu().numpy(), ref[b][1]) and np.array_equal(Ds[b].cpu().numpy(), ref[b][0]), b
    st = idx.last_stats()
    _record(record_property, st, nb * B)
    assert st["n_overflow"] == 0, st
    idx.close()


def test_the_out_of_range_flag_follows_the_stored_rows():
    """f16_unusable is state: cleared by reset(), raised by a later add — also for a search enqueued right behind that add —
    and a 12- / 8-bit image of such an index is never trusted"""
    import torch
    from anorag_hip import FlatIndex, METRIC_IP
    from anorag_hip._lib import OPT_SCAN_BITS, OPT_TINY
    name = "one_row_out_of_range-ip"
    x, q, metric, normalize, k = mc.case(name)
    bad = 31_337
    assert np.abs(x[bad]).max() > mc.F16_MAX and np.abs(np.delete(x, bad, axis=0)).max() < mc.F16_MAX
    idx = FlatIndex(x.shape[1], METRIC_IP, normalize=False)
    idx.set_option(OPT_TINY, 0)
    idx.add(x[:bad])                              # in range so far
    D, I = idx.search(q, k)
    st = idx.last_stats()
    assert st["scan_bytes"] > 0 and st["n_dense_exact"] == 0, st
    mc.check_exact(D, I, x[:bad], q, k, metric, normalize)
    # the row arrives through the device-pointer surface and a batch is enqueued behind it without a synchronisation
    dev = torch.device("cuda", 0)
    xb = torch.from_numpy(x[bad:]).to(dev)
    Q = torch.from_numpy(q).to(dev)
    Dd = torch.empty((len(q), k), device=dev)
    Id = torch.empty((len(q), k), device=dev, dtype=torch.int64)
    torch.cuda.synchronize()
    idx.reset_stats()
    idx.add_device(xb.data_ptr(), xb.shape[0])
    idx.search_device_async(Q.data_ptr(), len(q), k, Dd.data_ptr(), Id.data_ptr(), 0)
    idx.sync()
    torch.cuda.synchronize()
    st = idx.last_stats()
    assert st["n_dense_exact"] == len(q) and st["scan_bytes"] == 0, st
    assert mc.check_case(name, Dd.cpu().numpy(), Id.cpu().numpy()) == 0
    assert Id[5, 0].item() == bad                 # the query aimed at the long row finds it
    for bits in (12, 8, 16):                      # an image built on a filled, unusable index is not scanned either
        idx.set_option(OPT_SCAN_BITS, bits)
        D, I = idx.search(q, k)
        st = idx.last_stats()
        assert st["n_dense_exact"] == len(q) and st["scan_bytes"] == 0, (bits, st)
        mc.check_case(name, D, I)
    idx.reset()                                   # emptied: the flag goes with the rows
    good = np.delete(x, bad, axis=0)
    idx.add(good)
    D, I = idx.search(q, k)
    st = idx.last_stats()
    assert st["scan_bytes"] > 0 and st["n_dense_exact"] == 0 and st["n_fallback"] < len(q), st
    mc.check_exact(D, I, good, q, k, metric, normalize)
    idx.close()


def test_the_scan_images_of_out_of_range_rows_are_what_the_restatements_say():
    """pinned: reconstruct_scan_image answers on an index whose rows left the f16 range — the f16 and 12-bit images hold an
    infinity where the value overflows, the 8-bit image clamps its code so that the decoded value stays finite — and the
    tracked f16 / 12-bit error norms are infinite (which is moot: such an index scans nothing)"""
    from anorag_hip import FlatIndex, METRIC_IP
    from anorag_hip._lib import OPT_SCAN_BITS
    from anorag_hip._lib import AnoragError
    x = mc.case("one_row_out_of_range-ip")[0][31_000:32_000]
    q = mc.case("one_row_out_of_range-ip")[1]
    for bits in (12, 8):
        idx = FlatIndex(x.shape[1], METRIC_IP, normalize=False)
        idx.set_option(OPT_SCAN_BITS, bits)      # on an empty index the image is built by the first batch that scans it:
        idx.add(x)                               # here none does, and the image is never made
        idx.search(q, 10)
        with pytest.raises(AnoragError, match=f"no {bits}-bit image"):
            idx.reconstruct_scan_image(bits, 0, len(x))
        idx.close()
        idx = FlatIndex(x.shape[1], METRIC_IP, normalize=False)
        idx.add(x[:300])
        idx.set_option(OPT_SCAN_BITS, bits)      # on a filled index: k_build12 / k_build8 now, k_add for the rest
        idx.add(x[300:])
        img16 = idx.reconstruct_scan_image(16, 0, len(x))
        with np.errstate(over="ignore"):
            assert img16.tobytes() == orc.scan_image(x, 16).tobytes()
        assert np.isinf(img16[337, 3:7]).all() and np.isfinite(np.delete(img16, 337, axis=0)).all()
        img = idx.reconstruct_scan_image(bits, 0, len(x))
        with np.errstate(over="ignore"):
            ref = orc.scan_image(x, 12) if bits == 12 else s8.decode(x)
        assert img.tobytes() == ref.tobytes(), bits
        st = idx.scan_image_stats()
        assert np.isinf(st["max_err16"]), st
        if bits == 12:
            assert np.isinf(st["max_err12"]), st
        else:
            assert np.isfinite(img).all() and np.isfinite(st["max_err8"]), st
            true = s8.error_norm(x)
            assert true <= st["max_err8"] <= true * 1.0003 + 1e-12, (true, st)
        idx.close()


@pytest.mark.parametrize("scale", [2.0 ** -20, 2.0 ** -14])
def test_the_scan_images_of_a_subnormal_corpus_equal_the_restatements(scale):
    """a whole corpus whose f16 image is subnormal (2^-20: every value; 2^-14: most) and whose 8-bit group scales are
    subnormal f16 values: the three images bit for bit the restatements, the tracked error norms theirs — so neither the
    f16 conversion nor the packed-f16 multiply of x8_operand flushes subnormals"""
    from anorag_hip import FlatIndex, METRIC_IP
    from anorag_hip._lib import OPT_SCAN_BITS
    n, d = 6_000, 100
    x = np.random.default_rng(3).standard_normal((n, d), dtype=np.float32) * np.float32(scale)
    assert (np.abs(x.astype(np.float16)) < 6.1e-5).mean() > 0.6 and (s8.scales(x).astype(np.float32) < 6.1e-5).all()
    for bits in (12, 8):
        idx = FlatIndex(d, METRIC_IP, normalize=False)
        idx.add(x[:3000])
        idx.set_option(OPT_SCAN_BITS, bits)      # k_build12 / k_build8 for the rows so far, k_add for the rest
        idx.add(x[3000:])
        stored = idx.reconstruct_n(0, n)
        assert stored.tobytes() == x.tobytes()
        assert idx.reconstruct_scan_image(16, 0, n).tobytes() == orc.scan_image(x, 16).tobytes()
        ref = orc.scan_image(x, 12) if bits == 12 else s8.decode(x)
        assert idx.reconstruct_scan_image(bits, 0, n).tobytes() == ref.tobytes(), bits
        st = idx.scan_image_stats()
        true = {16: orc.scan_image_error(x, 16), 12: orc.scan_image_error(x, 12), 8: s8.error_norm(x)}
        assert true[16] > 0 and true[16] <= st["max_err16"] <= true[16] * 1.0003, (true, st)
        key = "max_err12" if bits == 12 else "max_err8"
        assert true[bits] <= st[key] <= true[bits] * 1.0003, (bits, true, st)
        norm = float(np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)).max())
        assert norm <= st["max_norm"] <= norm * 1.0003
        idx.close()


@pytest.mark.parametrize("name", ["scale_2^8-ip", "integers_0_255_d128-ip", "row_norms_1e-3_to_1e3-ip"])
def test_self_join_at_other_magnitudes(name):
    """raw inner-product self join of the first 3000 rows at the median pair score (half of the 4.5 M pairs qualify): the
    oracle's pair set, modulo pairs within two float32 spacings of the threshold, and float32(float64 sum) scores to one
    spacing"""
    n = 3000
    idx, x, q, k = _index(name, n_rows=n)
    s64 = x.astype(np.float64) @ x.astype(np.float64).T
    iu = np.triu_indices(n, 1)
    thr = float(np.float32(np.median(s64[iu])))
    I, J, S = idx.self_join(thr)
    idx.close()
    assert np.all(I < J)
    got = np.zeros((n, n), dtype=bool)
    got[I, J] = True
    assert got.sum() == len(I), "a pair is listed twice"
    want = np.triu(s64 >= thr, 1)
    near = np.abs(s64 - thr) <= 2.0 * float(np.spacing(np.float32(abs(thr))))
    assert not ((got != want) & ~near).any(), "pair sets differ beyond the threshold's own float32 spacing"
    assert abs(int(got.sum()) - len(iu[0]) // 2) <= len(iu[0]) // 100 + int(near.sum())    # the threshold sits in the middle
    ref = s64[I, J].astype(np.float32)
    assert np.all(np.abs(S.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64))


def test_self_join_refuses_an_index_beyond_the_f16_range():
    from anorag_hip._lib import AnoragError
    idx, x, q, k = _index("one_row_out_of_range-ip", n_rows=32_000)
    with pytest.raises(AnoragError, match="exceed the f16 range"):
        idx.self_join(0.5)
    idx.close()
