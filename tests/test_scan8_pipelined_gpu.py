"""The 8-bit scan's k-loop carries the decoded operand of the coming k-block from one k-block to the next, over chunk and tile
boundaries (csrc/index_kernels.hpp, ScanChunk8::Pipe; DESIGN.md §4 "Round 16").  An operand paired with the wrong scale, the
wrong B block or the previous tile's leftovers must show, so: corpora that really stream the 8-bit image with non-temporal
loads (the smallest that do), at every chunk form and trip count, with more tiles than the 3 072 waves and no multiple of
them (waves that hand over from tile to tile and waves that re-request their last chunk because no tile follows, in the
164 000-row cases about 1 000 waves with a single tile), group scales that differ by powers of two wherever the loop could
mix two of them up, and queries weighted per k-block.  Held to the bar of tests/magnitude_cases.py: ids equal the float64
oracle's position by position, scores to one float32 spacing; NO certificate fails — a failed one is recovered from the f16
image, which would hide a k_scan8 whose scores are garbage — and no query takes the dense exact path; the f16 image gives the
same bits.  (The seeds are chosen so that this holds for the unpipelined loop as well.)  A wave without any tile does not
occur in a scan of the 8-bit image under the default options: the image is scanned only from 1 024 tiles on (eight samples of at least 128 tiles),
and from 1 024 tiles on launch_scan gives every wave of its grid a tile."""
import functools

import numpy as np
import pytest

import magnitude_cases as mc
from oracle import flat_index as orc

pytestmark = pytest.mark.gpu

K = 100
# name -> (rows, dim): kb = dimp / 16 k-blocks; kb % 16 == 0 runs chunks of eight k-blocks, else of four (two per granule)
CASES = {
    "kb48_ch8_three_trips": (164_000, 768),
    "kb48_ch8_ragged_last_tile": (164_000 + 7, 768),
    "kb16_ch8_one_trip": (530_000, 256),          # the prologue feeds the epilogue directly
    "kb24_ch4_three_trips": (270_000, 384),
}
SEED = {"kb48_ch8_three_trips": 11, "kb48_ch8_ragged_last_tile": 12, "kb16_ch8_one_trip": 13, "kb24_ch4_three_trips": 14}
SCAN_WAVES = 3072                                 # 256 workgroups of 12 waves


def _exponents(n, groups):
    """the power of two of row r's group g (32 dimensions = one pair of k-blocks = one scale): differs between neighbouring
    pairs (also over a granule's edge), between the two scales of one word, between a pair and the same pair of the next
    chunk and granule, between rows r and r +- 1, and between a row and the same lane's row of the wave's previous tile"""
    r = np.arange(n, dtype=np.int64)[:, None]
    g = np.arange(groups, dtype=np.int64)[None, :]
    return (3 * g + (g >> 2) + 7 * r + 2 * (r >> 5)) % 5 - 2


@functools.lru_cache(maxsize=1)
def _data(name):
    n, d = CASES[name]
    rng = np.random.default_rng(SEED[name])
    groups = d // 32
    x = rng.random((n, groups, 32), dtype=np.float32)
    x *= 2.0
    x -= 1.0
    x[:, :, 5] = 1.0                              # the group's absmax, exactly
    x *= np.exp2(_exponents(n, groups)).astype(np.float32)[:, :, None]
    x = x.reshape(n, d)
    # every k-block (16 dimensions) of a query has its own weight: a B block in the wrong place changes every score
    w = 1.0 + (np.arange(d) // 16) / np.float32(d // 16)
    q = rng.standard_normal((64, d), dtype=np.float32) * w.astype(np.float32)[None, :]
    return x, np.ascontiguousarray(q)


@functools.lru_cache(maxsize=2)
def _reference(name, metric):
    """(Dr, Ir, s64) of the 64 queries, and the number of queries check_exact may ever have to excuse (from the oracle alone)"""
    x, q = _data(name)
    if metric == "ip":
        s64 = orc.exact_scores(q, x, "ip")
    else:
        # the oracle's direct form sum((q - x)^2) costs most of a minute here: float64 ||q||^2 + ||x||^2 - 2 q.x for every row
        # (off by ~1e-12 at distances of ~1e3, against a float32 spacing of 2e-4), the direct form for each query's best 2 000
        q64 = q.astype(np.float64)
        s64 = np.empty((q.shape[0], x.shape[0]))
        for at in range(0, x.shape[0], 65536):
            xb = x[at:at + 65536].astype(np.float64)
            s64[:, at:at + 65536] = (q64 * q64).sum(axis=1)[:, None] + (xb * xb).sum(axis=1)[None, :] - 2.0 * (q64 @ xb.T)
        for i in range(q.shape[0]):
            best = np.argpartition(s64[i], 2000)[:2000]
            s64[i, best] = orc.exact_scores(q[i:i + 1], x[best], "l2")[0]
    Dr, Ir = orc.flat_search(q, x, K, metric, scores=s64)
    return (Dr, Ir, s64), mc.near_tie_queries(s64, K, metric)[0]


def test_the_scales_differ_wherever_the_loop_could_mix_them_up():
    e = _exponents(SCAN_WAVES * 32 + 64, 24)
    assert (e[:, 1:] != e[:, :-1]).all()          # neighbouring pairs, the two halves of a scale word, a granule's edge
    assert (e[:, 2:] != e[:, :-2]).all()          # the same pair of the next chunk of four k-blocks
    assert (e[:, 4:] != e[:, :-4]).all()          # ... of the next granule / chunk of eight
    assert (e[1:] != e[:-1]).all()                # rows r and r + 1
    assert (e[32:] != e[:-32]).all()              # the same lane's row of the next tile
    assert (e[SCAN_WAVES * 32:] != e[:-SCAN_WAVES * 32]).all()   # ... of the wave's own next tile
    assert e.min() == -2 and e.max() == 2


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_pipelined_scan_gives_the_exact_top_k(name, metric):
    from anorag_hip import FlatIndex, METRIC_IP, METRIC_L2
    from anorag_hip._lib import OPT_SCAN_BITS, OPT_TINY
    x, q = _data(name)
    (Dr, Ir, s64), may_excuse = _reference(name, metric)
    n, d = x.shape
    tiles, dimp = -(-n // 32), -(-d // 128) * 128
    assert tiles > SCAN_WAVES and tiles % SCAN_WAVES   # some waves own one tile more than the others; every wave owns one
    assert tiles * (dimp // 16) * 1024 > 192 << 20, "too small for the streaming (non-temporal) pass"
    idx = FlatIndex(d, METRIC_IP if metric == "ip" else METRIC_L2, normalize=False)
    idx.set_option(OPT_TINY, 0)                   # the one-query batch takes the pipeline too
    idx.set_option(OPT_SCAN_BITS, 8)
    idx.reserve(n)
    idx.add(x)
    out = {}
    for bits in (8, 16):
        idx.set_option(OPT_SCAN_BITS, bits)
        for nq in (64, 1):                        # one query: 63 ladders of +inf beside it
            D, I = idx.search(q[:nq], K)
            st = idx.last_stats()
            print(f"{name} {metric} bits {bits} nq {nq}: failed certificates {st['n_fallback']}, dense exact "
                  f"{st['n_dense_exact']}, candidates {st['n_candidates']}, K' {st['overfetch']}, scan bytes {st['scan_bytes']}")
            assert st["n_fallback"] == 0 and st["n_dense_exact"] == 0, st   # every answer rests on this scan's own scores
            assert st["scan_bytes"] == tiles * 32 * dimp * (17 if bits == 8 else 32) // 16, st   # the image that was streamed
            excused = mc.check_exact(D, I, None, None, K, metric, False, ref=(Dr[:nq], Ir[:nq], s64[:nq]))
            assert excused <= may_excuse, (excused, may_excuse)
            out[bits, nq] = (D, I)
    idx.close()
    for nq in (64, 1):
        assert np.array_equal(out[8, nq][1], out[16, nq][1]) and np.array_equal(out[8, nq][0], out[16, nq][0]), nq
