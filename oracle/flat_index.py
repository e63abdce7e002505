"""ORACLE — test infrastructure only (never imported by the product path).

CPU restatement of the reference's exact dense search, vector_store/vector_index.py:
  * ``preprocess_vectors``  follows ``VectorIndex._preprocess_vectors`` (:265-282): float32 cast,
    C-contiguous, and for cosine ``v / where(norm == 0, 1, norm)`` with numpy's float32 norm;
  * ``flat_search``         restates what ``self.index.search(q, top_k)`` (:223) returns for
    ``index_type == 'Flat'`` (:77-80): faiss ``IndexFlatIP`` / ``IndexFlatL2`` — a third-party library
    (``faiss-cpu>=1.7.4`` / ``faiss-gpu-cu12>=1.7.4``, requirements.txt:9-10, not vendored, not
    installable here).  Published semantics restated: exact float32 inner product (larger first) or
    squared L2 (smaller first), best-first, ``-1`` ids when fewer than k rows exist;
  * ``shape_results``       follows the result loop of ``VectorIndex.search`` (:226-259).

PARITY UNPINNED at the faiss boundary: the reference holds no golden vector, fixture or test for this
call and faiss cannot be run here.  Ranking is arbitrated in float64 (the value
both faiss's float32 sgemm and this build's exact re-score approximate); ties go to the lower id.
"""
from __future__ import annotations

import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)


def preprocess_vectors(vectors: np.ndarray, similarity_metric: str = "cosine") -> np.ndarray:
    """vector_index.py:265-282."""
    if vectors.dtype != np.float32:
        vectors = vectors.astype(np.float32)
    if not vectors.flags["C_CONTIGUOUS"]:
        vectors = np.ascontiguousarray(vectors)
    if similarity_metric == "cosine":
        norms = np.linalg.norm(vectors, axis=1, keepdims=True)
        norms = np.where(norms == 0, 1, norms)
        vectors = vectors / norms
    return vectors


def exact_scores(q: np.ndarray, x: np.ndarray, metric: str = "ip", block: int = 65536) -> np.ndarray:
    """float64-accumulated scores of float32 inputs, [nq, n]; 'ip' or 'l2' (squared distance)."""
    q64 = q.astype(np.float64)
    out = np.empty((q.shape[0], x.shape[0]), dtype=np.float64)
    for s in range(0, x.shape[0], block):
        xb = x[s:s + block].astype(np.float64)
        if metric == "ip":
            out[:, s:s + block] = q64 @ xb.T
        else:
            # direct form, no cancellation
            d = q64[:, None, :] - xb[None, :, :] if xb.shape[0] * q.shape[0] * q.shape[1] < 2e8 else None
            if d is not None:
                out[:, s:s + block] = np.einsum("qnd,qnd->qn", d, d)
            else:
                for i in range(q.shape[0]):
                    dd = xb - q64[i]
                    out[i, s:s + block] = np.einsum("nd,nd->n", dd, dd)
    return out


def flat_search(q: np.ndarray, x: np.ndarray, k: int, metric: str = "ip", scores: np.ndarray | None = None):
    """Exact top-k of preprocessed float32 rows: returns (D float32 [nq,k], I int64 [nq,k]).

    Order: best first; ties by ascending id; padding id -1 with the neutral score of faiss's heaps
    (-FLT_MAX for IP, +FLT_MAX for L2).  `scores`: exact_scores(q, x, metric) where the caller already holds it.
    """
    nq, n = q.shape[0], x.shape[0]
    D = np.full((nq, k), -FLT_MAX if metric == "ip" else FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    if n == 0 or nq == 0:
        return D, I
    s = exact_scores(q, x, metric) if scores is None else scores
    s32 = s.astype(np.float32)  # the value reported (correctly rounded float32)
    kk = min(k, n)
    for i in range(nq):
        key = -s32[i].astype(np.float64) if metric == "ip" else s32[i].astype(np.float64)
        if kk < n:
            part = np.argpartition(key, kk - 1)[:kk]
            kth = key[part].max()
            cand = np.nonzero(key <= kth)[0]  # include every tie of the k-th value
        else:
            cand = np.arange(n)
        order = np.lexsort((cand, key[cand]))[:kk]
        sel = cand[order]
        I[i, :kk] = sel
        D[i, :kk] = s32[i, sel]
    return D, I


class BlockedTopK:
    """Streaming form of ``flat_search`` for corpora that are generated / loaded block by block (bench.py's recall
    leg at 10 M rows, the large parity tests): feed preprocessed float32 row blocks with ``push``; per block a
    float32 sgemm nominates every row within ``margin`` of the block's k-th best score, the nominees are re-scored
    with float64 accumulation (the arbiter, as in ``flat_search``) and merged into the running top-k
    (score desc / distance asc, ties by ascending id)."""

    def __init__(self, q: np.ndarray, k: int, metric: str = "ip", margin: float = 1e-4):
        self.q = np.ascontiguousarray(q, dtype=np.float32)
        self.q64 = self.q.astype(np.float64)
        self.k, self.metric, self.margin = int(k), metric, float(margin)
        nq = self.q.shape[0]
        self.S = np.zeros((nq, 0), dtype=np.float64)
        self.I = np.zeros((nq, 0), dtype=np.int64)

    def push(self, xb: np.ndarray, row0: int) -> None:
        n = xb.shape[0]
        if n == 0:
            return
        if self.metric == "ip":
            s = self.q @ xb.T
        else:
            s = -((self.q * self.q).sum(1)[:, None] - 2.0 * (self.q @ xb.T) + (xb * xb).sum(1)[None, :])
        kk = min(self.k, n)
        newS, newI = [], []
        for i in range(self.q.shape[0]):
            if kk < n:
                part = np.argpartition(-s[i], kk - 1)[:kk]
                cand = np.nonzero(s[i] >= s[i][part].min() - self.margin)[0]
            else:
                cand = np.arange(n)
            xc = xb[cand].astype(np.float64)
            if self.metric == "ip":
                e = xc @ self.q64[i]
            else:
                d = xc - self.q64[i]
                e = -np.einsum("nd,nd->n", d, d)
            newS.append(e)
            newI.append(cand.astype(np.int64) + int(row0))
        for i in range(self.q.shape[0]):
            S = np.concatenate([self.S[i], newS[i]]) if self.S.shape[1] else newS[i]
            I = np.concatenate([self.I[i], newI[i]]) if self.I.shape[1] else newI[i]
            # ranking on the float32-rounded value reported, ties by id — the order flat_search uses
            order = np.lexsort((I, -S.astype(np.float32).astype(np.float64)))[: self.k]
            newS[i], newI[i] = S[order], I[order]
        width = max(len(v) for v in newS)
        self.S = np.full((len(newS), width), -np.inf)
        self.I = np.full((len(newS), width), -1, dtype=np.int64)
        for i in range(len(newS)):
            self.S[i, : len(newS[i])] = newS[i]
            self.I[i, : len(newI[i])] = newI[i]

    def result(self):
        """(scores float64 [nq, <=k] — inner products, or MINUS squared distances for 'l2' — and ids int64)"""
        return self.S, self.I


def near_tie_equal(I_a: np.ndarray, I_ref: np.ndarray, scores64: np.ndarray, k: int, tol: float) -> bool:
    """True when the id sets agree up to rows whose exact score is within `tol` of the k-th best."""
    for i in range(I_ref.shape[0]):
        a = set(int(v) for v in I_a[i] if v >= 0)
        b = set(int(v) for v in I_ref[i] if v >= 0)
        if a == b:
            continue
        kth = np.sort(scores64[i])[::-1][min(k, scores64.shape[1]) - 1]
        for r in a ^ b:
            if abs(scores64[i, r] - kth) > tol:
                return False
    return True


def shape_results(D: np.ndarray, I: np.ndarray, similarity_metric: str = "cosine"):
    """vector_index.py:226-259: list-of-dicts, -1 ids dropped, flat list for a single query."""
    results = []
    for qi in range(D.shape[0]):
        qr = []
        for rank in range(D.shape[1]):
            idx = I[qi][rank]
            score = D[qi][rank]
            if idx == -1:
                continue
            r = {"index": int(idx), "score": float(score), "rank": rank}
            r["similarity"] = float(score) if similarity_metric == "cosine" else 1.0 / (1.0 + float(score))
            qr.append(r)
        results.append(qr)
    if len(results) == 1:
        return results[0]
    return results


def scan_image(x32: np.ndarray, bits: int = 12) -> np.ndarray:
    """The image of stored float32 rows that the device's streaming scan reads (test infrastructure: restates
    csrc/index_kernels.hpp f16_to_12 / k_add, nothing in the reference — faiss scans float32; the image only NOMINATES
    candidates, the float32 rows decide).  bits = 16: the rows rounded to float16 (round-to-nearest-even).  bits = 12: that
    float16 rounded again, to nearest-even, to its top 12 bits (sign, 5 exponent bits, 6 mantissa bits); a value that would
    round up to infinity is truncated instead.  Returned as float32."""
    h = np.asarray(x32, dtype=np.float32).astype(np.float16)
    if bits == 16:
        return h.astype(np.float32)
    if bits != 12:
        raise ValueError("bits must be 12 or 16")
    b = h.view(np.uint16).astype(np.uint32)
    r = (b + 7 + ((b >> 4) & 1)) >> 4
    would_overflow = ((r & 0x7C0) == 0x7C0) & ((b & 0x7C00) != 0x7C00)
    r = np.where(would_overflow, b >> 4, r) & 0xFFF
    return (r << 4).astype(np.uint16).view(np.float16).astype(np.float32)


def scan_image_error(x32: np.ndarray, bits: int = 12) -> float:
    """max over the rows of || image row - row || (float64): the quantity the device tracks for its certificate"""
    x = np.asarray(x32, dtype=np.float32)
    d = scan_image(x, bits).astype(np.float64) - x.astype(np.float64)
    return float(np.sqrt((d * d).sum(axis=1)).max()) if len(x) else 0.0


# ---- the certificate of the streaming scan, restated (csrc/index_kernels.hpp k_finalize / k_post; nothing of the reference) ----
# The index nominates K' rows by their SCAN score — image row x f16 query, accumulated in float32 by the MFMA, plus for L2 the
# float32 row bias -0.5 ||x||^2 — and certifies a query when  scan[K'-th] + eps < rank(k-th exact),  rank = q.x (IP) or
# q.x - 0.5 ||x||^2 (L2).  That is sound when (1) |scan - rank| <= eps for every row, and (2, L2) the k-th rank the kernel
# derives from the float32 values it holds, 0.5 * (float32 ||q||^2 - float32 dist), is off by no more than eps leaves over.
EPS_TERMS = ("xerr", "qerr", "accum", "bias", "convert")


def certificate_stats(x32: np.ndarray, bits: int = 16, image: np.ndarray | None = None):
    """(xmax, xerr, usable) as k_add tracks them for stored float32 rows: the largest row norm and the largest
    ||image row - row|| (for the 12- / 8-bit images the larger of that and the f16 image's, which the sample and the recovery
    scans read), each with the kernel's 1.0001 slack, as float32; usable = no stored value beyond the f16 range.  `image`:
    the decoded scan image where scan_image cannot restate it (bits = 8: tests/scan_image8.py)."""
    x = np.asarray(x32, dtype=np.float32)
    x64 = x.astype(np.float64)
    xmax = np.float32(np.sqrt((x64 * x64).sum(axis=1)).max()) * np.float32(1.0001)
    with np.errstate(over="ignore", invalid="ignore"):
        err = [scan_image(x, 16).astype(np.float64) - x64]
        if bits != 16:
            err.append((scan_image(x, bits) if image is None else np.asarray(image)).astype(np.float64) - x64)
        xerr = max(np.float32(np.sqrt((e * e).sum(axis=1)).max()) for e in err) * np.float32(1.0001)
    return xmax, xerr, bool(np.abs(x).max() <= 65504.0)


def certificate_eps(x32, q32, metric: str = "ip", bits: int = 16, image=None, kth=None, drop: str | None = None, stats=None):
    """eps [nq] (float64) of the kernels' formula for preprocessed float32 rows / queries:
        xerr ||q16|| + xmax ||q16 - q|| + 2 dimp 2^-24 xmax ||q||   (+ 1e-6 xmax^2 + 3e-8 (||q||^2 + |kth|) for L2)
    `kth`: the k-th reported float32 squared distance per query (the last term is 0 without it).  `drop`: one of EPS_TERMS
    left out — the mutants of tests/test_index_magnitudes_cpu.py.  `stats`: certificate_stats(x32, bits, image) where the
    caller already holds it.  A query whose f16 image overflows gets inf or NaN, as on
    the device (0 * inf when xerr == 0), which the kernels treat as "not certified"."""
    q = np.asarray(q32, dtype=np.float32)
    xmax, xerr, _ = certificate_stats(x32, bits, image) if stats is None else stats
    dimp = -(-q.shape[1] // 128) * 128
    with np.errstate(over="ignore", invalid="ignore"):
        q64 = q.astype(np.float64)
        h64 = q.astype(np.float16).astype(np.float64)
        slack = np.float32(1.0001)
        qn = np.sqrt((q64 * q64).sum(axis=1)).astype(np.float32) * slack
        qh = np.sqrt((h64 * h64).sum(axis=1)).astype(np.float32) * slack
        qe = np.sqrt(((h64 - q64) ** 2).sum(axis=1)).astype(np.float32) * slack
        qn2 = (q64 * q64).sum(axis=1).astype(np.float32)
        terms = {"xerr": float(xerr) * qh.astype(np.float64), "qerr": float(xmax) * qe.astype(np.float64),
                 "accum": 2.0 * dimp * 5.9604645e-8 * float(xmax) * qn.astype(np.float64)}
        if metric == "l2":
            terms["bias"] = np.full(q.shape[0], 1e-6 * float(xmax) * float(xmax))
            if kth is not None:
                terms["convert"] = 3.0e-8 * (qn2.astype(np.float64) + np.abs(np.asarray(kth, dtype=np.float64)))
        eps = np.zeros(q.shape[0])
        for name, t in terms.items():
            if name != drop:
                eps = eps + t
    return eps


def scan_scores(x32, q32, metric: str = "ip", bits: int = 16, image=None, block: int = 4096) -> np.ndarray:
    """The scan's score of every (query, row) pair, float32 [nq, n]: image row x f16 query accumulated as a float32 fma chain
    in k order from 0 — the MFMA's numerics; a product of two f16 values is exact in float32, so `acc + a * b` in float32
    IS the fused step — plus, for L2, the float32 row bias -0.5 * sum(v * v), itself a float32 chain in k order.  (A model
    of the order: the device adds the bias terms in partial sums of eight; both are within the same worst-case bound.)
    Queries whose f16 image is not finite get NaN."""
    x = np.asarray(x32, dtype=np.float32)
    q = np.asarray(q32, dtype=np.float32)
    with np.errstate(over="ignore"):
        qh = q.astype(np.float16).astype(np.float32)
    bad = ~np.isfinite(qh).all(axis=1)
    qh[bad] = 0.0
    img = np.asarray(scan_image(x, bits) if image is None else image, dtype=np.float32)
    out = np.empty((q.shape[0], x.shape[0]), dtype=np.float32)
    prod = np.empty((q.shape[0], block), dtype=np.float32)
    for s in range(0, x.shape[0], block):
        it = np.ascontiguousarray(img[s:s + block].T)
        m = it.shape[1]
        acc = np.zeros((q.shape[0], m), dtype=np.float32)
        for kk in range(it.shape[0]):
            np.multiply(qh[:, kk:kk + 1], it[kk][None, :], out=prod[:, :m])
            acc += prod[:, :m]
        if metric == "l2":
            xt = np.ascontiguousarray(x[s:s + block].T)
            n2 = np.zeros(m, dtype=np.float32)
            for kk in range(xt.shape[0]):
                n2 += xt[kk] * xt[kk]
            acc += (np.float32(-0.5) * n2)[None, :]
        out[:, s:s + m] = acc
    out[bad] = np.nan
    return out


def exact_ranks(x32, q32, metric: str = "ip", block: int = 65536) -> np.ndarray:
    """float64 [nq, n]: the quantity the scan score approximates — q.x, or q.x - 0.5 ||x||^2 for L2"""
    x = np.asarray(x32, dtype=np.float32)
    q64 = np.asarray(q32, dtype=np.float32).astype(np.float64)
    out = np.empty((q64.shape[0], x.shape[0]))
    for s in range(0, x.shape[0], block):
        xb = x[s:s + block].astype(np.float64)
        out[:, s:s + block] = q64 @ xb.T
        if metric == "l2":
            out[:, s:s + block] -= 0.5 * (xb * xb).sum(axis=1)[None, :]
    return out
