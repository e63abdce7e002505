"""Test helper: the IVF-PQ mode of anr_ivf (anr_ivf_create_pq, csrc/ivf.hip) restated in numpy in float64, on top of
tests/ivf_ref.py (coarse k-means, assignment, probing): residuals, the per-sub-space k-means, encoding (argmin, ties to
the lower code), decoding, ADC keys and the probed ADC top-k (ties to the lower id).  Keys: larger is better (IP
q.c + sum_j q_j.cb_j[code_j]; L2 -sum_j |(q - c)_j - cb_j[code_j]|^2)."""
from __future__ import annotations

import numpy as np

import ivf_ref

FLT_MAX = ivf_ref.FLT_MAX
U = 2.0 ** -24  # unit roundoff of float32


def sub(x: np.ndarray, m: int) -> np.ndarray:
    """[n, d] -> [n, m, d / m]"""
    return x.reshape(x.shape[0], m, -1)


def residuals(x: np.ndarray, cent: np.ndarray, lists: np.ndarray) -> np.ndarray:
    """x - c_list, in float32 (as the device subtracts)"""
    return (x.astype(np.float32) - cent.astype(np.float32)[lists]).astype(np.float32)


def train(res: np.ndarray, init: np.ndarray, niter: int) -> np.ndarray:
    """codebooks [m, 256, dsub]: one ivf_ref.lloyd(..., "l2") per sub-space of the residuals, from init"""
    m = init.shape[0]
    r = sub(res, m)
    return np.stack([ivf_ref.lloyd(np.ascontiguousarray(r[:, j]), init[j], niter, "l2") for j in range(m)])


def encode(res: np.ndarray, cb: np.ndarray) -> np.ndarray:
    """codes [n, m] uint8: per sub-space the float64 argmin of |r_j - cb_j[c]|^2 (differences squared directly), the
    lower code among equal distances"""
    m = cb.shape[0]
    r = sub(res, m).astype(np.float64)
    c64 = cb.astype(np.float64)
    out = np.empty((res.shape[0], m), dtype=np.uint8)
    for s in range(0, res.shape[0], 1024):
        blk = r[s:s + 1024]
        for j in range(m):
            d = ((blk[:, j, None, :] - c64[j][None]) ** 2).sum(axis=2)
            out[s:s + 1024, j] = np.argmin(d, axis=1)
    return out


def decode(lists: np.ndarray, codes: np.ndarray, cent: np.ndarray, cb: np.ndarray) -> np.ndarray:
    """c_list + the codebook entries, float32 (faiss's IVFPQ reconstruct)"""
    m = cb.shape[0]
    rt = cb[np.arange(m)[None, :], codes.astype(np.int64)].reshape(len(codes), -1)
    return (cent[lists].astype(np.float32) + rt.astype(np.float32)).astype(np.float32)


def adc_keys(q: np.ndarray, lists: np.ndarray, codes: np.ndarray, cent: np.ndarray, cb: np.ndarray,
             metric: str) -> np.ndarray:
    """float64 ADC keys [nq, n] of the coded rows (list, codes)"""
    m = cb.shape[0]
    q64, c64 = q.astype(np.float64), cent.astype(np.float64)
    rt = cb.astype(np.float64)[np.arange(m)[None, :], codes.astype(np.int64)].reshape(len(codes), -1)  # [n, d]
    if metric == "ip":
        return q64 @ c64[lists].T + q64 @ rt.T
    out = np.empty((q.shape[0], len(codes)))
    for i in range(q.shape[0]):
        v = q64[i][None, :] - c64[lists] - rt
        out[i] = -(v * v).sum(axis=1)
    return out


def key_bounds(q: np.ndarray, lists: np.ndarray, codes: np.ndarray, cent: np.ndarray, cb: np.ndarray,
               metric: str) -> np.ndarray:
    """[nq, n]: a bound on |device key - adc_keys| from float32 arithmetic (the derivation is in test_ivfpq_gpu.py)"""
    m = cb.shape[0]
    d = q.shape[1]
    dsub = d // m
    g = (dsub + m + 2) * U / (1.0 - (dsub + m + 2) * U)
    q64, c64 = q.astype(np.float64), cent.astype(np.float64)
    rt = cb.astype(np.float64)[np.arange(m)[None, :], codes.astype(np.int64)].reshape(len(codes), -1)
    if metric == "ip":
        s = np.abs(q64) @ np.abs(rt).T  # sum_d |q_d| |cb_d|
        key = q64 @ c64[lists].T + q64 @ rt.T
        return g * s + U * np.abs(key) + 1e-12 * (1.0 + np.abs(key))
    out = np.empty((q.shape[0], len(codes)))
    for i in range(q.shape[0]):
        a = q64[i][None, :] - c64[lists]      # q - c (exact); the device rounds it to float32
        v = a - rt
        eta = U * (1.01 * np.abs(a) + np.abs(v))
        out[i] = (eta * (2.0 * np.abs(v) + eta)).sum(axis=1) + g * ((np.abs(v) + eta) ** 2).sum(axis=1)
    return out * 1.01 + 1e-12


def search(q: np.ndarray, lists: np.ndarray, codes: np.ndarray, ids: np.ndarray, cent: np.ndarray, cb: np.ndarray,
           k: int, nprobe: int, metric: str):
    """ADC top-k over the coded rows of the probed lists, by (key desc, id asc): D float32 (IP key / squared L2
    distance), I int64, padded with -1 / -FLT_MAX (IP) / +FLT_MAX (L2); also the float64 keys [nq, n]"""
    nq = q.shape[0]
    D = np.full((nq, k), -FLT_MAX if metric == "ip" else FLT_MAX, dtype=np.float32)
    I = np.full((nq, k), -1, dtype=np.int64)
    P = ivf_ref.probed(q, cent, nprobe, metric)
    S = adc_keys(q, lists, codes, cent, cb, metric)
    for i in range(nq):
        sel = np.flatnonzero(np.isin(lists, P[i]))
        if len(sel) == 0:
            continue
        s = S[i, sel]
        order = np.lexsort((ids[sel], -s))[:k]
        D[i, :len(order)] = (s[order] if metric == "ip" else -s[order]).astype(np.float32)
        I[i, :len(order)] = ids[sel][order]
    return D, I, S
