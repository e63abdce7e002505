"""numpy restatement of what anr_index_remove does to the row numbering (test infrastructure; csrc/index_edit_kernels.hpp
k_gather_rows / edit_shift), and the certificate statistics of stored rows."""
from __future__ import annotations

import numpy as np

import scan_image8 as s8
from oracle import flat_index as orc


def valid_gone(rows, n: int) -> np.ndarray:
    """the rows a removal actually drops: inside [0, n), distinct, ascending (IndexFlat.remove_ids ignores the rest)"""
    r = np.asarray(rows, dtype=np.int64).reshape(-1)
    return np.unique(r[(r >= 0) & (r < n)])


def source_map(n: int, gone: np.ndarray) -> np.ndarray:
    """source row of every destination row 0 .. n - len(gone) - 1: j + c(j), c(j) = #{i : gone[i] - i <= j}, found by a
    binary search over the non-decreasing sequence gone[i] - i (gone ascending and distinct)"""
    gone = np.asarray(gone, dtype=np.int64)
    gm = gone - np.arange(len(gone), dtype=np.int64)
    j = np.arange(n - len(gone), dtype=np.int64)
    return j + np.searchsorted(gm, j, side="right")


def true_stats(stored: np.ndarray, bits_list=(16,)) -> dict:
    """float64 maxima over the stored float32 rows: the row norm and the image error norms the index tracks"""
    if len(stored) == 0:
        return {"max_norm": 0.0, **{f"max_err{b}": 0.0 for b in bits_list}}
    out = {"max_norm": float(np.sqrt((stored.astype(np.float64) ** 2).sum(axis=1)).max())}
    for b in bits_list:
        out[f"max_err{b}"] = s8.error_norm(stored) if b == 8 else orc.scan_image_error(stored, b)
    return out


def image(stored: np.ndarray, bits: int) -> np.ndarray:
    if len(stored) == 0:
        return np.zeros(stored.shape, dtype=np.float32)
    return s8.decode(stored) if bits == 8 else orc.scan_image(stored, bits)
