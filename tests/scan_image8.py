"""Test helper: the 8-bit scan image (ANR_OPT_SCAN_BITS 8) restated in numpy — what the device's k_add / k_build8 must
write and its scan decode, bit for bit (the layout and the rule are described at the top of index_kernels.hpp)."""
from __future__ import annotations

import numpy as np

F16_MAX = np.float32(65504.0)


def _groups(x32: np.ndarray) -> np.ndarray:
    """[n, dim] float32 -> [n, G, 32] float32, zero-padded to the row width the index keeps (a multiple of 128)"""
    n, d = x32.shape
    dp = -(-d // 128) * 128
    g = np.zeros((n, dp), dtype=np.float32)
    g[:, :d] = x32
    return g.reshape(n, dp // 32, 32)


def scales(x32: np.ndarray) -> np.ndarray:
    """[n, G] float16 scales: s = f16(absmax / 127), one f16 step up if s * 127 < absmax; 0 for an all-zero group"""
    amax = np.abs(_groups(x32)).max(axis=2)
    s = (amax / np.float32(127.0)).astype(np.float16)
    up = s.astype(np.float32) * np.float32(127.0) < amax
    bits = s.view(np.uint16).copy()
    bits[up] += 1
    s = bits.view(np.float16)
    s[amax == 0] = 0
    return s


def codes(x32: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(codes [n, G, 32] int16 in -127..127, scales [n, G] float16)"""
    s = scales(x32)
    s32 = s.astype(np.float32)[:, :, None]
    g = _groups(x32)
    with np.errstate(divide="ignore", invalid="ignore"):
        cmax = np.minimum(np.float32(127.0), np.floor(F16_MAX / s32))
        c = np.clip(np.rint(g / s32), -cmax, cmax)
    c = np.where(s32 > 0, c, 0).astype(np.int16)
    return c, s


def decode(x32: np.ndarray) -> np.ndarray:
    """the values the scan multiplies: f16(s * c), one rounding, as float32 [n, dim]"""
    c, s = codes(x32)
    v = (s.astype(np.float64)[:, :, None] * c.astype(np.float64)).astype(np.float16).astype(np.float32)
    return v.reshape(x32.shape[0], -1)[:, :x32.shape[1]]


def error_norm(x32: np.ndarray) -> float:
    """max over rows of ||decode(x) - x||"""
    if x32.shape[0] == 0:
        return 0.0
    e = decode(x32).astype(np.float64) - x32.astype(np.float64)
    return float(np.sqrt((e * e).sum(axis=1)).max())
