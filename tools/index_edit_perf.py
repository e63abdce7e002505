#!/usr/bin/env python3
"""Developer tool: in-place edits of the flat index (anr_index_remove / anr_index_update) against the host round trip they
replace, on N x 768 rows (default N = 1 000 000):

  remove 1 % random rows | remove the last 1 000 rows | update 1 000 scattered rows

Each edit is timed (wall clock around the call, which returns when the device work is complete) with the new calls and
with the method VectorIndex.remove_vectors used before them, spelled out below: reconstruct_n of everything, the edit in
numpy, a fresh FlatIndex, OPT_ADD_RAW, add.  Prints both times and the algorithmic bytes moved.

usage: index_edit_perf.py [N] [scan_bits]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ano-rag_amd"))
import numpy as np

from anorag_hip import FlatIndex, METRIC_IP
from anorag_hip._lib import OPT_ADD_RAW, OPT_SCAN_BITS

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
bits = int(sys.argv[2]) if len(sys.argv) > 2 else 16
d = 768
rng = np.random.default_rng(0)
x = rng.standard_normal((n, d), dtype=np.float32)
x /= np.linalg.norm(x, axis=1, keepdims=True)
image_bytes = {16: 2.0, 12: 3.5, 8: 3.0625}[bits] * d      # per row: x16, plus the coarse image where one is kept


def build():
    idx = FlatIndex(d, METRIC_IP, normalize=True)
    idx.reserve(n)
    idx.set_option(OPT_SCAN_BITS, bits)
    idx.add(x)
    return idx


def edit_bytes(kind, rows):
    """algorithmic device traffic of the in-place edit: compaction (read + write of every row behind the first removed
    one, twice where a chunk goes through the staging buffer), the re-image pass (one corpus read, image writes from the
    first edited tile on), and for an update the new rows and their images"""
    if kind == "remove":
        r0, m = int(np.min(rows)), len(np.unique(rows))
        moved = (n - m - r0) * d * 4
        return 4 * moved, n * d * 4 + (n - r0) * image_bytes
    return len(rows) * d * 4 * 2 + len(rows) * image_bytes, n * d * 4


def round_trip(idx, kind, rows, new):
    """the method before the in-place calls: everything to the host, the edit in numpy, a second index"""
    t0 = time.perf_counter()
    stored = idx.reconstruct_n(0, idx.ntotal)
    if kind == "remove":
        keep = np.ones(len(stored), dtype=bool)
        keep[rows] = False
        stored = stored[keep]
    else:
        stored[rows] = new / np.linalg.norm(new, axis=1, keepdims=True)
    fresh = FlatIndex(d, METRIC_IP, normalize=True)
    fresh.set_option(OPT_SCAN_BITS, bits)
    fresh.set_option(OPT_ADD_RAW, 1)
    fresh.add(stored)
    fresh.set_option(OPT_ADD_RAW, 0)
    dt = time.perf_counter() - t0
    fresh.close()
    return dt


cases = [("remove 1 % random rows", "remove", rng.choice(n, n // 100, replace=False)),
         ("remove the last 1 000 rows", "remove", np.arange(n - 1000, n)),
         ("update 1 000 scattered rows", "update", rng.choice(n, 1000, replace=False))]
print(f"{n} x {d} rows, scan bits {bits}; corpus {n * d * 4 / 1e9:.2f} GB float32")
warm = build()
warm.remove_rows([0])
warm.update_rows([0], x[:1])
warm.close()
for name, kind, rows in cases:
    new = rng.standard_normal((len(rows), d), dtype=np.float32) if kind == "update" else None
    idx = build()
    t0 = time.perf_counter()
    if kind == "remove":
        assert idx.remove_rows(rows) == len(rows)
    else:
        idx.update_rows(rows, new)
    t_edit = time.perf_counter() - t0
    idx.close()
    idx = build()
    t_trip = round_trip(idx, kind, rows, new)
    idx.close()
    moved, reimage = edit_bytes(kind, rows)
    print(f"{name}: in place {t_edit * 1e3:.2f} ms ({moved / 1e9:.3f} GB moved at most + {reimage / 1e9:.3f} GB re-image "
          f"= {(moved + reimage) / t_edit / 1e12:.2f} TB/s); host round trip {t_trip * 1e3:.0f} ms "
          f"({2 * n * d * 4 / 1e9:.2f} GB over the host link) -> {t_trip / t_edit:.0f} x")
