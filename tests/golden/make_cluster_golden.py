#!/usr/bin/env python3
"""Golden cases for DBSCAN topic clustering, produced by RUNNING sklearn's DBSCAN and THE REFERENCE's own
TopicClustering._find_optimal_eps / _cpu_clustering (doc/clustering.py:71-99, :149-169) on seeded inputs (build
container only; needs scikit-learn and the reference checkout):

  python tests/golden/make_cluster_golden.py [/root/reference]

writes tests/golden/cluster_cases.npz: per case c<i>_x (float32 rows), c<i>_labels (int64), and the arrays eps,
min_samples, metric (0 euclidean, 1 cosine), auto (1: eps is the reference's own, labels are _cpu_clustering's).  Data
only; no reference source is copied.  doc/clustering.py imports loguru and the reference's `utils` / `config` packages;
none of the arithmetic pinned here lives in them, so they are STAND-INS in sys.modules (config.get(key, default) ->
the case's override or the default).

A case is kept only if its INPUT is one on which the answer cannot hang on a rounding (conditions, not tolerances;
tests/test_cluster_cpu.py re-checks them on the stored file):
  (a) explicit-eps cases: no pair's float64 distance is within 4e-6 relative of eps.  Auto-eps cases: the same, except
      for the pairs at the defining distance itself (within 2e-7 relative of the reference's eps, which IS the distance
      of a pair; the device uses eps * (1 + 2^-20), condition (c) covers which side that pair falls on);
  (b) auto-eps cases: the largest forward difference of the sorted k-distance curve exceeds the second largest by more
      than 1e-5 relative, so the knee cannot move;
  (c) auto-eps cases: sklearn's labels are identical at eps * (1 - 4e-6), eps and eps * (1 + 4e-6).
The kept set must hold >= 12 explicit and >= 8 auto cases, both metrics, and cases with >= 2 clusters, noise and border
rows; the script fails otherwise.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cluster_ref as cr  # noqa: E402

MARGIN = 4e-6
OVERRIDES = {}


def install_stand_ins():
    lg = types.ModuleType("loguru")

    class _L:
        def __getattr__(self, _):
            return lambda *a, **k: None

    lg.logger = _L()
    sys.modules["loguru"] = lg
    ut = types.ModuleType("utils")

    class GPUUtils:
        @staticmethod
        def is_cudf_available():
            return False

    class BatchProcessor:
        def __init__(self, *a, **k):
            pass

    ut.GPUUtils, ut.BatchProcessor = GPUUtils, BatchProcessor
    sys.modules["utils"] = ut
    cf = types.ModuleType("config")

    class _C:
        def get(self, key, default=None):
            return OVERRIDES.get(key, default)

    cf.config = _C()
    sys.modules["config"] = cf


def load_reference():
    install_stand_ins()
    spec = importlib.util.spec_from_file_location("ref_clustering", os.path.join(REF, "doc", "clustering.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.TopicClustering


def make_input(rng):
    n = int(rng.integers(40, 240))
    d = int(rng.choice([8, 32, 64]))
    c = int(rng.integers(2, 7))
    spread = float(rng.choice([0.04, 0.08, 0.15]))
    centres = rng.standard_normal((c, d)) * float(rng.choice([0.5, 1.0]))
    x = centres[rng.integers(0, c, n)] + rng.standard_normal((n, d)) * spread
    stray = rng.random(n) < 0.06  # a few rows away from every centre: noise and border candidates
    x[stray] += rng.standard_normal((int(stray.sum()), d)) * spread * 4
    return x.astype(np.float32)


def pair_margin_ok(D, eps, skip_at=None):
    iu = np.triu_indices(D.shape[0], 1)
    rel = np.abs(D[iu] - eps) / eps
    if skip_at is not None:
        rel = rel[np.abs(D[iu] - skip_at) / skip_at > 2e-7]
    return bool((rel > MARGIN).all())


def traits(D, eps, ms, labels):
    inside = D <= eps
    np.fill_diagonal(inside, True)
    core = inside.sum(axis=1) >= ms
    return {"clusters": int(labels.max() + 1), "noise": bool((labels < 0).any()),
            "border": bool(((labels >= 0) & ~core).any())}


def main():
    from sklearn.cluster import DBSCAN
    TopicClustering = load_reference()
    cases, seen = [], {"explicit": 0, "auto": 0}
    for seed in range(400):
        rng = np.random.default_rng(1000 + seed)
        x = make_input(rng)
        ms = int(rng.choice([3, 5]))
        metric = "cosine" if seed % 2 else "euclidean"
        auto = seed % 3 == 0
        kind = "auto" if auto else "explicit"
        if seen[kind] >= (10 if auto else 14):
            continue
        rows = x if metric == "euclidean" else cr.normalize_rows(x)
        D = cr.distances(rows, metric)
        if auto:
            OVERRIDES.update({"clustering.algorithm": "dbscan", "clustering.min_samples": ms, "clustering.metric": metric})
            tc = TopicClustering()
            eps = float(tc._find_optimal_eps(x))
            labels = np.asarray(tc._cpu_clustering(x), dtype=np.int64)
            kd = cr.k_distances(x, ms)
            df = np.sort(np.diff(kd))
            if not df[-1] - df[-2] > 1e-5 * df[-1]:
                continue  # (b)
            if not pair_margin_ok(D, eps, skip_at=eps if metric == "euclidean" and 0.1 < eps < 2.0 else None):
                continue  # (a)
            same = all(np.array_equal(DBSCAN(eps=e, min_samples=ms, metric=metric).fit_predict(x), labels)
                       for e in (eps * (1 - MARGIN), eps, eps * (1 + MARGIN)))
            if not same:
                continue  # (c)
        else:
            iu = np.triu_indices(len(x), 1)
            eps = float(np.quantile(D[iu], float(rng.choice([0.03, 0.06, 0.12]))))
            if not pair_margin_ok(D, eps):
                continue  # (a)
            labels = np.asarray(DBSCAN(eps=eps, min_samples=ms, metric=metric).fit_predict(x), dtype=np.int64)
        t = traits(D, eps, ms, labels)
        seen[kind] += 1
        cases.append({"x": x, "eps": eps, "ms": ms, "metric": metric, "auto": auto, "labels": labels, **t})
        print(f"seed {seed}: {kind} {metric} n={len(x)} d={x.shape[1]} ms={ms} eps={eps:.6f} {t}")
    n_exp = sum(not c["auto"] for c in cases)
    n_auto = sum(c["auto"] for c in cases)
    assert n_exp >= 12 and n_auto >= 8, (n_exp, n_auto)
    for m in ("euclidean", "cosine"):
        for a in (False, True):
            assert any(c["metric"] == m and c["auto"] == a for c in cases), (m, a)
    assert any(c["clusters"] >= 2 for c in cases) and any(c["noise"] for c in cases) and any(c["border"] for c in cases)
    out = {"eps": np.array([c["eps"] for c in cases], dtype=np.float64),
           "min_samples": np.array([c["ms"] for c in cases], dtype=np.int64),
           "metric": np.array([c["metric"] == "cosine" for c in cases], dtype=np.int64),
           "auto": np.array([c["auto"] for c in cases], dtype=np.int64)}
    for i, c in enumerate(cases):
        out[f"c{i}_x"] = c["x"]
        out[f"c{i}_labels"] = c["labels"]
    path = os.path.join(HERE, "cluster_cases.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(cases)} cases ({n_exp} explicit, {n_auto} auto), {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
