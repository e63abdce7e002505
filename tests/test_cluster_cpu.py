"""CPU tests of the DBSCAN restatement (tests/cluster_ref.py) against the goldens recorded from sklearn and from the
reference's TopicClustering (tests/golden/make_cluster_golden.py), and of the conditions that generator promises."""
import os

import numpy as np
import pytest

import cluster_ref as cr

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 4e-6


def load_cases():
    z = np.load(os.path.join(HERE, "golden", "cluster_cases.npz"))
    return [{"x": z[f"c{i}_x"], "labels": z[f"c{i}_labels"], "eps": float(z["eps"][i]), "ms": int(z["min_samples"][i]),
             "metric": "cosine" if z["metric"][i] else "euclidean", "auto": bool(z["auto"][i])}
            for i in range(len(z["eps"]))]


CASES = load_cases()
IDS = [f"{i}-{'auto' if c['auto'] else 'eps'}-{c['metric']}" for i, c in enumerate(CASES)]


def rows_of(c):
    return c["x"] if c["metric"] == "euclidean" else cr.normalize_rows(c["x"])


def test_golden_set_covers_what_it_must():
    assert sum(not c["auto"] for c in CASES) >= 12 and sum(c["auto"] for c in CASES) >= 8
    for metric in ("euclidean", "cosine"):
        for auto in (False, True):
            assert any(c["metric"] == metric and c["auto"] == auto for c in CASES)
    assert any(c["labels"].max() >= 1 for c in CASES) and any((c["labels"] < 0).any() for c in CASES)
    border = False
    for c in CASES:
        inside = cr.distances(rows_of(c), c["metric"]) <= c["eps"]
        np.fill_diagonal(inside, True)
        border |= bool(((c["labels"] >= 0) & (inside.sum(axis=1) < c["ms"])).any())
    assert border
    assert os.path.getsize(os.path.join(HERE, "golden", "cluster_cases.npz")) < (1 << 20)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_gives_the_recorded_labels(c):
    eps = c["eps"] * cr.EPS_INFLATION if c["auto"] and 0.1 < c["eps"] < 2.0 else c["eps"]
    got = cr.dbscan_ref(rows_of(c), eps, c["ms"], c["metric"])
    assert np.array_equal(got, c["labels"])


@pytest.mark.parametrize("c", [c for c in CASES if c["auto"]], ids=[i for i, c in zip(IDS, CASES) if c["auto"]])
def test_restated_eps_is_the_references(c):
    # 2e-6 relative: the 2^-20 inflation (9.6e-7) plus the float32 rounding of sklearn's squared distance, halved by the
    # square root (6e-8); sklearn's float64 error is negligible beside these
    eps = cr.find_optimal_eps_ref(c["x"], c["ms"])
    print(f"eps {eps!r} reference {c['eps']!r} rel {abs(eps - c['eps']) / c['eps']:.3e}")
    assert abs(eps - c["eps"]) <= 2e-6 * c["eps"]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_generator_conditions_hold_on_the_stored_inputs(c):
    D = cr.distances(rows_of(c), c["metric"])
    d = D[np.triu_indices(len(D), 1)]
    rel = np.abs(d - c["eps"]) / c["eps"]
    if c["auto"] and c["metric"] == "euclidean" and 0.1 < c["eps"] < 2.0:
        rel = rel[rel > 2e-7]  # the pairs at the defining distance itself
        assert rel.size < d.size
    assert (rel > MARGIN).all()                                                       # (a)
    if c["auto"]:
        df = np.sort(np.diff(cr.k_distances(c["x"], c["ms"])))
        assert df[-1] - df[-2] > 1e-5 * df[-1]                                         # (b)
        for e in (c["eps"] * (1 - MARGIN), c["eps"] * (1 + MARGIN)):                   # (c), by the restatement
            assert np.array_equal(cr.dbscan_from_distances(D, e, c["ms"]), c["labels"])
