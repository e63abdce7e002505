"""The cluster-quality cohesion and the diversity cosine matrix are read from one float64 Gram tile (csrc/gram_f64.hpp):
for a pair of rows both divide the same G_ij by the product of the square roots of the same diagonal entries, clip at 1,
and are compiled without contraction — so they agree bit for bit, on either side of a tile edge of either tile shape."""
import numpy as np
import pytest

N = 130  # 65 two-row clusters: pair 31/32 lies across a 32-row tile edge, pair 63/64 across a 64-row one


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 5, 64, 65, 130])
def test_cohesion_of_a_pair_is_one_minus_its_diversity_cosine(d):
    from anorag_hip import METRIC_L2, FlatIndex
    from anorag_hip.diversity import diversify
    from anorag_hip.topic_clustering import cluster_quality

    rng = np.random.default_rng(7000 + d)
    x = np.abs(rng.standard_normal((N, d)) * np.exp(rng.uniform(-3, 3, (N, 1)))).astype(np.float32)
    assert (x > 0).all()
    index = FlatIndex(d, METRIC_L2, normalize=False, device=0)
    try:
        index.add(x)
        q = cluster_quality(index, np.arange(N) // 2, silhouette=False)
        rows = np.arange(N)
        (kept, sel, sim), = diversify(index, [rows], [np.zeros(N)], max_candidates=1024, dedup=False,
                                      similarity_threshold=2.0)
    finally:
        index.close()
    assert list(kept) == list(rows) and list(sel) == list(rows) and sim.shape == (N, N)
    assert list(q["labels"]) == list(range(N // 2)) and (q["sizes"] == 2).all()
    pair = sim[rows[0::2], rows[1::2]]
    differ = np.flatnonzero(q["cohesion"] != 1.0 - pair)
    assert differ.size == 0, (d, differ[:8], q["cohesion"][differ[:8]], 1.0 - pair[differ[:8]])
