"""Test infrastructure: DBSCAN as a closed form, in numpy float64 on a dense N x N distance matrix, and the reference's
eps selection (doc/clustering.py:149-169) with the documented inflation.  What the device is held to.

  N(i)      = { j : D(i, j) <= eps }, i included
  core(i)   = |N(i)| >= min_samples
  clusters  = connected components of the core rows under D <= eps, numbered from 0 by smallest core row
  non-core  = smallest label among its core neighbours, or -1

sklearn's sequential expansion gives the same: it opens clusters in the order of their first core row and expands each to
the end before the next opens, so a border row is claimed by the first-opened (= smallest-labelled) cluster that has a
core row within eps of it."""
import numpy as np

EPS_INFLATION = 1.0 + 2.0 ** -20


def normalize_rows(x):
    """the rows as a normalising index stores them: float32 x / float32(||x|| in float64)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    n = np.where(n == 0, np.float32(1), n)
    return (x / n[:, None]).astype(np.float32)


def distances(rows, metric):
    """float64 D of float32 rows; 'cosine' takes the rows as stored (already normalised): 1 - x_i . x_j"""
    x = np.asarray(rows, dtype=np.float32).astype(np.float64)
    if metric == "cosine":
        return 1.0 - x @ x.T
    if metric != "euclidean":
        raise ValueError(metric)
    if x.shape[0] > 600:
        # Gram form for the larger test shapes (a BLAS call): in float64 its cancellation error is ~1e-16 ||x||^2,
        # far below the spacing of the distances the tests choose eps between
        n2 = (x * x).sum(axis=1)
        return np.sqrt(np.maximum(n2[:, None] + n2[None, :] - 2.0 * (x @ x.T), 0.0))
    d2 = np.empty((x.shape[0], x.shape[0]))
    for i in range(x.shape[0]):  # direct form: no cancellation
        d2[i] = ((x - x[i]) ** 2).sum(axis=1)
    return np.sqrt(d2)


def dbscan_from_distances(D, eps, min_samples):
    n = D.shape[0]
    inside = D <= eps
    np.fill_diagonal(inside, True)
    core = inside.sum(axis=1) >= min_samples
    adj = inside & core[:, None] & core[None, :]
    # components of the core graph: every core row takes the smallest label in its neighbourhood, then labels are
    # followed to their own labels (pointer jumping), to the fixpoint; slot n is the "no core row" sentinel
    lab = np.append(np.where(core, np.arange(n), n), n)
    while True:
        new = lab.copy()
        new[:n] = np.minimum(lab[:n], np.where(adj, lab[None, :n], n).min(axis=1, initial=n))
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            break
        lab = new
    root = lab[:n]
    roots = np.unique(root[core])
    rank = {int(r): k for k, r in enumerate(roots)}
    out = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        if core[i]:
            out[i] = rank[int(root[i])]
        else:
            nb = inside[i] & core
            if nb.any():
                out[i] = min(rank[int(r)] for r in root[nb])
    return out


def dbscan_ref(rows, eps, min_samples, metric="euclidean"):
    return dbscan_from_distances(distances(rows, metric), float(eps), int(min_samples))


def k_distances(x, k):
    """sorted Euclidean distance of every row to its k-th nearest row, itself included"""
    D = distances(x, "euclidean")
    np.fill_diagonal(D, 0.0)
    return np.sort(np.sort(D, axis=1)[:, k - 1])


def find_optimal_eps_ref(x, min_samples):
    kd = k_distances(x, int(min_samples))
    eps = float(kd[int(np.argmax(np.diff(kd)))])
    if eps < 0.1:
        return 0.1
    if eps > 2.0:
        return 2.0
    return min(2.0, eps * EPS_INFLATION)
