"""Test infrastructure: the two quality measures of the reference's ``TopicClustering._analyze_clusters``
(doc/clustering.py:171-215) restated in numpy float64, and the error bounds of the device path for a given input
(DESIGN.md §5h has the derivations).

The restatement does NOT go through a Gram matrix: distances are taken in difference form ``||x_i - x_j||`` and the
cosine is scipy's expression ``1 - u.v / (||u|| ||v||)`` with the cosine clipped to [-1, 1].  Row sums are accumulated in
extended precision, so that the restatement's own rounding is a few units of 2^-53 and the bounds below are the device's.
"""
import numpy as np

U = 2.0 ** -53


def distances(x):
    """[N, N] float64 Euclidean distances in difference form; exact zeros on the diagonal and between equal rows"""
    x = np.asarray(x, dtype=np.float64)
    D = np.empty((len(x), len(x)))
    for i in range(len(x)):
        diff = x - x[i]
        D[i] = np.sqrt(np.sum(diff * diff, axis=1, dtype=np.longdouble).astype(np.float64))
    return D


def _label_sums(M, labels):
    """sums of the columns of M per distinct label (ascending): [N, L] longdouble, the labels, their sizes, and the
    index of every row's own label"""
    uniq, inv, sizes = np.unique(labels, return_inverse=True, return_counts=True)
    order = np.argsort(inv, kind="stable")
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    S = np.add.reduceat(M[:, order].astype(np.longdouble), starts, axis=1)
    return S, uniq, sizes, inv


def silhouette_parts(x, labels):
    """(s, a, b) per row: sklearn's silhouette_samples(metric='euclidean') and its two ingredients.  s is 0 for a label of
    one row, for 0 / 0 and when there is no other label."""
    labels = np.asarray(labels)
    n = len(labels)
    S, uniq, sizes, inv = _label_sums(distances(x), labels)
    rows = np.arange(n)
    own = sizes[inv]
    a = np.where(own > 1, S[rows, inv] / np.maximum(own - 1, 1), 0.0).astype(np.float64)
    other = (S / sizes).astype(np.float64)
    other[rows, inv] = np.inf
    b = other.min(axis=1)
    den = np.maximum(a, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where((own > 1) & np.isfinite(b) & (den > 0), (b - a) / den, 0.0)
    return s, a, b


def silhouette_samples(x, labels):
    return silhouette_parts(x, labels)[0]


def silhouette_bound(x, labels):
    """|s_dev - s_ref| per row.  E_ij = 2 (d + 8) 2^-53 (|x_i| + |x_j|)^2 bounds the squared distance formed from the Gram,
    so |dD_ij| <= min(E_ij / D_ij, sqrt(E_ij)); a_i and b_i inherit the mean of those over the cluster concerned, and
    |ds_i| <= 2 (da + max over the other labels of db) / max(a_i, b_i), a min being 1-Lipschitz."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    n, d = x.shape
    D = distances(x)
    nrm = np.sqrt(np.sum(x * x, axis=1))
    E = 2.0 * (d + 8) * U * (nrm[:, None] + nrm[None, :]) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        dD = np.where(D > 0, np.minimum(E / D, np.sqrt(E)), np.sqrt(E))
    np.fill_diagonal(dD, 0.0)
    T, uniq, sizes, inv = _label_sums(dD, labels)
    rows = np.arange(n)
    own = sizes[inv]
    da = (T[rows, inv] / np.maximum(own - 1, 1)).astype(np.float64)
    db = (T / sizes).astype(np.float64)
    db[rows, inv] = 0.0
    _, a, b = silhouette_parts(x, labels)
    den = np.maximum(a, np.where(np.isfinite(b), b, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, 2.0 * (da + db.max(axis=1)) / den, 0.0)


def cosine_pairs(rows):
    """scipy's pdist(rows, 'cosine') in float64: pairs i < j in row-major order, NaN where a norm is zero"""
    X = np.asarray(rows, dtype=np.float64)
    nrm = np.sqrt(np.sum(X * X, axis=1))
    iu, ju = np.triu_indices(len(X), 1)
    dot = np.sum(X[iu] * X[ju], axis=1, dtype=np.longdouble).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = dot / (nrm[iu] * nrm[ju])
    cos = np.where(np.abs(cos) > 1.0, np.copysign(1.0, cos), cos)
    return 1.0 - cos


def cohesion(x, labels):
    """{label: (mean, population std)} of the cosine distances of every label >= 0 with two rows or more"""
    x = np.asarray(x)
    labels = np.asarray(labels)
    out = {}
    for lab in np.unique(labels):
        if lab < 0 or np.sum(labels == lab) < 2:
            continue
        c = cosine_pairs(x[labels == lab]).astype(np.longdouble)
        m = c.mean()
        out[int(lab)] = (float(m), float(np.sqrt(((c - m) ** 2).mean())))
    return out


def cohesion_bound(d):
    """per pair, hence for the mean: 2 (d + 8) 2^-53; the standard deviation: twice that"""
    return 2.0 * (d + 8) * U


def std_bound(d):
    return 4.0 * (d + 8) * U


def analyze(embeddings, labels):
    """the reference's cluster_info dict from the restatement (centres: the reference's own float32 expression)"""
    emb = np.ascontiguousarray(embeddings, dtype=np.float32)
    labels = np.asarray(labels)
    uniq = np.unique(labels)
    n_clusters = len(uniq[uniq >= 0])
    info = {"n_clusters": n_clusters, "n_noise": np.sum(labels == -1), "cluster_sizes": {}, "cluster_centers": {},
            "cluster_quality": {}}
    coh = cohesion(emb, labels)
    for lab in uniq:
        if lab == -1:
            continue
        mask = labels == lab
        info["cluster_sizes"][lab] = int(np.sum(mask))
        info["cluster_centers"][lab] = np.mean(emb[mask], axis=0).tolist()
        if int(lab) in coh:
            info["cluster_quality"][lab] = {"cohesion": coh[int(lab)][0], "std": coh[int(lab)][1]}
    info["silhouette_score"] = 0.0
    if n_clusters > 1 and len(emb) > n_clusters and 1 < len(uniq) < len(emb):
        info["silhouette_score"] = float(np.mean(silhouette_samples(emb, labels)))
    return info
