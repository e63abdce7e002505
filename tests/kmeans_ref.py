"""numpy float64 restatement of anr_index_kmeans (csrc/kmeans.hip): sklearn's KMeans.fit (k-means++
seeding, Lloyd, best of n_init) on uncentred float32 rows, with the kernel's summation orders —

* a sum over rows (potential, inertia): halving trees over blocks of 256, halving trees over 256 of those, the rest
  one after the other (``ordered_sum``);
* the seeding's cumulative sum: Hillis-Steele inside blocks of 256, the blocks' offsets one after the other
  (``block_scan``); searchsorted as "the first row whose sum reaches the value";
* centre sums: rows in ascending order inside chunks of 512, chunks in ascending order (``centre_sums``);
* sums over dimensions (shift, inertia of a row, variance): ascending.

Only the dot product x.c is not the device's sequence (the MFMA's inner order is the hardware's): ``dot="ordered"`` adds
the products in ascending k, which makes a row and a centre copied from it exactly 0 apart as on the device;
``dot="blas"`` uses matmul (faster; for inputs whose decision margins are known to be far above 1e-13).  Everything a
decision does not hang on a dot product — centres, shift, tol, inertia — is the device's bit for bit once the labels agree.

``fit`` records the smallest relative margin of the decisions taken: a drawn value against the nearest cumulative-sum
boundary, the best against the second-best candidate potential, the nearest against the second-nearest centre, and the
centre shift against tol.
"""
import numpy as np

BLOCK = 256
CHUNK = 512


class EmptyCluster(Exception):
    pass


def draws(n, k, n_init, random_state=42):
    """The draws sklearn's KMeans(random_state).fit makes, in its order: per init one ``choice`` with the float32 unit
    weights' probabilities, then one ``uniform(size=2 + int(log(k)))`` per further centre."""
    rs = np.random.RandomState(random_state)
    trials = 2 + int(np.log(k))
    w = np.ones(n, dtype=np.float32)
    first = np.empty(n_init, dtype=np.int64)
    u = np.empty((n_init, k - 1, trials), dtype=np.float64)
    for i in range(n_init):
        first[i] = rs.choice(n, p=w / w.sum())
        for c in range(k - 1):
            u[i, c] = rs.uniform(size=trials)
    return first, u


def _blocks(v):
    v = np.asarray(v, dtype=np.float64)
    nb = max(1, -(-v.size // BLOCK))
    a = np.zeros(nb * BLOCK)
    a[:v.size] = v
    return a.reshape(nb, BLOCK)


def tree256(v):
    a = _blocks(v)
    o = BLOCK // 2
    while o >= 1:
        a = a[:, :o] + a[:, o:2 * o]
        o //= 2
    return a[:, 0]


def ordered_sum(v):
    s = np.float64(0.0)
    for x in tree256(tree256(v)):
        s = s + x
    return s


def block_scan(v):
    n = len(v)
    a = _blocks(v)
    o = 1
    while o < BLOCK:
        a[:, o:] = a[:, o:] + a[:, :-o]
        o *= 2
    off = np.zeros(a.shape[0])
    s = np.float64(0.0)
    for b in range(a.shape[0]):
        off[b] = s
        s = s + a[b, BLOCK - 1]
    return (off[:, None] + a).reshape(-1)[:n]


def first_reaching(cs, rv):
    hit = np.nonzero(cs >= rv)[0]
    return int(hit[0]) if hit.size else len(cs) - 1


def seq_sum(a, axis):
    """Sum along an axis in ascending order (np.add.accumulate is sequential)."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis))
    return np.take(np.add.accumulate(a, axis=axis), -1, axis=axis)


def _dot(X, C, dot):
    if dot == "blas":
        return X @ C.T
    acc = np.zeros((X.shape[0], C.shape[0]))
    for t in range(X.shape[1]):
        acc = acc + X[:, t, None] * C[None, :, t]
    return acc


def _norms(X, dot):
    if dot == "blas":
        return np.einsum("ij,ij->i", X, X)
    s = np.zeros(X.shape[0])
    for t in range(X.shape[1]):
        s = s + X[:, t] * X[:, t]
    return s


def sq_distances(X, nx, C, dot):
    return (nx[:, None] + _norms(C, dot)[None, :]) - 2.0 * _dot(X, C, dot)


def centre_sums(X, lab, k):
    n, d = X.shape
    sums = np.zeros((k, d))
    cnt = np.zeros(k, dtype=np.int64)
    for r0 in range(0, n, CHUNK):
        seg, l = X[r0:r0 + CHUNK], lab[r0:r0 + CHUNK]
        for j in range(k):
            m = l == j
            c = int(m.sum())
            if c:
                sums[j] = sums[j] + seq_sum(seg[m], 0)
                cnt[j] += c
    return sums, cnt


def tolerance(X, tol_scale):
    n, d = X.shape
    zero = np.zeros(n, dtype=np.int64)
    mean = centre_sums(X, zero, 1)[0][0] / np.float64(n)
    var = centre_sums((X - mean) * (X - mean), zero, 1)[0][0] / np.float64(n)
    return np.float64(tol_scale) * (seq_sum(var, 0) / np.float64(d))


def kpp(X, nx, k, first, u, marg, dot):
    n = X.shape[0]
    ids = [int(first)]
    closest = np.maximum(sq_distances(X, nx, X[ids], dot), 0.0)[:, 0]
    pot = ordered_sum(closest)
    for c in range(1, k):
        cs = block_scan(closest)
        rv = u[c - 1] * pot
        cand = [first_reaching(cs, r) for r in rv]
        if pot > 0:
            marg.extend(float(np.min(np.abs(cs - r)) / pot) for r in rv)
        dc = np.minimum(closest[:, None], np.maximum(sq_distances(X, nx, X[cand], dot), 0.0))
        pots = [ordered_sum(dc[:, t]) for t in range(len(cand))]
        b = 0
        for t in range(1, len(pots)):
            if pots[t] < pots[b]:
                b = t
        sp = np.sort(pots)
        if len(sp) > 1 and sp[1] > sp[0] and sp[0] > 0:
            marg.append(float((sp[1] - sp[0]) / sp[0]))
        pot, closest = pots[b], dc[:, b].copy()
        ids.append(cand[b])
    return ids


def assign(X, nx, C, marg, dot):
    D = sq_distances(X, nx, C, dot)
    lab = np.argmin(D, axis=1)  # the first smallest
    if marg is not None:
        s = np.sort(D, axis=1)
        marg.append(float(np.min((s[:, 1] - s[:, 0]) / np.maximum(np.abs(s[:, 1]), 1e-300))))
    return lab


def lloyd(X, nx, C, tol, max_iter, marg, dot):
    n, k = X.shape[0], C.shape[0]
    old = np.full(n, -1, dtype=np.int64)
    strict, it = False, 0
    for it in range(max_iter):
        lab = assign(X, nx, C, marg, dot)
        sums, cnt = centre_sums(X, lab, k)
        if (cnt == 0).any():
            raise EmptyCluster(f"a cluster lost all its rows (iteration {it})")
        Cn = sums / cnt[:, None].astype(np.float64)
        df = Cn - C
        per = seq_sum(df * df, 1)
        shift = np.float64(0.0)
        for j in range(k):
            shift = shift + per[j]
        C = Cn
        same = np.array_equal(lab, old)
        old = lab
        if same:
            strict = True
            break
        if tol > 0:
            marg.append(float(abs(shift - tol) / tol))
        if shift <= tol:
            break
    if not strict:
        old = assign(X, nx, C, marg, dot)
    df = X - C[old]
    inertia = ordered_sum(seq_sum(df * df, 1))
    return old, inertia, C, it + 1


def same_clustering(a, b, k):
    m = np.full(k, -1, dtype=np.int64)
    for x, y in zip(a, b):
        if m[x] == -1:
            m[x] = y
        elif m[x] != y:
            return False
    return True


def fit(X32, k, n_init, first=None, u=None, random_state=42, max_iter=300, tol_scale=1e-4, dot="ordered"):
    """dict(labels, centres, inertia, n_iter, best_init, tol, margin, inertias) of the best of n_init runs."""
    X = np.asarray(X32, dtype=np.float32).astype(np.float64)
    if first is None:
        first, u = draws(X.shape[0], k, n_init, random_state)
    nx = _norms(X, dot)
    tol = tolerance(X, tol_scale)
    marg, best, inertias = [], None, []
    for i in range(n_init):
        ids = kpp(X, nx, k, first[i], u[i], marg, dot)
        lab, ine, C, it = lloyd(X, nx, X[ids].copy(), tol, max_iter, marg, dot)
        inertias.append(float(ine))
        if best is None or (ine < best["inertia"] and not same_clustering(lab, best["labels"], k)):
            best = {"labels": lab.astype(np.int64), "centres": C, "inertia": float(ine), "n_iter": it, "best_init": i}
    best.update(tol=float(tol), margin=min(marg) if marg else float("inf"), inertias=inertias)
    return best


def find_elbow_point(k_values, inertias):
    """The reference's _find_elbow_point, its own expression."""
    if len(k_values) < 3:
        return k_values[0] if k_values else 2
    return k_values[int(np.argmax(np.diff(np.diff(inertias))) + 1)]


def find_optimal_k(X32, max_k=None, dot="ordered"):
    """(k, inertias, smallest margin) by the reference's _find_optimal_k loop: a fresh stream per k, n_init = 5."""
    n = len(X32)
    if max_k is None:
        max_k = min(10, n // 5)
    if max_k < 2:
        return 2, [], float("inf")
    ks = list(range(2, max_k + 1))
    fits = [fit(X32, k, 5, dot=dot) for k in ks]
    inertias = [f["inertia"] for f in fits]
    if len(inertias) < 2:
        return 2, inertias, min(f["margin"] for f in fits)
    return find_elbow_point(ks, inertias), inertias, min(f["margin"] for f in fits)


def make_rows(kind, n, d, seed):
    """The seeded inputs of tests/golden/kmeans_cases.npz (``np.random.default_rng(seed)``)."""
    g = np.random.default_rng(seed)
    if kind == "blobs":
        c = g.standard_normal((6, d))
        x = c[g.integers(0, 6, n)] + 0.35 * g.standard_normal((n, d))
    elif kind == "unit":
        c = g.standard_normal((7, d))
        x = c[g.integers(0, 7, n)] + 0.6 * g.standard_normal((n, d))
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    elif kind == "gauss":
        x = g.standard_normal((n, d))
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


KINDS = ("blobs", "unit", "gauss")


def load_golden(path):
    """The cases of kmeans_cases.npz as dicts; rows come from the file, or from their seed where the file holds only that
    (checked against the stored float64 checksum)."""
    z = np.load(path)
    cases = []
    for i in range(len(z["n"])):
        kind, n, d, seed = KINDS[int(z["kind"][i])], int(z["n"][i]), int(z["d"][i]), int(z["seed"][i])
        x = z[f"c{i}_x"] if f"c{i}_x" in z.files else make_rows(kind, n, d, seed)
        if float(x.astype(np.float64).sum()) != float(z["checksum"][i]):
            raise AssertionError(f"case {i}: the rows made from seed {seed} are not the recorded ones")
        cases.append({"name": f"{kind}-{n}x{d}-s{seed}", "x": x, "k": int(z["k"][i]), "labels": z[f"c{i}_labels"],
                      "n_iter": int(z["n_iter"][i]), "inertia": float(z["inertia"][i]), "elbow_inertias": z[f"c{i}_inertias"],
                      "fallback_labels": z[f"c{i}_fallback"], "fallback_inertia": float(z["fallback_inertia"][i]),
                      "fallback_n_iter": int(z["fallback_n_iter"][i]), "deviation": float(z["deviation"][i]),
                      "margin": float(z["margin"][i])})
    return cases, str(z["sklearn_version"]), float(z["max_deviation"])
