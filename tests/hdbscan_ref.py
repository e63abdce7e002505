"""HDBSCAN as sklearn 1.7 computes it for ``metric='euclidean'`` (its Prim path), restated in numpy / plain Python from the
behaviour: the checker of ``anr_index_hdbscan_mst`` and ``anr_hdbscan_labels``.

* distance: float64 ``sqrt(sum_k (x_k - y_k) * (x_k - y_k))``, k ascending, every operation rounded on its own;
* core distance: the ``min_samples``-th smallest distance of a row to all rows, itself included;
* spanning tree: Prim from row 0 over ``max(core_a, core_b, dist)``; the next row is the smallest (value, row) pair, so a
  tie goes to the lowest row;
* labels: edges sorted by weight (``tie_order`` says what happens to equal weights: ``'stable'`` keeps Prim's order,
  ``'reversed'`` turns it round), single linkage, condensed tree, stability, excess of mass without a single cluster,
  ``cluster_selection_epsilon``, labels by ascending cluster id and -1 for noise.
"""
from __future__ import annotations

import os
from collections import deque

import numpy as np

_cache = {"key": None, "dist": None}


def distance_matrix(x) -> np.ndarray:
    """[N, N] float64 Euclidean distances of the rows, accumulated column by column (k ascending, no fused operation).
    The last matrix is kept: ``core_distances`` and ``prim_mst`` of the same rows share it."""
    x64 = np.ascontiguousarray(x, dtype=np.float64)
    key = (x64.shape, hash(x64.tobytes()))
    if _cache["key"] == key:
        return _cache["dist"]
    n, d = x64.shape
    out = np.empty((n, n), dtype=np.float64)
    xt = np.ascontiguousarray(x64.T)
    step = 128
    for i in range(0, n, step):
        acc = np.zeros((min(step, n - i), n), dtype=np.float64)
        for k in range(d):
            t = x64[i:i + step, k][:, None] - xt[k][None, :]
            t *= t
            acc += t
        np.sqrt(acc, out=out[i:i + step])
    _cache["key"], _cache["dist"] = key, out
    return out


def core_distances(x, min_samples: int) -> np.ndarray:
    dist = distance_matrix(x)
    return np.ascontiguousarray(np.partition(dist, min_samples - 1, axis=1)[:, min_samples - 1])


def prim_mst(x, core):
    """(src int64, dst int64, w float64), N - 1 edges in the order Prim adds them, starting at row 0."""
    dist = distance_matrix(x)
    n = dist.shape[0]
    core = np.asarray(core, dtype=np.float64)
    in_tree = np.zeros(n, dtype=bool)
    reach = np.full(n, np.inf)
    source = np.ones(n, dtype=np.int64)
    src = np.empty(n - 1, dtype=np.int64)
    dst = np.empty(n - 1, dtype=np.int64)
    w = np.empty(n - 1, dtype=np.float64)
    cur = 0
    for i in range(n - 1):
        in_tree[cur] = True
        m = np.maximum(np.maximum(core[cur], core), dist[cur])
        upd = (m < reach) & ~in_tree
        reach[upd] = m[upd]
        source[upd] = cur
        j = int(np.argmin(np.where(in_tree, np.inf, reach)))  # the first smallest: ties to the lowest row
        src[i], dst[i], w[i] = source[j], j, reach[j]
        cur = j
    return src, dst, w


def labels_from_mst(src, dst, w, min_cluster_size: int, eps: float, tie_order: str = "stable") -> np.ndarray:
    src, dst, w = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64), np.asarray(w, dtype=np.float64)
    m = len(w)
    n = m + 1
    if tie_order == "stable":
        order = np.argsort(w, kind="stable")
    elif tie_order == "reversed":
        order = np.lexsort((-np.arange(m), w))
    else:
        raise ValueError(tie_order)

    # single linkage: merge i makes node n + i of the two nodes that hold the edge's ends
    up = list(range(2 * n - 1))
    size = [1] * n + [0] * m
    left, right, height = [0] * m, [0] * m, [0.0] * m

    def find(a):
        r = a
        while up[r] != r:
            r = up[r]
        while up[a] != r:
            up[a], a = r, up[a]
        return r

    for i, e in enumerate(order):
        a, b = find(int(src[e])), find(int(dst[e]))
        left[i], right[i], height[i] = a, b, float(w[e])
        size[n + i] = size[a] + size[b]
        up[a] = up[b] = n + i

    def points_of(node):
        out, stack = [], [node]
        while stack:
            v = stack.pop()
            if v < n:
                out.append(v)
            else:
                stack.append(left[v - n])
                stack.append(right[v - n])
        return out

    # condensed tree: clusters n (the root), n + 1, .. in breadth-first order of the splits that make them
    parent_of = [n]       # cluster c - n -> its parent cluster (the root: itself)
    birth = [0.0]         # lambda at which the cluster appears
    stability = [0.0]
    children = [[]]
    point_cluster = [n] * n
    queue = deque([(2 * n - 2, n)])
    while queue:
        node, c = queue.popleft()
        a, b, dd = left[node - n], right[node - n], height[node - n]
        lam = 1.0 / dd if dd > 0.0 else float("inf")
        big_a, big_b = size[a] >= min_cluster_size, size[b] >= min_cluster_size
        if big_a and big_b:
            for side in (a, b):
                cc = n + len(parent_of)
                parent_of.append(c), birth.append(lam), stability.append(0.0), children.append([])
                children[c - n].append(cc)
                stability[c - n] += (lam - birth[c - n]) * size[side]
                queue.append((side, cc))
        else:
            for side, big in ((a, big_a), (b, big_b)):
                if big:
                    queue.append((side, c))
                else:
                    for p in points_of(side):
                        point_cluster[p] = c
                        stability[c - n] += (lam - birth[c - n]) * 1
    n_cl = len(parent_of)

    # excess of mass, the root never selected: from the highest id down
    selected = [True] * n_cl
    selected[0] = False
    for c in range(n_cl - 1, 0, -1):
        sub = 0.0
        for ch in children[c]:
            sub = sub + stability[ch - n]
        if sub > stability[c]:
            selected[c] = False
            stability[c] = sub
        else:
            stack = list(children[c])
            while stack:
                v = stack.pop()
                selected[v - n] = False
                stack.extend(children[v - n])

    if eps != 0.0 and n_cl > 1:
        chosen = set()
        done = [False] * n_cl
        for c in range(n_cl - 1, 0, -1):
            if not selected[c]:
                continue
            if 1.0 / birth[c] < eps:
                if done[c]:
                    continue
                v = c  # climb to the first ancestor born at a distance above eps; a child of the root stays
                while True:
                    p = parent_of[v] - n
                    if p == 0:
                        break
                    v = p
                    if 1.0 / birth[p] > eps:
                        break
                chosen.add(v)
                stack = list(children[v])
                while stack:
                    u = stack.pop()
                    done[u - n] = True
                    stack.extend(children[u - n])
            else:
                chosen.add(c)
        selected = [i in chosen for i in range(n_cl)]

    number = {}
    for c in range(1, n_cl):
        if selected[c]:
            number[c] = len(number)
    labels = np.full(n, -1, dtype=np.int64)
    for p in range(n):
        c = point_cluster[p] - n
        while c != 0 and not selected[c]:
            c = parent_of[c] - n
        if c != 0:
            labels[p] = number[c]
    return labels


def hdbscan_labels(x, min_cluster_size: int, min_samples: int, eps: float, tie_order: str = "stable") -> np.ndarray:
    core = core_distances(x, min_samples)
    return labels_from_mst(*prim_mst(x, core), min_cluster_size, eps, tie_order)


def count_ties(w) -> int:
    w = np.asarray(w)
    return int(len(w) - len(np.unique(w)))


DUP_BLOCK = 9  # rows 10 .. 18 of a 'dups' input are one row


def make_rows(kind: str, n: int, d: int, seed: int) -> np.ndarray:
    """float32 [n, d]: 'blobs' Gaussian centres plus noise; 'dups' blobs with a block of DUP_BLOCK identical rows;
    'lattice' coordinates in 0 .. 5, so that very many distances are exactly equal; 'gauss' isotropic."""
    rng = np.random.default_rng(seed)
    if kind in ("blobs", "dups"):
        k = max(2, min(12, n // 40))
        cent = rng.standard_normal((k, d)).astype(np.float32)
        x = (cent[rng.integers(0, k, n)] + 0.35 * rng.standard_normal((n, d))).astype(np.float32)
        if kind == "dups":
            x[10:10 + DUP_BLOCK] = x[10]
        return x
    if kind == "lattice":
        return rng.integers(0, 6, (n, d)).astype(np.float32)
    if kind == "gauss":
        return rng.standard_normal((n, d)).astype(np.float32)
    raise ValueError(kind)


KINDS = ("blobs", "dups", "lattice", "gauss")


def load_cases():
    """the recorded cases of tests/golden/hdbscan_cases.npz as dicts; rows stored as a seed alone are made again"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdbscan_cases.npz"))
    cases = []
    for i in range(len(g["n"])):
        c = {k: g[k][i].item() for k in ("n", "d", "seed", "min_cluster_size", "min_samples", "eps", "n_ties", "checksum")}
        c["kind"] = KINDS[int(g["kind"][i])]
        c["x"] = g[f"c{i}_x"] if f"c{i}_x" in g.files else make_rows(c["kind"], c["n"], c["d"], c["seed"])
        for k in ("labels", "core", "src", "dst", "w"):
            c[k] = g[f"c{i}_{k}"]
        c["id"] = f"{c['kind']}-{c['n']}x{c['d']}-ms{c['min_samples']}"
        cases.append(c)
    return cases
