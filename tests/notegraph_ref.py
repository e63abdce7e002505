"""Plain numpy restatement of the note graph's two algorithms (csrc/notegraph.hip), with the summation orders the device
uses — the checker of the GPU tests, itself checked against the reference-run fixtures (tests/golden/notegraph_cases.npz).

PageRank (networkx 3.x _pagerank_scipy, uniform personalisation): x <- alpha * (x A + dangling(x) * p) + (1 - alpha) * p,
A[i][j] = (1 / S_i) * w_ij.  Orders: S_i adds row i's weights in ascending j from 0.0; x A adds x[i] * A[i][j] over row j
in ascending i from 0.0; the dangling mass and the L1 change are `tree_sum`s.

retrieve (graph/graph_retriever.py:61-92): per seed the fixed point of d[v] = min(d[v], d[u] + w) over nodes with
d[u] <= cutoff (candidates beyond the cutoff dropped), merged in seed order, scored (c / (d + 1e-5)) * imp, ordered by
(score descending, seed position, dist, id).
"""
import numpy as np

CHUNK, THREADS = 1024, 256


def build_csr(n, src, dst, w):
    """symmetric CSR, neighbours ascending inside a row: rowptr int64 [n + 1], nbr int64, wt float64"""
    r = np.concatenate([src, dst]).astype(np.int64)
    c = np.concatenate([dst, src]).astype(np.int64)
    ww = np.concatenate([w, w]).astype(np.float64)
    order = np.lexsort((c, r))
    r, c, ww = r[order], c[order], ww[order]
    rowptr = np.searchsorted(r, np.arange(n + 1), side="left").astype(np.int64)
    return rowptr, c, ww


def _fold(v):
    """v [rows, 256] -> [rows]: v[t] += v[t + s] for s = 128, 64, ..., 1"""
    v = v.copy()
    s = THREADS // 2
    while s > 0:
        v[:, :s] = v[:, :s] + v[:, s:2 * s]
        s //= 2
    return v[:, 0]


def tree_sum(v):
    """the device's fixed-shape sum: chunks of 1024 (thread t adds elements t, t + 256, t + 512, t + 768 in that order,
    then the fold), and the chunk sums again (thread t adds sums t, t + 256, ... in order, then the fold)"""
    v = np.asarray(v, dtype=np.float64)
    nb = max(1, -(-len(v) // CHUNK))
    pad = np.zeros(nb * CHUNK)
    pad[:len(v)] = v
    e = pad.reshape(nb, CHUNK // THREADS, THREADS)
    t = np.zeros((nb, THREADS))
    for k in range(CHUNK // THREADS):
        t = t + e[:, k, :]
    part = _fold(t)
    rows = -(-nb // THREADS)
    pad = np.zeros(rows * THREADS)
    pad[:nb] = part
    e = pad.reshape(rows, THREADS)
    t = np.zeros((1, THREADS))
    for k in range(rows):
        t = t + e[k][None, :]
    return float(_fold(t)[0])


def _row_sums_in_order(rowptr, values, n):
    """per row, the values added one at a time in storage order, from 0.0"""
    deg = np.diff(rowptr)
    acc = np.zeros(n)
    for k in range(int(deg.max()) if n and len(values) else 0):
        rows = np.flatnonzero(deg > k)
        acc[rows] = acc[rows] + values[rowptr[rows] + k]
    return acc


def pagerank(n, rowptr, nbr, wt, alpha=0.85, max_iter=100, tol=1.0e-6):
    """(x, iterations); raises RuntimeError without convergence (networkx: PowerIterationFailedConvergence)"""
    S = _row_sums_in_order(rowptr, wt, n)
    inv = np.zeros(n)
    inv[S != 0] = 1.0 / S[S != 0]
    a = inv[nbr] * wt                      # A[i][j] at entry (row j, neighbour i): a reciprocal times the weight
    dangling = S == 0
    p = 1.0 / n
    omp = (1.0 - alpha) * p
    x = np.full(n, p)
    for it in range(max_iter):
        dsum = tree_sum(np.where(dangling, x, 0.0))
        acc = _row_sums_in_order(rowptr, x[nbr] * a, n)
        xn = alpha * (acc + dsum * p) + omp
        err = tree_sum(np.abs(xn - x))
        x = xn
        if err < n * tol:
            return x, it + 1
    raise RuntimeError(f"no convergence in {max_iter} iterations")


def distances(n, rowptr, nbr, wt, seed, cutoff):
    """bounded single-source distances: inf where the node is not reached within the cutoff"""
    d = np.full(n, np.inf)
    d[seed] = 0.0
    rows = np.flatnonzero(np.diff(rowptr) > 0)
    if len(rows) == 0:
        return d
    while True:
        cand = d[nbr] + wt
        cand[~(cand <= cutoff)] = np.inf
        new = d.copy()
        new[rows] = np.minimum(d[rows], np.minimum.reduceat(cand, rowptr[rows]))
        if np.array_equal(new, d):
            return d
        d = new


def retrieve(n, rowptr, nbr, wt, seeds, cutoff, centrality, importance):
    """(ids, dist, score, seed_pos) of one seed list, best first"""
    visited = np.zeros(n, dtype=bool)
    ids, dist, pos = [], [], []
    for k, s in enumerate(seeds):
        if s < 0 or s >= n:
            continue
        d = distances(n, rowptr, nbr, wt, int(s), cutoff)
        reach = (d <= cutoff) & ~visited
        reach[s] = False                    # the seed is skipped, but not marked visited
        got = np.flatnonzero(reach)
        visited[got] = True
        ids.append(got)
        dist.append(d[got])
        pos.append(np.full(len(got), k, dtype=np.int32))
    if not ids:
        return (np.zeros(0, np.int64), np.zeros(0), np.zeros(0), np.zeros(0, np.int32))
    ids, dist, pos = np.concatenate(ids), np.concatenate(dist), np.concatenate(pos)
    score = (centrality[ids] / (dist + 1e-5)) * importance[ids]
    order = np.lexsort((ids, dist, pos, -score))
    return ids[order].astype(np.int64), dist[order], score[order], pos[order]
