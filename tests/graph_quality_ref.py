"""numpy restatement of the device graph quality metrics (csrc/notegraph.hip), checked against the
reference's own compute_metrics through tests/golden/graph_quality_cases.npz.

  components      min-label: hook every edge's larger label to the smaller (np.minimum.at), jump labels = labels[labels]
                  until stable, repeat until no edge joins two labels
  hop_histogram   bit-parallel BFS: `words` uint64 words per node, bit j = source j of the pass; a level is
                  next = OR over the row of frontier[neighbour] (np.bitwise_or.reduceat over the CSR) & ~seen
  metrics         the reference's dict from those integers; the one float division is Python's int / int
"""
import numpy as np

_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def popcount(a):
    return int(_POP8[np.ascontiguousarray(a).view(np.uint8)].sum())


def csr(n, src, dst):
    """symmetric CSR (rowptr [n + 1], nbr [2E]), neighbours ascending inside a row"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    rows, cols = np.concatenate([src, dst]), np.concatenate([dst, src])
    order = np.lexsort((cols, rows))
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, cols[order]


def components(n, src, dst):
    """(labels int64 [n] = the smallest node index of the component, sizes in ascending-label order)"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    labels = np.arange(n, dtype=np.int64)
    while True:
        ls, ld = labels[src], labels[dst]
        diff = ls != ld
        if not diff.any():
            break
        np.minimum.at(labels, np.maximum(ls, ld)[diff], np.minimum(ls, ld)[diff])
        while True:
            nxt = labels[labels]
            if np.array_equal(nxt, labels):
                break
            labels = nxt
    roots = np.flatnonzero(labels == np.arange(n))
    return labels, [int(s) for s in np.bincount(labels, minlength=n)[roots]]


def hop_histogram(n, src, dst, sources=None, words=16):
    """counts[l] = the (source, node) pairs at hop distance l, int64"""
    rowptr, nbr = csr(n, src, dst)
    sources = np.arange(n, dtype=np.int64) if sources is None else np.asarray(sources, np.int64).reshape(-1)
    starts = rowptr[:-1][np.diff(rowptr) > 0]  # reduceat over the non-empty rows only
    has = np.diff(rowptr) > 0
    counts = [len(sources)] if len(sources) else []
    per_pass = 64 * words
    for s0 in range(0, len(sources), per_pass):
        part = sources[s0:s0 + per_pass]
        seen = np.zeros((n, words), np.uint64)
        j = np.arange(len(part))
        np.bitwise_or.at(seen, (part, j >> 6), np.uint64(1) << (j & 63).astype(np.uint64))
        frontier = seen.copy()
        level = 1
        while True:
            nxt = np.zeros((n, words), np.uint64)
            if len(nbr):
                nxt[has] = np.bitwise_or.reduceat(frontier[nbr], starts, axis=0)
            nxt &= ~seen
            added = popcount(nxt)
            if added == 0:
                break
            seen |= nxt
            if len(counts) <= level:
                counts += [0] * (level + 1 - len(counts))
            counts[level] += added
            frontier = nxt
            level += 1
    return np.asarray(counts, dtype=np.int64)


def metrics(n, src, dst, self_loops=0, words=16):
    """compute_metrics (graph/graph_quality.py) and the hop histogram of the largest component's nodes"""
    labels, sizes = components(n, src, dst)
    largest = max(sizes)
    root = np.flatnonzero(labels == np.arange(n))[sizes.index(largest)]
    hist = hop_histogram(n, src, dst, np.flatnonzero(labels == root), words)
    if largest > 1:
        aspl = sum(l * int(c) for l, c in enumerate(hist)) / (largest * (largest - 1))
    else:
        aspl = 0.0
    out = {
        "average_degree": (2 * len(src) + 2 * self_loops) / float(n),
        "num_components": float(len(sizes)),
        "largest_component_size": float(largest),
        "average_shortest_path_length": aspl,
        "component_sizes": sizes,
    }
    return out, hist


def ring_with_chords(n_nodes, ring, seed):
    """a graph of n_nodes nodes whose largest component is a ring of `ring` nodes (scattered over the index range) with
    a few chords; the rest are pairs and isolated nodes.  Returns (src, dst)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n_nodes)
    r = perm[:ring]
    src, dst = list(r), list(np.roll(r, -1))
    if ring < 3:
        src, dst = ([r[0]], [r[1]]) if ring == 2 else ([], [])
    pairs = {(min(a, b), max(a, b)) for a, b in zip(src, dst)}
    for _ in range(min(5, ring // 8)):
        a, b = rng.choice(r, 2, replace=False)
        if (min(a, b), max(a, b)) not in pairs:
            pairs.add((min(a, b), max(a, b)))
    rest = perm[ring:]
    for k in range(0, len(rest) // 2 - 1, 2):  # every other pair of the rest: components of 2, others isolated
        pairs.add((min(rest[2 * k], rest[2 * k + 1]), max(rest[2 * k], rest[2 * k + 1])))
    arr = np.asarray(sorted(pairs), dtype=np.int64).reshape(-1, 2)
    return arr[:, 0].copy(), arr[:, 1].copy()
