"""numpy restatement of the graph index of csrc/graph.hip (anr_index_graph_*): the kNN lists, the rank-only prune with
reverse edges (integers only), the int8 traversal image and query codes, and the beam search with float64 traversal
scores (which equal the device's integer-exact ones) and a float64 re-score of the beam."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
ENTRY_SAMPLE = 4096


def knn_lists(I, K):
    """[n, K + 1] exact top-(K + 1) ids of every stored row (ties by ascending id, -1 padded) -> [n, K]: the row's own
    id dropped, or the last entry when the own id is absent (un-normalised IP)"""
    out = np.empty((I.shape[0], K), dtype=np.int32)
    for i, row in enumerate(np.asarray(I).tolist()):
        j = row.index(i) if i in row else K
        del row[j]
        out[i] = row
    return out


def detours(L):
    """detour(i, r) = #{s < r : L[i, r] appears in L[L[i, s]] at a position < r}, plain loops"""
    n, K = L.shape
    det = np.zeros((n, K), dtype=np.int64)
    for i in range(n):
        pos = {int(v): r for r, v in enumerate(L[i]) if v >= 0}
        for s in range(K):
            ns = int(L[i, s])
            if ns < 0:
                continue
            for t, m in enumerate(L[ns].tolist()):
                r = pos.get(m, -1)
                if r > s and r > t:
                    det[i, r] += 1
    return det


def forward_order(L, det=None):
    """F: the valid entries of every list stably sorted by (detour, rank), the -1 padding after them"""
    L = np.asarray(L, dtype=np.int32)
    n, K = L.shape
    if det is None:
        det = detours_fast(L)
    key = np.where(L >= 0, det * K + np.arange(K)[None, :], np.iinfo(np.int64).max)
    return np.take_along_axis(L, np.argsort(key, axis=1, kind="stable"), axis=1)


def detours_fast(L, chunk=512):
    """detours(), vectorised over rows (a sorted key table per chunk of rows instead of a dict per row)"""
    L = np.asarray(L, dtype=np.int64)
    n, K = L.shape
    det = np.zeros((n, K), dtype=np.int64)
    s_idx = np.arange(K)[None, :, None]
    t_idx = np.arange(K)[None, None, :]
    for a in range(0, n, chunk):
        Lc = L[a:a + chunk]
        c = len(Lc)
        base = (np.arange(c, dtype=np.int64) * (n + 1))[:, None]
        keys = np.where(Lc >= 0, base + Lc, -1).ravel()
        order = np.argsort(keys, kind="stable")
        sk, rank = keys[order], order % K
        LN = np.where(Lc[:, :, None] >= 0, L[np.maximum(Lc, 0)], -1)           # [c, s, t]
        q = np.where(LN >= 0, base[:, :, None] + LN, -2).ravel()
        at = np.minimum(np.searchsorted(sk, q), len(sk) - 1)
        r = np.where(sk[at] == q, rank[at], -1).reshape(c, K, K)
        ok = (r > s_idx) & (r > t_idx)
        rows = np.broadcast_to(np.arange(c)[:, None, None], r.shape)
        det[a:a + c] = np.bincount((rows[ok] * K + r[ok]).ravel(), minlength=c * K).reshape(c, K)
    return det


def prune(L, R, F=None):
    """[n, R] adjacency: first the first R/2 entries of F_i; then the rows j with i among the first R/2 entries of F_j,
    in (position of i in F_j, j) order, skipping duplicates, up to R; then the rest of F_i, skipping duplicates; -1
    padding"""
    F = forward_order(L) if F is None else F
    n, K = F.shape
    half = min(R // 2, K)
    rev = [[] for _ in range(n)]
    for pos in range(half):
        col = F[:, pos]
        for i in np.flatnonzero(col >= 0).tolist():
            rev[col[i]].append(i)
    adj = np.full((n, R), -1, dtype=np.int32)
    for i in range(n):
        out, seen = [], set()
        for v in list(F[i, :half]) + rev[i] + list(F[i, half:]):
            v = int(v)
            if len(out) == R:
                break
            if v >= 0 and v not in seen:
                seen.add(v)
                out.append(v)
        adj[i, :len(out)] = out
    return adj


def quantize(x):
    """int8 codes and power-of-two exponents, per row: scale 2^(E - 7) with max|x| = m 2^E, m in [0.5, 1)"""
    x = np.asarray(x, dtype=np.float32)
    m = np.abs(x).max(axis=1) if x.shape[1] else np.zeros(len(x), np.float32)
    _, E = np.frexp(m)
    e = np.where(m > 0, E - 7, 0).astype(np.int32)
    codes = np.clip(np.rint(np.ldexp(x, -e[:, None])), -127, 127).astype(np.int8)
    return codes, e


def decode(codes, e):
    return np.ldexp(codes.astype(np.float32), np.asarray(e, np.int32)[:, None])


def prepare(q, normalize):
    """k_prepq: every row divided by the float32 of its float64 norm (zero rows unchanged)"""
    q = np.asarray(q, dtype=np.float32)
    if not normalize:
        return q
    s = np.sqrt((q.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    return np.where(s[:, None] != 0, q / np.where(s == 0, 1, s)[:, None], q).astype(np.float32)


def search_one(qp, image, x32, adj, k, ef, metric, forget_every=0):
    """Beam search of one prepared query: (D [k], I [k], iterations, rows scored, capped).

    image: decoded traversal rows (float32, exact); the traversal key is q.x (IP) or 2 q.x - |x|^2 (L2) of the decoded
    query and row in float64.  Beam ef' = max(ef, k) rounded up to a power of two >= 64; the rows floor(i * n / S),
    i < S = min(n, 4096), are scored first and the best ef' of them start the beam; each iteration expands the first
    p = 256 // R unexpanded beam entries, scores their unvisited neighbours and keeps the best ef' of beam + candidates
    by (key desc, id asc); it stops when the whole beam is expanded or after ef' iterations.  forget_every > 0 clears
    the visited set every that many iterations (down to the beam's ids), as the device's hash does when it fills: the
    result must not change."""
    n, R = adj.shape
    efp = 64
    while efp < max(ef, k):
        efp *= 2
    p = max(1, 256 // R)
    qc, qe = quantize(qp[None, :])
    qd = decode(qc, qe)[0].astype(np.float64)
    X = np.asarray(image, dtype=np.float64)

    def keys(ids):
        xs = X[ids]
        s = xs @ qd
        return s if metric == "ip" else 2.0 * s - (xs * xs).sum(axis=1)

    S = min(n, ENTRY_SAMPLE)
    entry = np.arange(S, dtype=np.int64) * n // S
    visited = set(entry.tolist())
    beam = sorted([[-kk, int(i), False] for kk, i in zip(keys(entry), entry)], key=lambda e: (e[0], e[1]))[:efp]
    iters, scored, capped = 0, S, False
    while True:
        parents = [e for e in beam if not e[2]][:p]
        if not parents:
            break
        if iters == efp:
            capped = True
            break
        for e in parents:
            e[2] = True
        iters += 1
        if forget_every and iters % forget_every == 0:
            visited = {e[1] for e in beam}
        cand = []
        for e in parents:
            for v in adj[e[1]].tolist():
                if v >= 0 and v not in visited:
                    visited.add(v)
                    cand.append(v)
        scored += len(cand)
        if cand:
            ks = keys(np.array(cand, dtype=np.int64))
            beam = sorted(beam + [[-kk, c, False] for kk, c in zip(ks, cand)], key=lambda e: (e[0], e[1]))[:efp]
    ids = np.array([e[1] for e in beam], dtype=np.int64)
    xs = np.asarray(x32, dtype=np.float64)[ids]
    q64 = qp.astype(np.float64)
    s = xs @ q64 if metric == "ip" else ((xs - q64) ** 2).sum(axis=1)
    key = s if metric == "ip" else -s
    order = sorted(range(len(ids)), key=lambda j: (-key[j], ids[j]))[:k]
    D = np.full(k, -FLT_MAX if metric == "ip" else FLT_MAX, dtype=np.float32)
    I = np.full(k, -1, dtype=np.int64)
    D[:len(order)] = s[order]
    I[:len(order)] = ids[order]
    return D, I, iters, scored, capped


def search(qp, image, x32, adj, k, ef, metric, forget_every=0):
    out = [search_one(q, image, x32, adj, k, ef, metric, forget_every) for q in np.asarray(qp, np.float32)]
    D = np.stack([o[0] for o in out]) if out else np.zeros((0, k), np.float32)
    I = np.stack([o[1] for o in out]) if out else np.zeros((0, k), np.int64)
    return D, I, [o[2] for o in out], [o[3] for o in out], [o[4] for o in out]
