"""Plain-Python restatement of the second hop of the reference's multi-hop query path: the rerank of
``QueryProcessor._rerank_khop_candidates`` (query/query_processor.py:1549-1635) and the greedy near-duplicate suppression of
``_apply_cluster_suppression`` (:1637-1697).  Python floats only, in the reference's order of operations; what the device
(``anr_index_khop_rerank`` / ``anr_index_cluster_suppress``) is compared with, and itself pinned to the reference's own
code by tests/golden/khop_cases.json (tests/test_khop_cpu.py)."""
import json
import math
import os
import struct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "khop_cases.json")
FUSION_DEFAULTS = {"dense_weight": 1.0, "bm25_weight": 0.6, "focused_weight_hop2": 0.30, "rrf_lambda": 0.2}
FEATURE_DEFAULTS = {"hop_decay": 0.85, "cov_weight": 0.10, "cons_weight": 0.05}
RRF_K = 50
U = 2.0 ** -53


def load_cases():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)


def bits(x):
    return struct.pack("<d", float(x)).hex()


def _float_or(d, key, default):
    try:
        return float(d.get(key, default))
    except (TypeError, ValueError):
        return default


def parse_config(config):
    """the weights and the suppression settings as the reference reads them: its defaults, and the default again where a
    value cannot be parsed (:1556-1583, :1643-1659)"""
    fus = config.get("fusion") or {}
    feat = config.get("features") or {}
    cs = config.get("cluster_suppression") or {}
    w = {k: _float_or(fus, k, v) for k, v in FUSION_DEFAULTS.items()}
    w.update({k: _float_or(feat, k, v) for k, v in FEATURE_DEFAULTS.items()})
    enabled = cs.get("enabled", True)
    if isinstance(enabled, str):
        enabled = enabled.strip().lower() not in {"false", "0", "no"}
    else:
        enabled = bool(enabled)
    thr = _float_or(cs, "cos_threshold", 0.90)
    try:
        keep_m = int(cs.get("keep_per_cluster", 2))
    except (TypeError, ValueError):
        keep_m = 2
    return w, enabled, thr, keep_m


def cov_cons(note, path_entities):
    """entity coverage and path consistency (:843-852)"""
    ne = set(note.get("entities") or [])
    pe = set(e.lower() for e in (path_entities or []))
    if not pe:
        return 0.0, 0
    cov = len({e.lower() for e in ne} & pe) / max(1, len(pe))
    text = f"{note.get('title', '')} {note.get('content', '')}".lower()
    return float(cov), int(1 if any(e in text for e in pe) else 0)


def decay_factor(hop_decay, hop_no):
    """what the final score is multiplied by (:1628-1629); 1.0 where the reference does not multiply"""
    if hop_no > 1 and 0.0 < hop_decay < 1.0:
        return hop_decay ** (hop_no - 1)
    return 1.0


def ranks_desc(scores, on=None):
    """1-based rank of every entry by score descending, ties in list order; entries with on[i] false are left out (rank 0)"""
    idx = [i for i in range(len(scores)) if on is None or on[i]]
    idx.sort(key=lambda i: scores[i], reverse=True)   # stable, also when reversed
    out = [0] * len(scores)
    for r, i in enumerate(idx):
        out[i] = r + 1
    return out


def rerank(dense, focused, bm25, is_prf, prf_sim, cov, cons, hop_no, decay, w, rrf_k=RRF_K):
    """final score of every candidate and the stable order by it, best first"""
    n = len(dense)
    rd, rb, rp = ranks_desc(dense), ranks_desc(bm25), ranks_desc(prf_sim, is_prf)
    final = []
    for c in range(n):
        rrf = 0.0 + 1.0 / (rrf_k + rd[c])
        rrf = rrf + 1.0 / (rrf_k + rb[c])
        if is_prf[c]:
            rrf = rrf + 1.0 / (rrf_k + rp[c])
        base = w["dense_weight"] * dense[c] + w["bm25_weight"] * bm25[c]
        fw2 = w["focused_weight_hop2"]
        fw = fw2 if hop_no[c] == 2 else max(0.0, fw2 - 0.10 * (hop_no[c] - 2))
        f = base + fw * focused[c] + w["cov_weight"] * cov[c] + w["cons_weight"] * cons[c] + w["rrf_lambda"] * rrf
        f = f * decay[c]
        final.append(float(f))
    order = sorted(range(n), key=lambda c: final[c], reverse=True)
    return final, order


def suppress(cos, score, thr, keep_m):
    """positions kept, in final order.  ``cos(i, j)`` for j > i; ``score`` the candidates' final_score"""
    n = len(score)
    kept, used = [], set()
    for i in range(n):
        if i in used:
            continue
        cluster = [i] + [j for j in range(i + 1, n) if j not in used and cos(i, j) >= thr]
        cluster.sort(key=lambda k: score[k], reverse=True)
        kept.extend(cluster[:keep_m])
        used.update(cluster)
    kept.sort(key=lambda k: score[k], reverse=True)
    return kept


def dot_fsum(a, b):
    return math.fsum(float(x) * float(y) for x, y in zip(a, b))   # float32 products are exact in float64


def cosine_clamped(q, x):
    """max(0.0, q . x / (|q| |x|)), 0.0 where a norm is zero; correctly rounded sums"""
    nq, nx = math.sqrt(dot_fsum(q, q)), math.sqrt(dot_fsum(x, x))
    if nq == 0.0 or nx == 0.0:
        return 0.0
    return max(0.0, dot_fsum(q, x) / (nq * nx))


def cosine_eps_matrix(rows):
    """G_ij / ((|x_i| + 1e-8) (|x_j| + 1e-8)) in float64 (numpy; for the suppression's inputs and margins)"""
    import numpy as np
    a = np.asarray(rows, dtype=np.float64)
    if a.shape[0] == 0:
        return np.zeros((0, 0))
    g = a @ a.T
    n = np.sqrt(np.einsum("ij,ij->i", a, a)) + 1e-8
    return g / (n[:, None] * n[None, :])


def case_inputs(case):
    """per-candidate arrays of a rerank case, from the fields the reference read"""
    w, enabled, thr, keep_m = parse_config(case["config"])
    cands = case["candidates"]
    cc = [cov_cons(c, case["path_entities"]) for c in cands]
    hop = [int(c.get("hop_no", 1)) for c in cands]
    return {
        "w": w, "enabled": enabled, "thr": thr, "keep_m": keep_m,
        "dense": [float(v) for v in case["dense"]],
        "focused": [float(v) if case["has_focus"] else 0.0 for v in case["focused"]],
        "bm25": [float(v) for v in case["bm25"]],
        "is_prf": [c.get("retrieval_method") == "prf_bridge" for c in cands],
        "prf_sim": [float(c.get("similarity_score", 0.0)) for c in cands],
        "cov": [v[0] for v in cc], "cons": [v[1] for v in cc], "hop_no": hop,
        "decay": [decay_factor(w["hop_decay"], h) for h in hop],
    }


def restate_case(case):
    """(final, order, kept) of a golden case: positions of the case's candidate list"""
    import numpy as np
    if case["kind"] == "suppress":
        _, enabled, thr, keep_m = parse_config(case["config"])
        score = [float(v) for v in case["scores"]]
        if not enabled:
            return None, None, list(range(len(score)))
        sim = cosine_eps_matrix(np.asarray(case["vectors"], dtype=np.float32).reshape(len(score), -1))
        return None, None, suppress(lambda i, j: sim[i, j], score, thr, keep_m)
    a = case_inputs(case)
    final, order = rerank(a["dense"], a["focused"], a["bm25"], a["is_prf"], a["prf_sim"], a["cov"], a["cons"], a["hop_no"],
                          a["decay"], a["w"])
    if not a["enabled"]:
        return final, order, list(order)
    sim = cosine_eps_matrix(np.asarray(case["vectors"], dtype=np.float32).reshape(len(final), -1))
    kept = suppress(lambda i, j: sim[order[i], order[j]], [final[c] for c in order], a["thr"], a["keep_m"])
    return final, order, [order[k] for k in kept]
