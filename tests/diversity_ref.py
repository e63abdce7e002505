"""numpy float64 restatement of the diversity scheduler's arithmetic (reference retrieval/diversity_scheduler.py): the
cosine rule (:431-444) and the decision procedure on a similarity matrix — dedup (:383-401), pass-through (:655), stable
sort (:659), quota round one (:698-719), greedy fill (:666-687, :724-754, :761-805).  The checker of anr_index_diversify
and of the drop-in's host loop; plain loops, no vectorised shortcuts, so the order of every float64 operation is the
reference's.

``schedule`` also returns the smallest decision margin it met: |sim - threshold| over the pairs the dedup compared, and
best minus runner-up at every greedy step (a runner-up whose inputs are bit-identical to the best is skipped: that tie
is decided by position, not by arithmetic).  A golden case or a seeded test input is one whose margin exceeds 1e-9."""
import numpy as np

MARGIN = 1e-9


def cosine_matrix(rows):
    """clamp(a_i . a_j / (|a_i| |a_j|), 0, 1) in float64 on the rows as given; 0 where a norm is zero"""
    a = np.asarray(rows, dtype=np.float64)
    n = a.shape[0]
    g = np.einsum("ik,jk->ij", a, a)   # one summation loop per pair: equal rows give equal columns
    nrm = np.sqrt(np.einsum("ij,ij->i", a, a))
    out = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        for j in range(n):
            if nrm[i] == 0.0 or nrm[j] == 0.0:
                continue
            out[i, j] = max(0.0, min(1.0, float(g[i, j] / (nrm[i] * nrm[j]))))
    return out


def cosine_matrix_fast(rows):
    """the same values with array operations (for the larger GPU shapes)"""
    a = np.asarray(rows, dtype=np.float64)
    g = a @ a.T
    nrm = np.sqrt(np.einsum("ij,ij->i", a, a))
    den = nrm[:, None] * nrm[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = g / den
    s = np.where(s < 1.0, s, 1.0)
    s = np.where(s > 0.0, s, 0.0)
    s[den == 0.0] = 0.0
    return s


def word_jaccard(t1, t2):
    w1, w2 = set(t1.lower().split()), set(t2.lower().split())
    if not w1 or not w2:
        return 0.0
    u = len(w1 | w2)
    return len(w1 & w2) / u if u > 0 else 0.0


def set_jaccard(a, b):
    s1, s2 = set(a), set(b)
    if not s1 or not s2:
        return 0.0
    u = len(s1 | s2)
    return len(s1 & s2) / u if u > 0 else 0.0


def _bonus(mask, counts, quotas, balance):
    bonus = 0.0
    for t in range(32):
        if not (mask >> t) & 1:
            continue
        quota = quotas[t] if t < len(quotas) else 0
        if quota > 0:
            fill = counts[t] / quota
            if fill < balance:
                bonus += (balance - fill) * 0.5
    return bonus


def dedup(sim, scores, threshold):
    """-> kept positions in kept order, smallest |sim - threshold| compared, events (replaced, dropped)"""
    kept, margin, replaced, dropped = [], np.inf, 0, 0
    for i in range(len(scores)):
        hit = None
        for p, k in enumerate(kept):
            s = sim[i][k]
            margin = min(margin, abs(s - threshold))
            if s >= threshold:
                hit = p
                break
        if hit is None:
            kept.append(i)
        elif scores[i] > scores[kept[hit]]:
            del kept[hit]
            kept.append(i)
            replaced += 1
        else:
            dropped += 1
    return kept, margin, replaced, dropped


def select(sim, scores, masks, kept, max_candidates, quota, quotas, balance):
    """-> selected positions in selection order, smallest best-minus-runner-up of the greedy steps, info dict"""
    info = {"passthrough": False, "round_two_picks": 0, "stopped_short": False, "round_one": 0}
    if len(kept) <= max_candidates:
        info["passthrough"] = True
        return list(kept), np.inf, info
    order = sorted(range(len(kept)), key=lambda p: (-scores[kept[p]], p))   # stable, descending
    srt = [kept[p] for p in order]
    counts = [0] * 32
    selected, taken = [], [False] * len(srt)
    if quota:
        for pos, c in enumerate(srt):
            if len(selected) >= max_candidates:
                break
            m = int(masks[c])
            if any((m >> t) & 1 and counts[t] < (quotas[t] if t < len(quotas) else 0) for t in range(32)):
                selected.append(c)
                taken[pos] = True
                for t in range(32):
                    if (m >> t) & 1:
                        counts[t] += 1
        info["round_one"] = len(selected)
    else:
        selected.append(srt[0])
        taken[0] = True
    margin = np.inf
    while len(selected) < max_candidates and not all(taken):
        best, bpos, vals = -1.0, None, []
        for pos, c in enumerate(srt):
            if taken[pos]:
                continue
            if selected:
                total = 0.0
                for s in selected:
                    total += sim[s][c]
                gain = 0.7 * (1.0 - total / len(selected)) + 0.3 * min(1.0, scores[c])
            else:
                gain = 1.0
            v = gain
            if quota:
                v = scores[c] * 0.5 + gain * 0.3 + _bonus(int(masks[c]), counts, quotas, balance) * 0.2
            vals.append((pos, v))
            if v > best:
                best, bpos = v, pos
        if bpos is None:
            info["stopped_short"] = True
            # the nearest miss of the -1.0 start
            margin = min(margin, min((-1.0 - v for _, v in vals if v == v), default=np.inf))
            break
        cb = srt[bpos]
        margin = min(margin, best + 1.0)
        for pos, v in vals:
            if pos == bpos:
                continue
            c = srt[pos]
            same = (scores[c] == scores[cb] and int(masks[c]) == int(masks[cb])
                    and all(sim[s][c] == sim[s][cb] for s in selected))
            if same:
                continue
            if v == v:
                margin = min(margin, best - v)
        selected.append(cb)
        taken[bpos] = True
        m = int(masks[cb])
        for t in range(32):
            if (m >> t) & 1:
                counts[t] += 1
        info["round_two_picks"] += 1
    return selected, margin, info


def schedule(sim, scores, masks=None, *, max_candidates, similarity_threshold, dedup_on=True, quota=False, quotas=(),
             balance_factor=0.8):
    """stages 1-6 on one query -> (kept, selected, selected_sim, margin, info)"""
    sim = np.asarray(sim, dtype=np.float64)
    scores = [float(s) for s in scores]
    n = len(scores)
    masks = [0] * n if masks is None else [int(m) for m in masks]
    if dedup_on:
        kept, m1, replaced, dropped = dedup(sim, scores, similarity_threshold)
    else:
        kept, m1, replaced, dropped = list(range(n)), np.inf, 0, 0
    selected, m2, info = select(sim, scores, masks, kept, max_candidates, quota, list(quotas), balance_factor)
    info.update(replaced=replaced, dropped=dropped)
    ks = sim[np.ix_(selected, selected)] if selected else np.zeros((0, 0))
    return kept, selected, ks, min(m1, m2), info


def semantic_diversity(sel_sim):
    """SemanticDiversityEvaluator.evaluate_diversity (:173-194) on the selected candidates' similarities"""
    k = len(sel_sim)
    if k <= 1:
        return 1.0
    total, pairs = 0.0, 0
    for i in range(k):
        for j in range(i + 1, k):
            total += float(sel_sim[i][j])
            pairs += 1
    return max(0.0, min(1.0, 1.0 - total / pairs))


# ---- golden cases (tests/golden/diversity_cases.npz) ------------------------------------------------------------------
TYPE_NAMES = ["vector", "graph", "path_aware", "semantic", "entity_rich", "general"]   # bit order: the quota table's, then the rest
QUOTAS = [15, 10, 8, 12, 6, 0]
STRATEGIES = ["hybrid", "semantic", "topical"]
DEDUP_METHODS = ["hybrid", "semantic", "hash"]
CASE_ARRAYS = ("emb", "has_emb", "ids", "content", "scores", "path_score", "src_mask", "entities", "topics", "timestamp",
               "source")


def case_candidates(z, i):
    """the candidate dicts of golden case i, as the scheduler's callers pass them"""
    g = {k: z[f"c{i}_{k}"] for k in CASE_ARRAYS}
    out = []
    for j in range(len(g["ids"])):
        c = {"id": str(g["ids"][j]), "content": str(g["content"][j]), "score": float(g["scores"][j]),
             "path_score": float(g["path_score"][j]),
             "entities": [e for e in str(g["entities"][j]).split("|") if e],
             "topics": [t for t in str(g["topics"][j]).split("|") if t]}
        m = int(g["src_mask"][j])
        kinds = [n for b, n in enumerate(("vector", "graph")) if (m >> b) & 1]
        if m & 4 and len(kinds) == 1:
            c["source_info"] = {"source_type": kinds[0]}
        elif kinds:
            c["source_types"] = kinds
        if bool(g["has_emb"][j]):
            c["embedding"] = [float(x) for x in g["emb"][j]]
        if not np.isnan(g["timestamp"][j]):
            c["timestamp"] = float(g["timestamp"][j])
        if str(g["source"][j]):
            c["source"] = str(g["source"][j])
        out.append(c)
    return out


def case_config(z, i):
    """the scheduler config of golden case i and whether the plain form is switched on after construction"""
    cfg = {"diversity_scheduler": {"strategy": STRATEGIES[int(z["strategy"][i])], "max_candidates": int(z["max_candidates"][i]),
                                   "deduplication": {"method": DEDUP_METHODS[int(z["dedup_method"][i])],
                                                     "similarity_threshold": float(z["dedup_threshold"][i])}}}
    return cfg, not bool(z["quota"][i])


def infer_type_mask(cand):
    """CandidateItem's evidence-type inference (:119-141) as bits of TYPE_NAMES"""
    kinds = set(cand.get("source_types", []))
    st = cand.get("source_info", {}).get("source_type", "")
    if st:
        kinds.add(st)
    content = cand.get("content", "")
    density = len(cand.get("entities", [])) / max(len(content.split()), 1) if content else 0.0
    m = 0
    if "vector" in kinds:
        m |= 1
    if "graph" in kinds:
        m |= 2
    if cand.get("path_score", 0.0) > 0.3:
        m |= 4
    if cand.get("score", 0.0) > 0.7:
        m |= 8
    if density > 0.5:
        m |= 16
    return m or 32


def semantic_matrix(cands):
    """the per-pair semantic rule (:426-446): cosine where both carry an embedding, word Jaccard otherwise"""
    n = len(cands)
    has = [bool(c.get("embedding")) for c in cands]
    m = np.zeros((n, n))
    idx = [i for i in range(n) if has[i]]
    if idx:
        m[np.ix_(idx, idx)] = cosine_matrix([cands[i]["embedding"] for i in idx])
    for i in range(n):
        for j in range(n):
            if not (has[i] and has[j]):
                m[i, j] = word_jaccard(cands[i]["content"], cands[j]["content"])
    return m


def topical_matrix(cands):
    n = len(cands)
    return np.array([[set_jaccard(cands[i]["topics"], cands[j]["topics"]) for j in range(n)] for i in range(n)]).reshape(n, n)


def topical_diversity(topic_lists):
    """TopicalDiversityEvaluator.evaluate_diversity (:238-272)"""
    if len(topic_lists) <= 1:
        return 1.0
    counts = {}
    for ts in topic_lists:
        for t in ts:
            counts[t] = counts.get(t, 0) + 1
    if not counts:
        return 0.5
    total = sum(counts.values())
    entropy = 0.0
    for n in counts.values():
        p = n / total
        entropy -= p * np.log2(p)
    top = np.log2(len(counts))
    return max(0.0, min(1.0, entropy / top if top > 0 else 0.0))


def restate_case(cands, strategy, max_candidates, dedup_method, dedup_threshold, quota):
    """the whole schedule_candidates flow on candidate dicts -> dict(kept_ids, selected_ids, diversity_score, margin, info)"""
    items = list(cands)
    if dedup_method in ("hybrid", "hash"):
        import hashlib
        seen, first = set(), []
        for c in items:
            h = hashlib.md5(c["content"].encode()).hexdigest()[:12]
            if h not in seen:
                seen.add(h)
                first.append(c)
        items = first
    margin, info = np.inf, {"replaced": 0, "dropped": 0}
    if dedup_method in ("hybrid", "semantic"):
        kept, _, _, margin, info = schedule(semantic_matrix(items), [c["score"] for c in items], None,
                                            max_candidates=max(len(items), 1), similarity_threshold=dedup_threshold)
        items = [items[k] for k in kept]
    kept_ids = [c["id"] for c in items]
    sim = topical_matrix(items) if strategy == "topical" else semantic_matrix(items)
    masks = [infer_type_mask(c) for c in items]
    # the stable descending sort happens inside: positions are those of the kept list
    _, sel, _, m2, info2 = schedule(sim, [c["score"] for c in items], masks, max_candidates=max_candidates,
                                    similarity_threshold=2.0, dedup_on=False, quota=quota, quotas=QUOTAS, balance_factor=0.8)
    chosen = [items[s] for s in sel]
    sem = semantic_matrix(chosen)
    score = 0.0
    if chosen:
        score = (semantic_diversity(sem) + topical_diversity([c["topics"] for c in chosen])) / 2
    info2.update(replaced=info["replaced"], dropped=info["dropped"])
    return {"kept_ids": kept_ids, "selected_ids": [c["id"] for c in chosen], "diversity_score": score,
            "margin": min(margin, m2), "info": info2, "masks": masks}
