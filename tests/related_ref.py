"""Brute-force restatement of the related-notes semantics (include/anorag.h, anr_index_related_notes) in
numpy and plain Python: the checker of tests/test_related_cpu.py and tests/test_related_gpu.py and of the golden generator
tests/golden/make_related_golden.py.  Nothing here imports the product.

  base(i, j)  math.fsum of the exact float64 products of the two stored float32 rows (the correctly rounded dot product)
  ent(i, j)   0.5 / 0.0 / min(inter / uni + (0.1 if inter >= min_shared else 0), 1.0)
  combined    base * (1 - w) + ent * w + cb, left to right in float64
  row i       the first M unskipped pairs with combined > threshold, by (combined descending, column ascending)
"""
import base64
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "related_notes_cases.json")
U = 2.0 ** -53

DEFAULTS = {"threshold": 0.75, "w": 0.3, "min_shared": 1, "exclude_same_cluster": True, "bonus": 0.1, "M": 5}


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def params_of_config(config):
    """the reference's config keys (utils/note_similarity.py:19-35) -> params"""
    return params(threshold=config.get("similarity_threshold", 0.75), w=config.get("entity_similarity_weight", 0.3),
                  min_shared=config.get("min_shared_entities", 1), exclude_same_cluster=config.get("exclude_same_cluster", True),
                  bonus=config.get("cluster_similarity_bonus", 0.1), M=config.get("max_related_notes", 5))


def stored_rows(emb):
    """what a normalising inner-product index stores (oracle/flat_index.py preprocess_vectors): float32 rows / float32 norms"""
    x = np.ascontiguousarray(emb, dtype=np.float32)
    norms = np.linalg.norm(x, axis=1, keepdims=True)
    return x / np.where(norms == 0, 1, norms)


_BASE_CACHE = {}


def base_matrix(x):
    """[n, n] float64: the correctly rounded dot product of every pair of float32 rows (kept per input: computed once and
    shared by the tests that need it; callers leave it unchanged)"""
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    key = (x32.shape, x32.tobytes())
    if key not in _BASE_CACHE:
        _BASE_CACHE[key] = _base_matrix(x32)
    return _BASE_CACHE[key]


def _base_matrix(x32):
    x64 = x32.astype(np.float64)
    n = len(x64)
    out = np.zeros((n, n))
    for i in range(n):
        prods = x64[i][None, :] * x64[i:]  # exact: 24-bit x 24-bit significands
        for k, row in enumerate(prods.tolist()):
            out[i, i + k] = out[i + k, i] = math.fsum(row)
    return out


def exact_cosine(emb):
    """[n, n] float64 cosine of the raw float32 embeddings: fsum dot products and norms, one rounding each"""
    g = base_matrix(emb)
    d = np.sqrt(np.diag(g))
    d = np.where(d == 0, 1, d)
    return g / d[:, None] / d[None, :]


def ent_counts(a, b):
    a, b = set(a), set(b)
    return len(a & b), len(a | b), len(a), len(b)


def ent_sim(inter, uni, la, lb, min_shared):
    if not la and not lb:
        return 0.5
    if not la or not lb:
        return 0.0
    j = inter / uni
    if inter >= min_shared:
        j += 0.1
    return min(j, 1.0)


def combine(base, ent, ci, cj, p):
    cb = 0
    if (not p["exclude_same_cluster"]) and ci != cj and base > p["threshold"] - 0.1:
        cb = p["bonus"]
    return base * (1 - p["w"]) + ent * p["w"] + cb


def all_pairs(base, entities, clusters, p):
    """per row i the list of its unskipped columns: (j, combined, base, ent, inter, uni), j ascending"""
    n = len(base)
    b = base.tolist()
    sets = [set(e) for e in entities]
    rows = []
    for i in range(n):
        row = []
        for j in range(n):
            if i == j:
                continue
            if p["exclude_same_cluster"] and clusters[j] == clusters[i] and clusters[i] != -1:
                continue
            inter, uni = len(sets[i] & sets[j]), len(sets[i] | sets[j])
            ent = ent_sim(inter, uni, len(sets[i]), len(sets[j]), p["min_shared"])
            row.append((j, combine(b[i][j], ent, clusters[i], clusters[j], p), b[i][j], ent, inter, uni))
        rows.append(row)
    return rows


def related(base, entities, clusters, p):
    """per row the first M kept entries of all_pairs, in result order"""
    out = []
    for row in all_pairs(base, entities, clusters, p):
        kept = [e for e in row if e[1] > p["threshold"]]
        kept.sort(key=lambda e: e[1], reverse=True)  # stable: ties stay in ascending column order
        out.append(kept[:p["M"]])
    return out


def round_margin(v):
    """distance of v to the nearest x.xxx5, where round(v, 3) changes"""
    f = math.fmod(abs(v) * 1000.0, 1.0)
    return abs(f - 0.5) / 1000.0


def margins(base, entities, clusters, p, allow_ties=False):
    """The smallest distances a computation of `base` would have to cross to decide differently:
      threshold  |combined - threshold| over all unskipped pairs
      order      gap between consecutive combined values among each row's first M + 1 kept (exact ties skipped only
                 with allow_ties: they are decided by the column on every side)
      bonus      |base - (threshold - 0.1)| over the pairs of different clusters, when the bonus rule is live
      rounding   distance of every reported value (similarity, base_similarity, entity_similarity) to the nearest x.xxx5
    inf where nothing applies."""
    m = {"threshold": math.inf, "order": math.inf, "bonus": math.inf, "rounding": math.inf}
    thr = p["threshold"]
    for i, row in enumerate(all_pairs(base, entities, clusters, p)):
        for (j, c, b, ent, inter, uni) in row:
            m["threshold"] = min(m["threshold"], abs(c - thr))
            if not p["exclude_same_cluster"] and clusters[i] != clusters[j]:
                m["bonus"] = min(m["bonus"], abs(b - (thr - 0.1)))
        kept = sorted((e for e in row if e[1] > thr), key=lambda e: e[1], reverse=True)[:p["M"] + 1]
        for a, b2 in zip(kept, kept[1:]):
            gap = a[1] - b2[1]
            if gap == 0 and allow_ties:
                continue
            m["order"] = min(m["order"], gap)
        for e in kept[:p["M"]]:
            m["rounding"] = min(m["rounding"], round_margin(e[1]), round_margin(e[2]), round_margin(e[3]))
    return m


# ---- the host rules of find_related_notes, restated (utils/note_similarity.py:115-167, :221-231, :261-280) ----

def note_id(note):
    return note.get('id', str(hash(note.get('content', ''))))


def prepare_text(note, use_content=True):
    texts = []
    if use_content and note.get('content'):
        content = note['content'].strip()
        if content:
            texts.append(content)
    if not texts and note.get('keywords'):
        kw = note['keywords']
        if isinstance(kw, list):
            texts.append(' '.join(kw))
        elif isinstance(kw, str):
            texts.append(kw)
    return ' '.join(texts) if texts else ''


def valid_positions(notes, config=None):
    use_content = (config or {}).get('use_content', True)
    return [k for k, note in enumerate(notes) if prepare_text(note, use_content)]


def find_related_notes(notes, emb_valid, config):
    """the reference's return value from the embeddings of the notes with text (one row each, in order)"""
    p = params_of_config(config)
    valid = valid_positions(notes, config)
    if len(valid) < 2:
        return notes
    vn = [notes[k] for k in valid]
    base = base_matrix(stored_rows(emb_valid))
    rel = related(base, [n.get('entities', []) for n in vn], [n.get('cluster_id', -1) for n in vn], p)
    pos = {k: r for r, k in enumerate(valid)}
    out = []
    for k, note in enumerate(notes):
        e = note.copy()
        e['related_notes'] = [{
            'id': note_id(vn[j]),
            'title': vn[j].get('content', '')[:50] + '...',
            'similarity': round(c, 3),
            'base_similarity': round(b, 3),
            'entity_similarity': round(ent, 3),
            'cluster_id': vn[j].get('cluster_id', -1),
        } for (j, c, b, ent, inter, uni) in rel[pos[k]]] if k in pos else []
        out.append(e)
    return out


def case_margins(case):
    """margins of a golden case, over its notes with text"""
    notes, config = case["notes"], case["config"]
    vn = [notes[k] for k in valid_positions(notes, config)]
    base = base_matrix(stored_rows(np.asarray(case["embeddings"], dtype=np.float32)))
    return margins(base, [n.get('entities', []) for n in vn], [n.get('cluster_id', -1) for n in vn], params_of_config(config))


def load_cases():
    """the golden cases, with `embeddings` decoded to float32 [valid notes, dim]"""
    with open(GOLDEN) as f:
        cases = json.load(f)["cases"]
    for c in cases:
        q = np.frombuffer(base64.b64decode(c["embeddings_i8"]), dtype=np.int8).reshape(-1, c["dim"])
        c["embeddings"] = q.astype(np.float32) / 16
        c["expected"] = expand_expected(c["related"], c["notes"])
    return cases


def pack_expected(expected, notes):
    """the reference's return value as rows [note position, related note's position, similarity, base_similarity,
    entity_similarity], each value as round(float(reference's), 3) — under NumPy 2 the reference rounds a float32, and that
    is the form the comparison uses (same_related); everything else in its output is a copy of the input (expand_expected)"""
    pos = {note_id(n): k for k, n in enumerate(notes)}
    return [[k, pos[r['id']]] + [round(float(r[v]), 3) for v in ('similarity', 'base_similarity', 'entity_similarity')]
            for k, e in enumerate(expected) for r in e['related_notes']]


def expand_expected(rows, notes):
    out = [dict(n, related_notes=[]) for n in notes]
    for k, j, sim, base, ent in rows:
        out[k]['related_notes'].append({
            'id': note_id(notes[j]), 'title': notes[j].get('content', '')[:50] + '...', 'similarity': sim,
            'base_similarity': base, 'entity_similarity': ent, 'cluster_id': notes[j].get('cluster_id', -1)})
    return out


def same_related(got, want):
    """ids, order, keys and cluster ids equal; each value equal after round(float(ref), 3)"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert list(g) == list(w), (list(g), list(w))
        assert {k: v for k, v in g.items() if k != 'related_notes'} == {k: v for k, v in w.items() if k != 'related_notes'}
        gr, wr = g['related_notes'], w['related_notes']
        assert [r['id'] for r in gr] == [r['id'] for r in wr], (g.get('id'), gr, wr)
        for a, b in zip(gr, wr):
            assert list(a) == list(b) == ['id', 'title', 'similarity', 'base_similarity', 'entity_similarity', 'cluster_id']
            assert a['title'] == b['title'] and a['cluster_id'] == b['cluster_id']
            assert type(a['cluster_id']) is type(b['cluster_id'])
            for k in ('similarity', 'base_similarity', 'entity_similarity'):
                assert a[k] == round(float(b[k]), 3), (g.get('id'), a['id'], k, a[k], b[k])


# ---- seeded synthetic inputs of the GPU tests ----

def clustered(n, d, seed, n_clusters=6, spread=0.25, n_entities=12, ent_per_row=(0, 4)):
    """(embeddings float32 [n, d], entities, cluster ids): rows around n_clusters centres, entity ids from a small pool (so
    unions stay below 16 and ent never sits on a rounding boundary), cluster ids -1 for every seventh row"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, d))
    lab = rng.integers(0, n_clusters, n)
    emb = (centres[lab] + spread * rng.standard_normal((n, d))).astype(np.float32)
    ents = [sorted(rng.choice(n_entities, rng.integers(ent_per_row[0], ent_per_row[1] + 1), replace=False).tolist()) for _ in range(n)]
    # cluster ids that do not follow the geometry, so that close pairs survive the same-cluster filter
    clusters = [int(c) if k % 7 else -1 for k, c in enumerate(rng.integers(0, 4, n))]
    return emb, ents, clusters
