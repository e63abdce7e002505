"""Brute-force restatement, in Python sets and numpy, of the set-overlap join (csrc/setjoin.hip) and of the two relation
builders on top of it (anorag_hip/note_relations.py).  Quadratic on purpose: nothing here shares a line with the device
path or with its host wrapper.

  encode(rows)                     ids by first appearance, every row as a sorted list of distinct ids
  cooccur(rows_ids, min_common)    (I, J, inter, uni, common_ptr, common_items) sorted by (i, j)
  pair_counts(rows_ids, I, J)      (inter, uni)
  entity_coexistence(notes, threshold, weight)   relation_extractor.py:418-481 in canonical order
  topic(notes, weight)             relation_extractor.py:543-589 in the reference's order
  canonical(relations)             co-occurrence relations sorted by (source, target) position, shared entities sorted
"""
from collections import Counter

import numpy as np


def encode(rows):
    index, items, out = {}, [], []
    for row in rows:
        ids = set()
        for x in row:
            if x not in index:
                index[x] = len(items)
                items.append(x)
            ids.add(index[x])
        out.append(sorted(ids))
    return items, out


def to_csr(rows_ids):
    indptr = np.zeros(len(rows_ids) + 1, dtype=np.int64)
    for r, row in enumerate(rows_ids):
        indptr[r + 1] = indptr[r] + len(row)
    flat = [x for row in rows_ids for x in row]
    return indptr, np.asarray(flat, dtype=np.int32)


def cooccur(rows_ids, min_common):
    """all pairs through the dense incidence matrix A [n][n_items]: the overlaps are A A^T (small integers, exact in
    float32), the union of a pair is |S_i| + |S_j| less the overlap, the shared ids are the items of row i, ascending,
    whose bit is set in row j.  O(n * n_items) memory and O(n^2 * n_items) work: test shapes only."""
    n = len(rows_ids)
    n_items = max((max(r) for r in rows_ids if r), default=-1) + 1
    A = np.zeros((n, max(n_items, 1)), dtype=bool)
    for r, row in enumerate(rows_ids):
        A[r, row] = True
    Af = A.astype(np.float32)
    sizes = A.sum(axis=1).astype(np.int32)
    I, J, inter, uni, common = [], [], [], [], []
    for i0 in range(0, n, 512):
        C = (Af[i0:i0 + 512] @ Af.T).astype(np.int32)
        for i in range(i0, min(i0 + 512, n)):
            js = i + 1 + np.flatnonzero(C[i - i0, i + 1:] >= min_common)
            if not len(js):
                continue
            mine = np.asarray(rows_ids[i], dtype=np.int64)
            both = A[np.ix_(js, mine)]
            I.append(np.full(len(js), i, np.int32))
            J.append(js.astype(np.int32))
            inter.append(both.sum(axis=1).astype(np.int32))
            uni.append(sizes[i] + sizes[js] - inter[-1])
            common.append(mine[np.nonzero(both)[1]].astype(np.int32))  # row-major: pair by pair, ids ascending

    def cat(parts, dtype):
        return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    inter = cat(inter, np.int32)
    ptr = np.concatenate([[0], np.cumsum(inter, dtype=np.int64)]).astype(np.int64)
    return cat(I, np.int32), cat(J, np.int32), inter, cat(uni, np.int32), ptr, cat(common, np.int32)


def pair_counts(rows_ids, I, J):
    sets = [set(r) for r in rows_ids]
    inter = np.asarray([len(sets[i] & sets[j]) for i, j in zip(I, J)], dtype=np.int32)
    uni = np.asarray([len(sets[i] | sets[j]) for i, j in zip(I, J)], dtype=np.int32)
    return inter, uni


def entity_coexistence(notes, threshold=2, weight=0.8):
    """every pair of notes, earlier note first, that shares at least max(threshold, 1) entities; shared entities in order of
    first appearance over the notes"""
    first = {}
    for note in notes:
        for e in note.get('entities', []):
            first.setdefault(e, len(first))
    sets = [set(note.get('entities', [])) for note in notes]
    out = []
    for i in range(len(notes)):
        for j in range(i + 1, len(notes)):
            common = sets[i] & sets[j]
            if common and len(common) >= max(threshold, 1):
                out.append({
                    'source_id': notes[i].get('note_id'),
                    'target_id': notes[j].get('note_id'),
                    'relation_type': 'entity_coexistence',
                    'weight': weight * min(len(common) / 5.0, 1.0),
                    'metadata': {
                        'common_entities': sorted(common, key=first.__getitem__),
                        'entity_count': len(common),
                        'jaccard_similarity': len(common) / len(sets[i] | sets[j]),
                    },
                })
    return out


def canonical(relations, notes):
    """co-occurrence relations in the form the goldens store: sorted by the positions of (source, target) in the note list,
    shared entities sorted as strings"""
    pos = {note.get('note_id'): k for k, note in enumerate(notes)}
    out = []
    for r in sorted(relations, key=lambda r: (pos[r['source_id']], pos[r['target_id']])):
        r = dict(r)
        r['metadata'] = dict(r['metadata'])
        r['metadata']['common_entities'] = sorted(r['metadata']['common_entities'])
        out.append(r)
    return out


def _cohesion(notes):
    if len(notes) < 2:
        return 1.0
    words = [k for note in notes for k in note.get('keywords', [])]
    if not words:
        return 0.5
    counts = Counter(words)
    return min(sum(1 for c in counts.values() if c > 1) / len(counts), 1.0)


def _similarity(a, b):
    ka, kb = set(a.get('keywords', [])), set(b.get('keywords', []))
    if not ka and not kb:
        return 0.5
    if not ka or not kb:
        return 0.1
    ea, eb = set(a.get('entities', [])), set(b.get('entities', []))
    jac = len(ka & kb) / len(ka | kb)
    ent = len(ea & eb) / len(ea | eb) if (ea | eb) else 0.0
    return min(0.7 * jac + 0.3 * ent, 1.0)


def topic(notes, weight=0.7):
    groups = {}
    for note in notes:
        key = note.get('cluster_id')
        if key is None:
            key = note.get('topic', '')
        if key:
            groups.setdefault(key, []).append(note)
    out = []
    for key, members in groups.items():
        if len(members) < 2:
            continue
        cohesion = _cohesion(members)
        for i in range(len(members)):
            for j in range(i + 1, len(members)):
                sim = _similarity(members[i], members[j])
                out.append({
                    'source_id': members[i].get('note_id'),
                    'target_id': members[j].get('note_id'),
                    'relation_type': 'topic_relation',
                    'weight': weight * cohesion * sim,
                    'metadata': {'topic': str(key), 'topic_cohesion': cohesion, 'note_similarity': sim},
                })
    return out


def same_relations(got, want, ordered_keys=False):
    """equal as lists of dicts, with floats compared by their bits and types checked"""
    def norm(x):
        if isinstance(x, float):
            return ('f', np.float64(x).tobytes())
        if isinstance(x, dict):
            return [(k, norm(v)) for k, v in x.items()] if ordered_keys else {k: norm(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [norm(v) for v in x]
        return (type(x).__name__, x)
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert norm(g) == norm(w), (k, g, w)


# the goldens keep one short row per relation; make_relations_golden.py refuses a relation that does not survive the round trip
def pack_coexistence(relations, notes):
    pos = {note.get('note_id'): k for k, note in enumerate(notes)}
    return [[pos[r['source_id']], pos[r['target_id']], r['weight'], r['metadata']['common_entities'],
             r['metadata']['entity_count'], r['metadata']['jaccard_similarity']] for r in relations]


def pack_topic(relations, notes):
    pos = {note.get('note_id'): k for k, note in enumerate(notes)}
    return [[pos[r['source_id']], pos[r['target_id']], r['weight'], r['metadata']['topic'], r['metadata']['topic_cohesion'],
             r['metadata']['note_similarity']] for r in relations]


def expand_case(case):
    ids = [note.get('note_id') for note in case['notes']]
    case = dict(case)
    case['coexistence'] = [{'source_id': ids[s], 'target_id': ids[t], 'relation_type': 'entity_coexistence', 'weight': w,
                            'metadata': {'common_entities': common, 'entity_count': count, 'jaccard_similarity': jac}}
                           for s, t, w, common, count, jac in case['coexistence']]
    case['topic'] = [{'source_id': ids[s], 'target_id': ids[t], 'relation_type': 'topic_relation', 'weight': w,
                      'metadata': {'topic': topic, 'topic_cohesion': cohesion, 'note_similarity': sim}}
                     for s, t, w, topic, cohesion, sim in case['topic']]
    return case


def load_cases():
    """tests/golden/relation_cases.json: what the reference's own two methods returned (make_relations_golden.py)"""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relation_cases.json")) as f:
        return {c["name"]: expand_case(c) for c in json.load(f)["cases"]}
