"""Numpy / pure-Python restatement of the TF-IDF join (csrc/tfidf.hip, anorag_hip.note_dedup), written apart from the
product code: the checker of tests/test_tfidf_cpu.py and tests/test_tfidf_gpu.py, and the thing
tests/golden/make_dedup_golden.py certifies against sklearn bit for bit before it records a case.

  normalize      sklearn's normalize(copy=True) of a CSR: squares added one at a time in stored order, sqrt, divide
  relabel        a term's label = its rank by (first row that holds it, position there); every row must then ascend
  pair_matrix    S[i, j] = (((0.0 + x_i0 * x_j0) + x_i1 * x_j1) + ...) over the labels ascending, float64, two roundings
                 a term: on a dense copy, where a term one of the two rows lacks adds +0.0 and leaves the bits alone
  duplicates     the pairs i < j with S[i, j] >= threshold in (i, j) order
  scores         per query and document, 0.0 + w_0 * m + w_1 * m + ... over the query's terms in the order given
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dedup_cases.npz")


def normalize(indptr, data):
    out = np.array(data, dtype=np.float64)
    for r in range(len(indptr) - 1):
        s = 0.0
        for k in range(indptr[r], indptr[r + 1]):
            v = float(out[k])
            s += v * v
        if s != 0.0:
            out[indptr[r]:indptr[r + 1]] /= np.sqrt(np.float64(s))
    return out


def relabel(indptr, indices, n_cols):
    """(terms int32 [nnz], label int32 [n_cols]); ValueError when a row does not ascend afterwards"""
    label = {}
    for k in range(len(indices)):   # CSR entries in (row, position) order: the first visit of a column is its key
        label.setdefault(int(indices[k]), len(label))
    for c in range(n_cols):
        label.setdefault(c, len(label))
    lab = np.array([label[c] for c in range(n_cols)], dtype=np.int32)
    terms = lab[np.asarray(indices, dtype=np.int64)] if len(indices) else np.zeros(0, np.int32)
    for r in range(len(indptr) - 1):
        row = terms[indptr[r]:indptr[r + 1]]
        if len(row) > 1 and np.any(np.diff(row.astype(np.int64)) <= 0):
            raise ValueError(f"row {r} does not ascend")
    return terms.astype(np.int32), lab


def dense(indptr, terms, values, n_terms):
    n = len(indptr) - 1
    d = np.zeros((n, n_terms), dtype=np.float64)
    for r in range(n):
        d[r, terms[indptr[r]:indptr[r + 1]]] = values[indptr[r]:indptr[r + 1]]
    return d


def pair_matrix(indptr, terms, values, n_terms):
    d = dense(indptr, terms, values, n_terms)
    n = len(indptr) - 1
    s = np.zeros((n, n), dtype=np.float64)
    held = np.count_nonzero(d, axis=0)
    for k in np.flatnonzero(held >= 2):     # ascending label; a label one row holds adds +0.0 off the diagonal
        col = d[:, k]
        s = s + np.multiply.outer(col, col)  # one rounded multiply, one rounded add
    return s


def duplicates(s, threshold):
    """(I int32, J int32, sim float64) of the pairs i < j with s[i, j] >= threshold, sorted by (i, j)"""
    keep = np.triu(s >= threshold, 1)
    I, J = np.nonzero(keep)   # row-major: sorted by (i, j)
    return I.astype(np.int32), J.astype(np.int32), s[I, J].astype(np.float64)


def scores(indptr, terms, values, n_terms, q_indptr, q_terms, q_weights):
    d = dense(indptr, terms, values, n_terms)
    nq = len(q_indptr) - 1
    out = np.zeros((nq, len(indptr) - 1), dtype=np.float64)
    for q in range(nq):
        acc = out[q]
        for k in range(q_indptr[q], q_indptr[q + 1]):
            col = d[:, q_terms[k]]
            upd = acc + q_weights[k] * col
            acc = np.where(col != 0.0, upd, acc)   # a document the posting does not hold is not touched
        out[q] = acc
    return out


def random_unit_rows(rng, lengths, n_terms):
    """(indptr int64, terms int32, values float64): rows of the given lengths over random ascending labels, each of unit
    length up to rounding (all values positive)"""
    indptr = np.zeros(len(lengths) + 1, dtype=np.int64)
    terms, values = [], []
    for r, ln in enumerate(lengths):
        t = np.sort(rng.choice(n_terms, size=ln, replace=False)).astype(np.int32)
        v = rng.random(ln) + 0.05
        if ln:
            v = v / np.sqrt(np.sum(v * v))
        terms.append(t)
        values.append(v)
        indptr[r + 1] = indptr[r] + ln
    cat = (lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt))
    return indptr, cat(terms, np.int32), cat(values, np.float64)


# ---- the reference's set loops, restated (utils/note_validator.py:395-440)
def jaccard_duplicates(notes, sets, threshold):
    out = []
    for i in range(len(sets)):
        for j in range(i + 1, len(sets)):
            a, b = sets[i], sets[j]
            if not a or not b:
                continue
            sim = len(a & b) / len(a | b)
            if sim >= threshold:
                out.append((notes[i].get('note_id', ''), notes[j].get('note_id', ''), sim))
    return out


def lexical_duplicates(notes, threshold=0.85):
    return jaccard_duplicates(notes, [set(n.get('content', '').lower().split()) for n in notes], threshold)


def entity_duplicates(notes, threshold=0.8):
    return jaccard_duplicates(notes, [set(n.get('entities', [])) for n in notes], threshold)


# ---- golden file
class Csr:
    """the recorded arrays of a scipy CSR, with the attributes anorag_hip.note_dedup reads (no scipy needed)"""
    format = "csr"

    def __init__(self, rec):
        self.shape = tuple(rec["shape"])
        self.indptr = np.asarray(rec["indptr"], dtype=np.int64)
        self.indices = np.asarray(rec["indices"], dtype=np.int32)
        self.data = np.asarray(rec["data"], dtype=np.float64)


def save_file(obj):
    """the golden file: every numpy array of obj as a member of the .npz, the rest as JSON text in the member `json`"""
    arrays = {}

    def strip(x):
        if isinstance(x, np.ndarray):
            arrays[f"a{len(arrays)}"] = x
            return {"__npz__": f"a{len(arrays) - 1}"}
        if isinstance(x, dict):
            return {k: strip(v) for k, v in x.items()}
        return [strip(v) for v in x] if isinstance(x, (list, tuple)) else x

    text = json.dumps(strip(obj), separators=(",", ":"))
    np.savez_compressed(GOLDEN, json=np.frombuffer(text.encode(), dtype=np.uint8), **arrays)


def load_file():
    with np.load(GOLDEN) as z:
        def fill(x):
            if isinstance(x, dict):
                return z[x["__npz__"]] if "__npz__" in x else {k: fill(v) for k, v in x.items()}
            return [fill(v) for v in x] if isinstance(x, list) else x
        return fill(json.loads(z["json"].tobytes().decode()))


def load_cases():
    return load_file()["cases"]


def pack_kept(kept, notes):
    """deduplicated_notes as rows [position of the note in notes, its duplicates_removed sorted, or None]"""
    at = {n.get('note_id', ''): k for k, n in enumerate(notes)}
    assert len(at) == len(notes)
    return [[at[n.get('note_id', '')], sorted(n['duplicates_removed']) if 'duplicates_removed' in n else None] for n in kept]


def expand_kept(rows, notes):
    out = []
    for k, removed in rows:
        note = dict(notes[k])
        if removed is not None:
            note['duplicates_removed'] = removed
        out.append(note)
    return out


def load_expected(case):
    """the recorded dict of a case with deduplicated_notes expanded"""
    want = dict(case["expected"])
    want["deduplicated_notes"] = expand_kept(want["deduplicated_notes"], case["notes"])
    return want


def semantic_from_csr(case, threshold=0.85):
    """the restatement's semantic duplicates of a recorded case: [(id_i, id_j, value)] in (i, j) order"""
    m = Csr(case["csr"])
    vals = normalize(m.indptr, m.data)
    terms, _ = relabel(m.indptr, m.indices, m.shape[1])
    I, J, sim = duplicates(pair_matrix(m.indptr, terms, vals, m.shape[1]), threshold)
    ids = [n.get('note_id', '') for n in case["notes"]]
    return [(ids[i], ids[j], float(v)) for i, j, v in zip(I.tolist(), J.tolist(), sim)]


def tuples(rows):
    return [(a, b, float(v)) for a, b, v in rows]


def same_result(got, want):
    """a detect_duplicate_notes dict against the recorded one: everything equal, floats by value (== on Python floats is
    bit equality away from zero), duplicates_removed as a set (the reference builds it with list(set))"""
    assert list(got.keys()) == list(want.keys()), (list(got.keys()), list(want.keys()))
    assert got["status"] == want["status"]
    assert got["exact_duplicates"] == want["exact_duplicates"]
    assert list(got["exact_duplicates"].keys()) == list(want["exact_duplicates"].keys())
    for key in ("semantic_duplicates", "entity_duplicates"):
        assert tuples(got[key]) == tuples(want[key]), key
    assert got["duplicate_rate"] == want["duplicate_rate"]
    assert got["removed_count"] == want["removed_count"] and got["remaining_count"] == want["remaining_count"]
    a, b = got["deduplicated_notes"], want["deduplicated_notes"]
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = dict(x), dict(y)
        assert set(x.pop("duplicates_removed", [])) == set(y.pop("duplicates_removed", []))
        assert x == y
