#!/usr/bin/env python3
"""Generate the duplicate-detection golden vectors from the REFERENCE itself (run in the build container only).

  python tests/golden/make_dedup_golden.py /path/to/reference

Imports, by file path, the reference's utils/note_validator.py with a labelled stand-in for loguru (no arithmetic lives in
it) and the real sklearn, and runs its own ``NoteValidator.detect_duplicate_notes``, ``_find_lexical_duplicates`` and
``_find_entity_duplicates``.  Writes tests/golden/dedup_cases.npz (tests/tfidf_ref.py save_file) — data only:

  cases[k] = {name, seed, notes, csr, expected, lexical, entity}
    csr        the matrix ``fit_transform`` returned inside the reference's call, exactly as stored (indices IN STORED
               ORDER); null when the vectoriser was not reached (< 2 notes) or raised (empty vocabulary)
    expected   the reference's dict; ``deduplicated_notes`` as one short row per surviving note (tfidf_ref.pack_kept),
               ``duplicates_removed`` sorted (the reference builds it with list(set))
    lexical    {threshold: the reference's _find_lexical_duplicates}, entity likewise, at 0.85 / 0.8 and at 0.5
  retriever = {notes, queries, top_k, csr, query_csr, sims}: the matrix of VectorRetriever._build_bm25_index
               (vector_store/retriever.py:924-964), the transformed queries and sklearn's cosine_similarity(q, M)

A case is REFUSED when the restatement (tests/tfidf_ref.py) is not bit-equal to sklearn's ``cosine_similarity`` on every
pair i != j (the order argument of DESIGN.md §5o would be broken: stop and find out why); when the product's host half
(note_dedup.normalize_rows, relabel_terms) differs from the restatement's; when a pair lies within 1e-9 of the 0.85
threshold (the seeds are then walked upward, the kept seed recorded); (retriever) when two positive scores inside the top_k
window or at its edge are equal.  Each case ASSERTS the property it is there for.
"""
import copy
import importlib.util
import json
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "ano-rag_amd"))
import tfidf_ref as tr  # noqa: E402

MARGIN = 1e-9
THRESHOLD = 0.85
STOP = ["the", "and", "of", "to", "is", "in", "that", "it"]


def load_reference(ref):
    m = types.ModuleType("loguru")

    class _L:
        def __getattr__(self, _):
            return lambda *a, **k: None

    m.logger = _L()
    sys.modules["loguru"] = m
    spec = importlib.util.spec_from_file_location("ref_note_validator", os.path.join(ref, "utils", "note_validator.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def words(rng, vocab, n, zipf=1.3):
    ranks = np.minimum(rng.zipf(zipf, size=n), vocab) - 1
    return [f"w{int(r):04d}" for r in ranks]


def sprinkle(rng, ws):
    out = []
    for w in ws:
        out.append(w)
        if rng.random() < 0.3:
            out.append(STOP[int(rng.integers(len(STOP)))])
    return out


def build(seed, n, vocab, groups, extras):
    """n notes of Zipf-distributed words; ``groups`` lists the sizes of near-duplicate groups (a member is a copy of the
    group's first note with a few words changed)"""
    rng = np.random.default_rng(seed)
    lo, hi = extras.get("len", (12, 40))
    texts = [sprinkle(rng, words(rng, vocab, int(rng.integers(lo, hi + 1)))) for _ in range(n)]
    order = rng.permutation(n)
    at = 0
    member = {}
    for g, size in enumerate(groups):
        ks = [int(k) for k in order[at:at + size]]
        at += size
        for k in ks[1:]:
            t = list(texts[ks[0]])
            for _ in range(int(rng.integers(0, extras.get("edits", 3)))):
                t[int(rng.integers(len(t)))] = words(rng, vocab, 1)[0]
            texts[k] = t
        for k in ks:
            member[k] = g
    for k in extras.get("exact", []):          # exact copies of an earlier note's content
        texts[order[k]] = list(texts[order[0]])
    notes = []
    for k in range(n):
        g = member.get(k)
        pool = [f"g{g}e{t}" for t in range(5)] if g is not None else [f"b{t}" for t in range(extras.get("bg_entities", 40))]
        cnt = int(rng.integers(*extras.get("ent", (1, 5))))
        if g is not None:   # a group's members hold a prefix of the group's pool: equal, or nested sets
            ents = pool[:cnt]
        else:
            ents = [pool[t] for t in rng.choice(len(pool), min(cnt, len(pool)), replace=False)]
        if extras.get("repeats") and ents:
            ents = ents + [ents[0]] * int(rng.integers(1, 3))
        note = {"note_id": f"n{k:04d}", "content": " ".join(texts[k]), "entities": ents}
        if extras.get("no_entities") and k % 7 == 0:
            del note["entities"]
        if extras.get("no_entities") and k % 7 == 1:
            note["entities"] = []
        notes.append(note)
    for k, content in extras.get("contents", {}).items():
        notes[k]["content"] = content
    for k in extras.get("no_content", []):
        del notes[k]["content"]
    return notes


# name, first seed, n, vocab, near-duplicate groups, extras
SPECS = [
    ("vocab_below_max_features", 100, 60, 300, [3, 2, 2], {}),
    ("vocab_above_max_features", 200, 300, 4000, [4, 3, 3, 2, 2, 2], {"len": (20, 60), "bg_entities": 400}),
    ("exact_duplicate_contents", 300, 40, 200, [2], {"exact": [5, 9, 13]}),
    ("empty_and_stop_word_notes", 400, 30, 150, [3, 2], {"contents": {2: "", 5: "the and of", 7: "is it in the", 11: "   "},
                                                         "no_content": [13]}),
    ("one_note", 500, 1, 50, [], {}),
    ("no_notes", 550, 0, 50, [], {}),
    ("empty_vocabulary_lexical_fallback", 600, 6, 50, [], {"contents": {0: "the and of", 1: "of the and", 2: "is it",
                                                                        3: "", 4: "it is", 5: "the and of to is in that"}}),
    ("notes_without_entities", 700, 45, 250, [5, 4], {"no_entities": True}),
    ("entity_lists_with_repeats", 800, 45, 250, [4, 2], {"repeats": True, "ent": (2, 5)}),
    ("status_passed", 900, 60, 2000, [2], {"bg_entities": 400, "ent": (3, 6)}),
    ("status_failed", 1000, 30, 200, [6, 5, 4, 3], {"edits": 2}),
]


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, set):
        return sorted(plain(v) for v in x)
    if isinstance(x, np.generic):
        return x.item()
    return x


def record_csr(m):
    assert m.format == "csr" and m.data.dtype == np.float64
    return {"shape": [int(m.shape[0]), int(m.shape[1])], "indptr": m.indptr.astype(np.int32),
            "indices": m.indices.astype(np.int32), "data": m.data.copy()}


def certify_restatement(name, m, sim):
    """refuse unless the restatement and the product's host half reproduce sklearn's matrix bit for bit"""
    from anorag_hip import note_dedup as nd
    from sklearn.preprocessing import normalize
    rec = tr.Csr(record_csr(m))
    vals = tr.normalize(rec.indptr, rec.data)
    if vals.tobytes() != normalize(m, copy=True).data.tobytes():
        raise SystemExit(f"refused: case {name}: the restated normalize is not sklearn's")
    if nd.normalize_rows(rec.indptr, rec.data).tobytes() != vals.tobytes():
        raise SystemExit(f"refused: case {name}: anorag_hip.note_dedup.normalize_rows is not sklearn's")
    terms, lab = tr.relabel(rec.indptr, rec.indices, rec.shape[1])
    pt, pl = nd.relabel_terms(rec)
    if not (np.array_equal(pt, terms) and np.array_equal(pl, lab)):
        raise SystemExit(f"refused: case {name}: anorag_hip.note_dedup.relabel_terms differs from the restatement")
    s = tr.pair_matrix(rec.indptr, terms, vals, rec.shape[1])
    off = ~np.eye(m.shape[0], dtype=bool)
    if not np.array_equal(s[off].view(np.uint64), np.asarray(sim, dtype=np.float64)[off].view(np.uint64)):
        bad = int(np.count_nonzero(s[off] != sim[off]))
        raise SystemExit(f"refused: case {name}: the restatement differs from cosine_similarity on {bad} pairs")
    if not np.array_equal(sim, sim.T):
        raise SystemExit(f"refused: case {name}: cosine_similarity is not bitwise symmetric")
    return s


def run_case(mod, name, seed, n, vocab, groups, extras):
    notes = build(seed, n, vocab, groups, extras)
    seen = {}
    real_fit = mod.TfidfVectorizer.fit_transform
    real_cos = mod.cosine_similarity

    def fit(self, raw):
        seen["csr"] = real_fit(self, raw)
        return seen["csr"]

    def cos(a):
        seen["sim"] = real_cos(a)
        return seen["sim"]

    mod.TfidfVectorizer.fit_transform = fit
    mod.cosine_similarity = cos
    try:
        v = object.__new__(mod.NoteValidator)   # the duplicate methods read no attribute of the instance
        expected = v.detect_duplicate_notes(copy.deepcopy(notes))
        lexical = {repr(t): v._find_lexical_duplicates(copy.deepcopy(notes), t) for t in (0.85, 0.5)}
        entity = {repr(t): v._find_entity_duplicates(copy.deepcopy(notes), t) for t in (0.8, 0.5)}
    finally:
        mod.TfidfVectorizer.fit_transform = real_fit
        mod.cosine_similarity = real_cos
    assert expected["status"] != "error", expected
    case = {"name": name, "seed": seed, "notes": notes, "csr": None}
    if "sim" in seen:
        sim = seen["sim"]
        iu = np.triu_indices(sim.shape[0], 1)
        if len(iu[0]) and np.min(np.abs(sim[iu] - THRESHOLD)) < MARGIN:
            return None   # a margin: the next seed
        certify_restatement(name, seen["csr"], sim)
        case["csr"] = record_csr(seen["csr"])
        case["max_off_diagonal"] = float(np.max(sim[iu])) if len(iu[0]) else None
    case["expected"] = plain(expected)
    # the surviving notes as rows [position in notes, duplicates_removed or null]: the reference changes nothing else
    full = case["expected"]["deduplicated_notes"]
    for n in full:
        if "duplicates_removed" in n:
            n["duplicates_removed"] = sorted(n["duplicates_removed"])
    case["expected"]["deduplicated_notes"] = tr.pack_kept(full, notes)
    if tr.expand_kept(json.loads(json.dumps(case["expected"]["deduplicated_notes"])), notes) != full:
        raise SystemExit(f"refused: case {name}: the packed rows do not give the reference's deduplicated_notes back")
    case["lexical"] = plain(lexical)
    case["entity"] = plain(entity)
    return case


def make_retriever_case(seed0):
    from sklearn.feature_extraction.text import TfidfVectorizer
    from sklearn.metrics.pairwise import cosine_similarity

    def pre(text):   # VectorRetriever._preprocess_text (retriever.py:958-964)
        text = re.sub(r"[^a-zA-Z0-9\s]", " ", text)
        return re.sub(r"\s+", " ", text).strip().lower()

    top_k = 10
    for seed in range(seed0, seed0 + 200):
        rng = np.random.default_rng(seed)
        notes = [{"note_id": f"r{k:03d}", "content": " ".join(sprinkle(rng, words(rng, 120, int(rng.integers(8, 30)))))
                  + ("." if k % 2 else "")} for k in range(90)]
        notes[7]["content"] = ""
        queries = [" ".join(words(rng, 120, int(rng.integers(2, 7)))) for _ in range(4)] + ["zzz unknown words only"]
        vec = TfidfVectorizer(lowercase=True, stop_words="english", max_features=10000, ngram_range=(1, 2))
        m = vec.fit_transform([pre(n["content"]) if n["content"] else "" for n in notes])
        q = vec.transform([pre(t) for t in queries])
        sims = cosine_similarity(q, m)
        ok = True
        for row in sims:
            top = np.sort(row[row > 0])[::-1][:top_k + 1]
            ok = ok and len(np.unique(top)) == len(top)
        if not ok:
            continue
        assert np.count_nonzero(sims[-1]) == 0 and all(np.count_nonzero(r) > top_k for r in sims[:-1])
        # the restatement of the search: per document the query's terms in ascending column id, from 0.0
        from anorag_hip import note_dedup as nd
        mrec, qrec = tr.Csr(record_csr(m)), tr.Csr(record_csr(q))
        terms, lab = tr.relabel(mrec.indptr, mrec.indices, mrec.shape[1])
        got = tr.scores(mrec.indptr, terms, tr.normalize(mrec.indptr, mrec.data), mrec.shape[1], qrec.indptr,
                        lab[qrec.indices], tr.normalize(qrec.indptr, qrec.data))
        if got.tobytes() != np.ascontiguousarray(sims, dtype=np.float64).tobytes():
            raise SystemExit("refused: retriever case: the restated scores are not cosine_similarity(q, M)")
        assert np.array_equal(nd.relabel_terms(mrec)[1], lab)
        return {"seed": seed, "notes": notes, "queries": queries, "top_k": top_k, "csr": record_csr(m),
                "query_csr": record_csr(q), "sims": np.ascontiguousarray(sims, dtype=np.float64)}
    raise SystemExit("refused: retriever case: no seed without a tie among the positive scores")


def check(cases):
    by = {c["name"]: c for c in cases}
    sem = {k: c["expected"]["semantic_duplicates"] for k, c in by.items()}
    assert by["vocab_below_max_features"]["csr"]["shape"][1] < 1000 and sem["vocab_below_max_features"]
    assert by["vocab_above_max_features"]["csr"]["shape"] == [300, 1000] and sem["vocab_above_max_features"]
    assert len(by["exact_duplicate_contents"]["expected"]["exact_duplicates"]) == 1
    assert len(next(iter(by["exact_duplicate_contents"]["expected"]["exact_duplicates"].values()))) == 4
    m = tr.Csr(by["empty_and_stop_word_notes"]["csr"])
    assert np.count_nonzero(np.diff(m.indptr) == 0) >= 5 and sem["empty_and_stop_word_notes"]
    assert by["one_note"]["csr"] is None and by["no_notes"]["csr"] is None
    assert by["no_notes"]["expected"]["duplicate_rate"] == 0.0
    c = by["empty_vocabulary_lexical_fallback"]
    assert c["csr"] is None and c["expected"]["semantic_duplicates"] == c["lexical"]["0.85"] and len(c["lexical"]["0.85"]) >= 2
    c = by["notes_without_entities"]
    assert any("entities" not in n for n in c["notes"]) and any(n.get("entities") == [] for n in c["notes"])
    assert c["expected"]["entity_duplicates"]
    c = by["entity_lists_with_repeats"]
    assert any(len(set(n["entities"])) < len(n["entities"]) for n in c["notes"]) and c["expected"]["entity_duplicates"]
    assert {"passed", "warning", "failed"} <= {c["expected"]["status"] for c in cases}
    assert by["status_passed"]["expected"]["status"] == "passed" and by["status_failed"]["expected"]["status"] == "failed"
    assert any(c["entity"]["0.5"] != c["entity"]["0.8"] for c in cases) and any(c["lexical"]["0.5"] for c in cases)


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_dedup_golden.py /path/to/reference")
    mod = load_reference(sys.argv[1])
    cases = []
    for name, seed0, n, vocab, groups, extras in SPECS:
        for seed in range(seed0, seed0 + 50):
            case = run_case(mod, name, seed, n, vocab, groups, extras)
            if case is not None:
                break
        else:
            raise SystemExit(f"refused: case {name}: no seed in [{seed0}, {seed0 + 50}) keeps every pair {MARGIN} away from {THRESHOLD}")
        cases.append(case)
    check(cases)
    retriever = make_retriever_case(2000)
    tr.save_file({"source": "reference utils/note_validator.py NoteValidator.detect_duplicate_notes, _find_lexical_duplicates, "
                            "_find_entity_duplicates with the real sklearn; retriever: sklearn on the matrix of "
                            "vector_store/retriever.py _build_bm25_index", "margin": MARGIN, "cases": cases, "retriever": retriever})
    for c in cases:
        e = c["expected"]
        print(c["name"], c["seed"], len(c["notes"]), c["csr"]["shape"] if c["csr"] else None, e["status"],
              len(e["exact_duplicates"]), len(e["semantic_duplicates"]), len(e["entity_duplicates"]), c.get("max_off_diagonal"))
    print(tr.GOLDEN, os.path.getsize(tr.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
