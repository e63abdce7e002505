#!/usr/bin/env python3
"""Generate the related-notes golden vectors from the REFERENCE itself (run in the build container only).

  python tests/golden/make_related_golden.py /path/to/reference

Imports, by file path, the reference's utils/note_similarity.py with labelled stand-ins for loguru and
sentence_transformers (no arithmetic lives in them; the stand-in model's ``encode`` returns the case's recorded float32
embeddings) and the real sklearn ``cosine_similarity``, and runs its own ``find_related_notes`` on the inputs below.
Writes tests/golden/related_notes_cases.json — data only:

  cases[k] = {name, seed, config, notes, dim, embeddings_i8, related, base_dev, margins}
    embeddings_i8   int8 [valid notes][dim] in base64: the recorded float32 embeddings times 16 (the generator draws them
                    on that grid), one row per note WITH text, in note order
    related         the reference's return value as one short row per related note (tests/related_ref.py pack_expected);
                    values as round(float(v), 3), the form every comparison uses; the generator refuses a case that
                    expand_expected does not give back — keys, their order, ids, titles, cluster ids, rounded values
    base_dev        the largest |reference cosine - exact cosine| over the pairs of the case (tests/related_ref.py
                    exact_cosine): what the reference's float32 normalize + sgemm costs
    margins         tests/related_ref.py margins of the case

A case is REFUSED when one of its margins is below 1e-5 — two orders above float32 cosine rounding, so NumPy 1 and NumPy 2
scalar arithmetic, sklearn's float32 and a float64 dot product all decide, order and round alike.  A case's inputs come
from a seeded generator; the generator walks the seeds upward from the case's first seed until a draw is not refused and
records the seed it kept.  Each case ASSERTS the property it is there for.
"""
import base64
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import related_ref as rr  # noqa: E402

MIN_MARGIN = 1e-5


def load_reference(ref):
    m = types.ModuleType("loguru")

    class _L:
        def __getattr__(self, _):
            return lambda *a, **k: None

    m.logger = _L()
    sys.modules["loguru"] = m
    s = types.ModuleType("sentence_transformers")

    class SentenceTransformer:  # stand-in: never constructed, the generator installs the model object itself
        def __init__(self, *a, **k):
            raise RuntimeError("the golden generator supplies the embeddings")

    s.SentenceTransformer = SentenceTransformer
    sys.modules["sentence_transformers"] = s
    spec = importlib.util.spec_from_file_location("ref_note_similarity", os.path.join(ref, "utils", "note_similarity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class RecordedModel:
    """stand-in for the sentence transformer: returns the recorded embeddings of the texts it is asked for"""

    def __init__(self, emb):
        self.emb = emb

    def encode(self, texts, batch_size=32, show_progress_bar=False):
        assert len(texts) == len(self.emb)
        return self.emb


# name, first seed, n, d, sizes of the tight groups, config, extras
SPECS = [
    ("defaults", 100, 28, 40, [6, 3, 3, 2], {}, {}),
    ("bonus_fires", 200, 24, 8, [4, 3, 2], {"exclude_same_cluster": False, "similarity_threshold": 0.8}, {"tight": 0.3}),
    ("cluster_absent_minus1_none", 300, 24, 96, [4, 4, 3], {}, {"cluster_kinds": True}),
    ("empty_entities", 400, 24, 8, [5, 4, 3], {"similarity_threshold": 0.62}, {"ent_range": (0, 1)}),
    ("min_shared_0", 500, 24, 40, [4, 3, 3, 2], {"min_shared_entities": 0, "similarity_threshold": 0.65}, {}),
    ("min_shared_2", 600, 24, 40, [4, 3, 3, 2], {"min_shared_entities": 2}, {"ent_range": (1, 5)}),
    ("entity_weight_0", 700, 24, 40, [4, 3, 3, 2], {"entity_similarity_weight": 0}, {}),
    ("entity_weight_06", 800, 24, 40, [5, 3, 3], {"entity_similarity_weight": 0.6, "similarity_threshold": 0.6}, {}),
    ("note_without_text", 900, 24, 40, [4, 3, 3], {}, {"no_text": True}),
    ("more_than_m_related", 1000, 32, 8, [8, 3], {"max_related_notes": 5, "similarity_threshold": 0.7, "entity_similarity_weight": 0.1}, {"clusters_off": True}),
    ("max_related_1", 1100, 24, 8, [5, 4], {"max_related_notes": 1, "similarity_threshold": 0.8}, {"clusters_off": True, "tight": 0.1}),
]


def build(seed, n, d, groups, extras):
    """notes and the embeddings of those with text: tight groups (cosine ~0.9 inside) among unrelated background rows"""
    rng = np.random.default_rng(seed)
    tight = extras.get("tight", 0.15)
    emb = rng.standard_normal((n, d))
    member = {}
    at = 0
    order = rng.permutation(n)
    for g, size in enumerate(groups):
        centre = rng.standard_normal(d)
        for k in order[at:at + size]:
            emb[k] = centre + tight * rng.standard_normal(d)
            member[int(k)] = g
        at += size
    emb = (np.clip(np.round(emb * 16), -127, 127) / 16).astype(np.float32)   # on the grid the file stores: int8 sixteenths
    lo, hi = extras.get("ent_range", (0, 4))
    notes = []
    for k in range(n):
        g = member.get(k)
        pool = [f"g{g}e{t}" for t in range(6)] if g is not None else [f"b{t}" for t in range(9)]
        cnt = int(rng.integers(lo, hi + 1))
        ents = [pool[t] for t in rng.choice(len(pool), min(cnt, len(pool)), replace=False)]
        content = f"note {k}" + (f" of group {g}, a text long enough to be cut at fifty characters" if k % 8 == 0 else "")
        note = {"id": f"n{k:03d}", "content": content, "entities": ents}
        if k % 5 == 0 or extras.get("no_text"):
            note["keywords"] = [f"kw{k % 3}"]
        if extras.get("clusters_off"):
            pass  # no cluster_id key at all: everything is -1
        elif extras.get("cluster_kinds"):
            kind = k % 4
            if kind == 0:
                note["cluster_id"] = -1
            elif kind == 1:
                note["cluster_id"] = None
            elif kind == 2:
                note["cluster_id"] = int(rng.integers(0, 3))
        else:
            note["cluster_id"] = int(rng.integers(0, 4)) if k % 6 else -1
        if k % 9 == 4:
            del note["entities"]
        notes.append(note)
    if extras.get("no_text"):
        some = sorted(member)  # members of groups, so that a dropped note would have been somebody's neighbour
        notes[some[0]]["content"] = ""
        del notes[some[0]]["keywords"]                  # no text at all: not a candidate
        notes[some[1]]["content"] = "   "                # blank content, keywords stand in: stays a candidate
        notes[some[2]]["content"] = ""
        notes[some[2]]["keywords"] = "one keyword string"
        lone = next(k for k in range(n) if k not in member)  # a background note with neither key
        del notes[lone]["content"]
        del notes[lone]["keywords"]
    valid = rr.valid_positions(notes)
    return notes, np.ascontiguousarray(emb[valid])


def plain(x):
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    return x


def quick_margins(notes, emb, config):
    """margins with float64 matmul in place of fsum: the screen of the seed walk (the kept draw is checked exactly)"""
    vn = [notes[k] for k in rr.valid_positions(notes, config)]
    x = rr.stored_rows(emb).astype(np.float64)
    return rr.margins(x @ x.T, [n.get('entities', []) for n in vn], [n.get('cluster_id', -1) for n in vn],
                      rr.params_of_config(config))


def make_case(mod, name, seed0, n, d, groups, config, extras):
    for seed in range(seed0, seed0 + 400):
        notes, emb = build(seed, n, d, groups, extras)
        if min(quick_margins(notes, emb, config).values()) >= 2 * MIN_MARGIN:
            break
    else:
        raise SystemExit(f"refused: case {name}: no seed in [{seed0}, {seed0 + 400}) keeps every margin above {MIN_MARGIN}")
    case = {"name": name, "seed": seed, "config": config, "notes": notes, "dim": d,
            "embeddings": emb}
    m = rr.case_margins(case)
    if min(m.values()) < MIN_MARGIN:
        raise SystemExit(f"refused: case {name} seed {seed}: margins {m}")
    seen = {}
    real = mod.cosine_similarity

    def recording(a):
        seen["sim"] = real(a)
        return seen["sim"]

    mod.cosine_similarity = recording
    try:
        calc = mod.NoteSimilarityCalculator(dict(config))
        calc.model = RecordedModel(emb)
        expected = plain(calc.find_related_notes([dict(note) for note in notes]))
    finally:
        mod.cosine_similarity = real
    exact = rr.exact_cosine(emb)
    off = ~np.eye(len(emb), dtype=bool)
    case["base_dev"] = float(np.max(np.abs(seen["sim"].astype(np.float64) - exact)[off]))
    case["expected"] = expected
    case["related"] = rr.pack_expected(expected, notes)
    back = rr.expand_expected(json.loads(json.dumps(case["related"])), notes)
    try:
        rr.same_related(back, expected)
        assert [r['id'] for e in back for r in e['related_notes']] == [r['id'] for e in expected for r in e['related_notes']]
    except AssertionError:
        raise SystemExit(f"refused: case {name}: the packed rows do not give the reference's output back")
    case["margins"] = {k: (v if np.isfinite(v) else None) for k, v in m.items()}
    # the restatement must already agree: a disagreement here is a bug in one of the two, not a case to record
    rr.same_related(rr.find_related_notes(notes, emb, config), expected)
    return case


def check(cases):
    by = {c["name"]: c for c in cases}
    rel = {k: [r for note in c["expected"] for r in note["related_notes"]] for k, c in by.items()}
    assert all(len(v) > 0 for v in rel.values()), {k: len(v) for k, v in rel.items()}
    c = by["bonus_fires"]
    assert any(abs(r["similarity"] - (0.7 * r["base_similarity"] + 0.3 * r["entity_similarity"]) - 0.1) < 2e-3 for r in rel["bonus_fires"])
    kinds = {repr(n.get("cluster_id", "absent")) for n in by["cluster_absent_minus1_none"]["notes"]}
    assert {"'absent'", "-1", "None"} <= kinds and any(r["cluster_id"] is None for r in rel["cluster_absent_minus1_none"])
    ents = {r["entity_similarity"] for r in rel["empty_entities"]}
    assert 0.5 in ents and 0.0 in ents
    assert any(r["entity_similarity"] == 0.1 for r in rel["min_shared_0"])          # inter 0 >= 0: the bonus alone
    assert all(r["similarity"] == r["base_similarity"] for r in rel["entity_weight_0"])
    c = by["note_without_text"]
    assert len(rr.valid_positions(c["notes"])) == len(c["notes"]) - 2
    assert sum(1 for n in c["expected"] if not n["related_notes"] and not rr.prepare_text(n)) == 2
    c = by["more_than_m_related"]
    assert sum(1 for n in c["expected"] if len(n["related_notes"]) == 5) >= 8
    assert max(len(n["related_notes"]) for n in by["max_related_1"]["expected"]) == 1
    assert {c["dim"] for c in cases} == {8, 40, 96} and max(len(c["notes"]) for c in cases) == 32


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_related_golden.py /path/to/reference")
    mod = load_reference(sys.argv[1])
    cases = [make_case(mod, *spec) for spec in SPECS]
    check(cases)
    path = os.path.join(HERE, "related_notes_cases.json")
    with open(path, "w") as f:
        f.write('{"source": "reference utils/note_similarity.py NoteSimilarityCalculator.find_related_notes, embeddings '
                'supplied by a stand-in model, sklearn cosine_similarity",\n "min_margin": %r,\n "cases": [\n' % MIN_MARGIN)
        rows = []
        for c in cases:
            c = dict(c)
            emb = np.asarray(c.pop("embeddings"), dtype=np.float32)
            q = np.round(emb * 16).astype(np.int8)
            assert np.array_equal(q.astype(np.float32) / 16, emb)
            c["embeddings_i8"] = base64.b64encode(q.tobytes()).decode("ascii")
            del c["expected"]
            rows.append(json.dumps(c, separators=(",", ":")))
        f.write(",\n".join(rows))
        f.write("\n]}\n")
    for c in cases:
        n_rel = sum(len(n["related_notes"]) for n in c["expected"])
        print(f"{c['name']}: seed={c['seed']} notes={len(c['notes'])} d={c['dim']} related={n_rel} base_dev={c['base_dev']:.3g} "
              f"min_margin={min(v for v in c['margins'].values() if v is not None):.3g}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
