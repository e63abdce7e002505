#!/usr/bin/env python3
"""Generate the note-relation golden vectors from the REFERENCE itself (run in the build container only).

  python tests/golden/make_relations_golden.py /path/to/reference

Imports, by file path, the reference's graph/relation_extractor.py with the stand-ins make_golden.py uses (loguru, utils,
config: no arithmetic lives in them) and runs its own extract_entity_coexistence_relations and extract_topic_relations on
the recorded inputs below.  Writes tests/golden/relation_cases.json — data only:

  cases[k] = {name, threshold, notes, coexistence, topic}
    coexistence   the reference's relations in CANONICAL form: sorted by the positions of (source, target) in the note
                  list, common_entities sorted (the reference's own order of both follows Python's string hashing)
    topic         the reference's list as it returned it (its order is deterministic)
  Both lists are stored as one short row per relation (tests/setjoin_ref.py: pack_coexistence / pack_topic); the generator
  refuses a relation that expand_case does not give back exactly — keys, their order, nesting, types, floats by their bits.

A case is refused when the reference's source_id is not the earlier note of a pair, and when a second run in a fresh child
process with another PYTHONHASHSEED gives a different canonical form or another topic list.  Each case ASSERTS the property
it is there for.
"""
import importlib.util
import json
import os
import random
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import setjoin_ref  # noqa: E402  (the row form of the stored relations)


def load_reference(ref):
    m = types.ModuleType("loguru")

    class _L:
        def __getattr__(self, _):
            return lambda *a, **k: None

    m.logger = _L()
    sys.modules["loguru"] = m
    u = types.ModuleType("utils")

    class _Any:
        def __init__(self, *a, **k):
            pass

    u.TextUtils = u.GPUUtils = u.BatchProcessor = _Any
    sys.modules["utils"] = u
    c = types.ModuleType("config")

    class _Cfg:
        def get(self, key, default=None):
            return default

    c.config = _Cfg()
    sys.modules["config"] = c
    spec = importlib.util.spec_from_file_location("ref_relation_extractor", os.path.join(ref, "graph", "relation_extractor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_notes(rng, n, vocab_of, n_ent, keywords_of=None, prefix="n"):
    notes = []
    for i in range(n):
        vocab = vocab_of(i)
        k = min(rng.randint(*n_ent), len(vocab))
        note = {"note_id": f"{prefix}{i:04d}", "entities": rng.sample(vocab, k)}
        if keywords_of is not None:
            note["keywords"] = keywords_of(i)
        notes.append(note)
    return notes


def inputs():
    """(name, threshold, notes) — built from a seeded generator only, never from the iteration order of a set"""
    rng = random.Random(20261018)
    out = []

    # four entity vocabularies, a note draws from one: overlaps inside a cluster, none across
    vocabs = [[f"ent{c}_{k}" for k in range(14)] for c in range(4)]
    words = [f"kw{k}" for k in range(30)]
    notes = make_notes(rng, 60, lambda i: vocabs[i % 4], (2, 6), lambda i: rng.sample(words, rng.randint(1, 5)))
    for i, note in enumerate(notes):
        note["cluster_id"] = 1 + (i * 7) % 9
    out.append(("clustered", 2, notes))

    # notes without entities: an empty list, and the key missing altogether
    pool = [f"e{k}" for k in range(25)]
    notes = make_notes(rng, 40, lambda i: pool, (0, 4))
    for i in range(0, 40, 11):
        del notes[i]["entities"]
    out.append(("no_entities", 1, notes))

    # an entity repeated inside a note counts once
    notes = make_notes(rng, 30, lambda i: pool[:12], (2, 5))
    for note in notes[::3]:
        note["entities"] = note["entities"] + note["entities"][:2] + note["entities"][:1]
    out.append(("duplicates", 2, notes))

    # one entity shared by every note: every pair is a candidate
    notes = make_notes(rng, 14, lambda i: pool, (1, 3))
    for note in notes:
        note["entities"].insert(rng.randint(0, len(note["entities"])), "everywhere")
    out.append(("shared_by_all_t1", 1, notes))
    out.append(("shared_by_all_t2", 2, [dict(n) for n in notes]))

    dense = [f"d{k}" for k in range(16)]
    notes = make_notes(rng, 24, lambda i: dense, (3, 8))
    out.append(("dense_t3", 3, notes))
    out.append(("dense_t1_small", 1, [dict(n) for n in notes[:16]]))

    # a threshold above every overlap, and the threshold 0 the reference lifts to 1
    notes = make_notes(rng, 30, lambda i: pool, (1, 3))
    out.append(("nothing_kept", 9, notes))
    out.append(("threshold_zero", 0, [dict(n) for n in notes[:20]]))

    # the grouping rule: cluster_id 0 is dropped, None falls back to the topic, an empty topic is dropped, a group of one
    # gives nothing; keywords empty on one side, on both, missing; repeated keywords inside a note
    notes = make_notes(rng, 64, lambda i: pool, (0, 4))
    topics = ["alpha", "", "beta", "gamma"]
    for i, note in enumerate(notes):
        sel = i % 8
        if sel in (0, 1):
            note["cluster_id"] = 0
        elif sel in (2, 3):
            note["cluster_id"] = None
            note["topic"] = topics[(i // 8) % 4]
        elif sel == 4:
            note["topic"] = topics[(i // 8 + 1) % 4]       # no cluster_id key at all
        else:
            note["cluster_id"] = 1 + (i // 8) % 3
        kind = (i * 5) % 7
        if kind == 0:
            note["keywords"] = []
        elif kind == 1:
            pass                                            # key missing
        elif kind == 2:
            note["keywords"] = ["kw1", "kw1", "kw2"]
        else:
            note["keywords"] = rng.sample(words[:8], rng.randint(1, 4))
    notes.append({"note_id": "lonely", "cluster_id": 77, "keywords": ["kw1"], "entities": ["e1"]})
    notes.append({"note_id": "silent-a", "cluster_id": 78, "entities": ["e1", "e2"]})
    notes.append({"note_id": "silent-b", "cluster_id": 78, "keywords": [], "entities": ["e2"]})
    out.append(("grouping", 2, notes))
    return out


def canonical(relations, notes):
    pos = {note["note_id"]: k for k, note in enumerate(notes)}
    for r in relations:
        if pos[r["source_id"]] >= pos[r["target_id"]]:
            raise SystemExit(f"refused: source {r['source_id']} is not the earlier note of its pair")
    out = []
    for r in sorted(relations, key=lambda r: (pos[r["source_id"]], pos[r["target_id"]])):
        md = dict(r["metadata"])
        md["common_entities"] = sorted(md["common_entities"])
        out.append({**r, "metadata": md})
    return out


def run(ref):
    rx = load_reference(ref)
    cases = []
    for name, threshold, notes in inputs():
        ext = rx.RelationExtractor()
        ext.entity_cooccurrence_threshold = threshold
        co = canonical(ext.extract_entity_coexistence_relations(notes), notes)
        tp = ext.extract_topic_relations(notes)
        cases.append({"name": name, "threshold": threshold, "notes": notes, "coexistence": co, "topic": tp})
    return cases


def check(cases):
    by = {c["name"]: c for c in cases}
    n = {k: len(c["coexistence"]) for k, c in by.items()}
    assert n["clustered"] > 40 and all("_" in e for r in by["clustered"]["coexistence"] for e in r["metadata"]["common_entities"])
    assert any(not note.get("entities") for note in by["no_entities"]["notes"]) and n["no_entities"] > 0
    assert n["shared_by_all_t1"] == 14 * 13 // 2 and 0 < n["shared_by_all_t2"] < n["shared_by_all_t1"]
    assert n["dense_t3"] > 0 and min(r["metadata"]["entity_count"] for r in by["dense_t3"]["coexistence"]) == 3
    assert n["nothing_kept"] == 0 and n["threshold_zero"] > 0
    assert min(r["metadata"]["entity_count"] for r in by["threshold_zero"]["coexistence"]) == 1
    assert any(r["metadata"]["entity_count"] > 5 for r in by["dense_t3"]["coexistence"])  # the weight's min(., 1.0)
    g = by["grouping"]["topic"]
    topics = {r["metadata"]["topic"] for r in g}
    assert "0" not in topics and "" not in topics and "77" not in topics and {"alpha", "beta", "gamma", "1", "78"} <= topics
    sims = {r["metadata"]["note_similarity"] for r in g}
    assert 0.5 in sims and 0.1 in sims and len(sims) > 5
    assert [r for r in g if r["metadata"]["topic"] == "78"][0]["metadata"]["topic_cohesion"] == 0.5
    assert len(by["clustered"]["topic"]) > 100


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        json.dump(run(sys.argv[2]), sys.stdout)
        return
    if len(sys.argv) != 2:
        sys.exit("usage: make_relations_golden.py /path/to/reference")
    ref = sys.argv[1]
    cases = run(ref)
    check(cases)
    mine = json.loads(json.dumps(cases))
    for seed in ("1", "4242"):
        if os.environ.get("PYTHONHASHSEED") == seed:
            continue
        env = dict(os.environ, PYTHONHASHSEED=seed)
        other = json.loads(subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", ref], env=env))
        for a, b in zip(mine, other):
            if a != b:
                sys.exit(f"refused: case {a['name']} differs under PYTHONHASHSEED={seed}")
    packed = []
    for c in mine:
        p = {"name": c["name"], "threshold": c["threshold"], "notes": c["notes"],
             "coexistence": setjoin_ref.pack_coexistence(c["coexistence"], c["notes"]),
             "topic": setjoin_ref.pack_topic(c["topic"], c["notes"])}
        back = setjoin_ref.expand_case(json.loads(json.dumps(p)))
        setjoin_ref.same_relations(back["coexistence"], c["coexistence"], ordered_keys=True)
        setjoin_ref.same_relations(back["topic"], c["topic"], ordered_keys=True)
        packed.append(p)
    path = os.path.join(HERE, "relation_cases.json")
    with open(path, "w") as f:
        f.write('{"source": "reference graph/relation_extractor.py RelationExtractor.extract_entity_coexistence_relations '
                '(canonical order) and extract_topic_relations (its own order)",\n "cases": [\n')
        f.write(",\n".join(json.dumps(p, separators=(",", ":")) for p in packed))
        f.write("\n]}\n")
    for c in cases:
        print(f"{c['name']}: notes={len(c['notes'])} threshold={c['threshold']} coexistence={len(c['coexistence'])} "
              f"topic={len(c['topic'])}")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
