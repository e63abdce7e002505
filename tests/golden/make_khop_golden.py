#!/usr/bin/env python3
"""Golden cases for the second-hop rerank and the cluster suppression, produced by RUNNING THE REFERENCE's own method
bodies (build container only, CPU; needs the reference checkout):

  python tests/golden/make_khop_golden.py <path to the reference checkout>

query/query_processor.py cannot be imported here (LLM clients, rerankers, ...), so, as make_golden.py does for the candidate
fusion, four METHODS of QueryProcessor are taken from its source with ``ast`` and compiled as they stand:
_rerank_khop_candidates, _apply_cluster_suppression, _rrf_score, _compute_cov_cons.  They run on a stand-in ``self`` whose
collaborators return the case's recorded values: _calculate_vector_similarities (the dense scores for the query, the
focused score of the one candidate it is handed otherwise — looked up by candidate, never by the focus string, which the
reference assembles from a ``set`` and whose word order therefore follows the hash seed), _calculate_bm25_similarities,
_get_config_dict, _extract_relation_focus_phrase and vector_index.embed (float32 vectors by the candidate's text).  The
recorded scores are Python floats, so numpy's scalar promotion cannot enter the score arithmetic.

Writes tests/golden/khop_cases.json — data only, no reference source: per case the inputs, every final_score by its bits,
the reranked order and the kept list (positions of the case's candidate list).  A case is refused when
  - a float64 cosine of its vectors lies within ``margin`` = d * 2^-23 of the threshold: the reference takes the cosine as
    a float32 dot product of float32-normalised rows, whose error for unit rows stays below d rounding units of float32;
    the margin is stored in the fixture;
  - it comes out differently under another PYTHONHASHSEED (the script runs itself again under two other seeds);
  - the property it is there for does not hold (each case asserts it).
Never imported by a test.
"""
import ast
import copy
import json
import os
import random
import struct
import subprocess
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
METHODS = ("_rerank_khop_candidates", "_apply_cluster_suppression", "_rrf_score", "_compute_cov_cons")
QUERY = "who founded the company that acquired the studio"
ENTS = ["Acme", "Borealis", "Cobalt Studio", "Dara Lin", "Evermore", "Fjord", "Gale"]
WORDS = "alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu".split()


def bits(x):
    return struct.pack("<d", float(x)).hex()


def load_methods(ref):
    path = os.path.join(ref, "query", "query_processor.py")
    tree = ast.parse(open(path, encoding="utf-8").read())
    wanted = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef) and node.name == "QueryProcessor":
            for fn in node.body:
                if isinstance(fn, ast.FunctionDef) and fn.name in METHODS:
                    fn.decorator_list = []
                    wanted[fn.name] = fn
    assert set(wanted) == set(METHODS), sorted(wanted)

    class _Log:
        def __getattr__(self, _):
            return lambda *a, **k: None

    from typing import Any, Dict, List
    ns = {"List": List, "Dict": Dict, "Any": Any, "logger": _Log()}
    exec(compile(ast.fix_missing_locations(ast.Module(body=list(wanted.values()), type_ignores=[])), path, "exec"), ns)
    return ns


def stand_in(ns, case):
    """a ``self`` for the extracted methods: collaborators answer from the case"""
    by_id = {c["note_id"]: i for i, c in enumerate(case["candidates"])}
    vec_of = {}
    if case.get("vectors") is not None:
        d = case["dim"]
        for i, c in enumerate(case["candidates"]):
            vec_of[f"{c.get('title', '')} {c.get('content', '')}"] = np.asarray(case["vectors"][i * d:(i + 1) * d], dtype=np.float32)
        assert len(vec_of) == len(case["candidates"])

    def vector_sims(text, cands):
        src = case["dense"] if text == QUERY else case["focused"]
        self.focus_calls += text != QUERY
        return [src[by_id[c["note_id"]]] for c in cands]

    self = types.SimpleNamespace(focus_calls=0)
    self._get_config_dict = lambda a, b: dict(case["config"].get(b, {}))
    self._calculate_vector_similarities = vector_sims
    self._calculate_bm25_similarities = lambda q, cands: [case["bm25"][by_id[c["note_id"]]] for c in cands]
    self._extract_relation_focus_phrase = lambda q: case["relation_focus"]
    self.vector_index = types.SimpleNamespace(embed=lambda text: vec_of[text])
    for name in METHODS:
        setattr(self, name, types.MethodType(ns[name], self))
    return self


def run_case(ns, case):
    """the reference's answers for a case: rerank + suppression of the reranked list, or the suppression alone"""
    self = stand_in(ns, case)
    cands = copy.deepcopy(case["candidates"])
    pos = {c["note_id"]: i for i, c in enumerate(cands)}
    if case["kind"] == "suppress":
        for c, s in zip(cands, case["scores"]):
            c["final_score"] = s
        kept = self._apply_cluster_suppression(cands)
        return {"kept": [pos[c["note_id"]] for c in kept]}
    out = self._rerank_khop_candidates(QUERY, cands, case["path_entities"])
    final = [None] * len(cands)
    for c in out:
        assert type(c["final_score"]) is float
        final[pos[c["note_id"]]] = bits(c["final_score"])
    kept = self._apply_cluster_suppression(out)
    case["has_focus"] = self.focus_calls > 0   # whether the reference asked for a focused similarity at all
    assert self.focus_calls in (0, len(cands))
    return {"final_bits": final, "order": [pos[c["note_id"]] for c in out], "kept": [pos[c["note_id"]] for c in kept]}


# ---- inputs ----------------------------------------------------------------------------------------------------------
def f32_list(a):
    return [float(v) for v in np.asarray(a, dtype=np.float32).reshape(-1)]


def make_vectors(rng, C, d, groups):
    """rows around a few centres; ``groups``: lists of positions that are near-duplicates of their first member"""
    x = rng.standard_normal((C, d)) * np.exp(rng.uniform(-1.0, 1.0, (C, 1)))
    for g in groups:
        for j in g[1:]:
            x[j] = x[g[0]] * rng.uniform(0.5, 2.0) + rng.choice([0.05, 0.3, 0.7]) * np.linalg.norm(x[g[0]]) / np.sqrt(d) * rng.standard_normal(d)
    return x.astype(np.float32)


def make_case(rng, name, prop, C, d=16, *, fusion=None, features=None, cs=None, hops=(2,), prf="mixed", ties=False,
              path_entities=("Acme", "Cobalt Studio", "Dara Lin"), relation_focus="founded", groups=((0, 3), (1, 4, 6))):
    nr = np.random.default_rng(rng.randrange(1 << 30))
    cands = []
    for i in range(C):
        ents = rng.sample(ENTS, rng.randrange(0, 4))
        words = rng.sample(WORDS, rng.randrange(2, 6))
        if rng.random() < 0.4:
            words.append(rng.choice(ENTS).lower())
        is_prf = {"none": False, "all": True, "mixed": rng.random() < 0.45}[prf]
        c = {"note_id": f"n{i:03d}", "title": f"title {i}", "content": " ".join(words) + f" #{i}", "entities": ents,
             "hop_no": hops[i % len(hops)], "retrieval_method": "prf_bridge" if is_prf else "dense"}
        if is_prf or rng.random() < 0.3:
            c["similarity_score"] = round(rng.uniform(0.1, 0.9), 1 if ties else 6)
        cands.append(c)
    rnd = (lambda v: round(v, 1)) if ties else (lambda v: v)
    groups = [[j for j in g if j < C] for g in groups]
    vec = make_vectors(nr, C, d, [g for g in groups if len(g) > 1])
    return {"name": name, "property": prop, "kind": "rerank", "query": QUERY, "path_entities": list(path_entities),
            "relation_focus": relation_focus,
            "config": {"fusion": dict(fusion or {}), "features": dict(features or {}), "cluster_suppression": dict(cs or {})},
            "candidates": cands, "dense": [rnd(rng.uniform(0.0, 0.95)) for _ in range(C)],
            "bm25": [rnd(rng.uniform(0.0, 1.0)) if rng.random() < 0.8 else 0.0 for _ in range(C)],
            "focused": [rnd(rng.uniform(0.0, 0.9)) for _ in range(C)], "dim": d, "vectors": f32_list(vec)}


def build_cases():
    rng = random.Random(20261019)
    cases = []

    def add(*a, **k):
        cases.append(make_case(rng, *a, **k))
        return cases[-1]

    add("ties", "ties in dense and in bm25: ranks follow candidate order", 14, ties=True)
    add("prf_none", "no PRF candidate: two rankings only", 9, prf="none")
    add("prf_all", "every candidate is a PRF candidate", 9, prf="all")
    add("prf_mixed", "the PRF ranking covers only the PRF candidates", 13, prf="mixed", ties=True)
    add("hops", "hop_no 1, 2, 3, 5: the focused weight at hop 5 clamps to 0.0", 12, hops=(1, 2, 3, 5),
        fusion={"focused_weight_hop2": 0.30})
    add("decay_085", "hop_decay 0.85 applies from hop 2", 10, hops=(1, 2, 3, 5), features={"hop_decay": 0.85})
    add("decay_one", "hop_decay 1.0 is outside (0, 1): no decay", 10, hops=(1, 2, 3), features={"hop_decay": 1.0})
    add("decay_zero", "hop_decay 0 is outside (0, 1): no decay", 10, hops=(2, 3), features={"hop_decay": 0})
    add("no_focus", "no focus phrase: focused is 0.0", 8, path_entities=(), relation_focus="")
    add("no_path_entities", "empty path_entities: cov and cons are 0", 8, path_entities=(), relation_focus="acquired studio")
    add("keep_1", "keep_per_cluster 1", 12, cs={"keep_per_cluster": 1, "cos_threshold": 0.9}, groups=((0, 3, 7), (1, 4, 6, 9)))
    add("keep_2", "keep_per_cluster 2", 12, cs={"keep_per_cluster": 2}, groups=((0, 3, 7), (1, 4, 6, 9)))
    add("keep_all", "keep_per_cluster >= C: nothing is dropped", 12, cs={"keep_per_cluster": 40}, groups=((0, 3, 7), (1, 4, 6, 9)))
    add("disabled", "suppression disabled: candidates pass through", 9, cs={"enabled": "False"})
    add("unparsable", "values that cannot be parsed fall back to the defaults", 9,
        fusion={"dense_weight": "much", "bm25_weight": None, "rrf_lambda": "0.35"}, features={"cov_weight": []},
        cs={"cos_threshold": "high", "keep_per_cluster": "two"})
    add("one", "a single candidate", 1, groups=())
    add("larger", "forty candidates, dimension 32", 40, d=32, hops=(2, 2, 3), groups=((0, 9, 17, 33), (2, 5), (11, 12, 13)))

    # the suppression alone, on input that is not sorted by score
    def sup(name, prop, C, d, scores, groups, cs, edit=None):
        nr = np.random.default_rng(rng.randrange(1 << 30))
        vec = make_vectors(nr, C, d, groups)
        if edit:
            edit(vec)
        cands = [{"note_id": f"s{i:03d}", "title": f"t{i}", "content": f"text {i}"} for i in range(C)]
        cases.append({"name": name, "property": prop, "kind": "suppress", "config": {"cluster_suppression": cs},
                      "candidates": cands, "scores": scores, "dim": d, "vectors": f32_list(vec)})

    sup("unsorted", "a seed loses its place to a later, higher-scored member", 8, 16,
        [0.2, 0.9, 0.5, 0.7, 0.1, 0.7, 0.3, 0.6], [[0, 3, 5], [2, 6]], {"keep_per_cluster": 1})
    sup("identical_rows", "cosine of a row with its duplicate", 7, 8, [0.5, 0.4, 0.6, 0.4, 0.3, 0.8, 0.1], [], {},
        edit=lambda v: v.__setitem__(4, v[1]))
    sup("zero_row", "a zero row: cosine is 0", 6, 8, [0.5, 0.4, 0.6, 0.4, 0.3, 0.8], [[1, 5]], {"keep_per_cluster": 1},
        edit=lambda v: v.__setitem__(2, 0.0))
    sup("equal_scores", "equal scores inside a cluster and in the final sort keep their order", 9, 16,
        [0.5, 0.5, 0.7, 0.5, 0.7, 0.5, 0.2, 0.5, 0.7], [[1, 3, 5, 7]], {"keep_per_cluster": 2})
    return cases


# ---- checks ----------------------------------------------------------------------------------------------------------
def cosines64(case):
    C, d = len(case["candidates"]), case["dim"]
    a = np.asarray(case["vectors"], dtype=np.float32).reshape(C, d).astype(np.float64)
    n = np.sqrt(np.einsum("ij,ij->i", a, a)) + 1e-8
    return (a @ a.T) / (n[:, None] * n[None, :])


def check_property(case, out):
    name, C = case["name"], len(case["candidates"])
    cos = cosines64(case)
    above = [(i, j) for i in range(C) for j in range(i + 1, C) if cos[i, j] >= 0.9]
    if name == "ties":
        assert len(set(case["dense"])) < C and len(set(case["bm25"])) < C
    elif name == "prf_none":
        assert not any(c["retrieval_method"] == "prf_bridge" for c in case["candidates"])
    elif name == "prf_all":
        assert all(c["retrieval_method"] == "prf_bridge" for c in case["candidates"])
    elif name == "prf_mixed":
        n = sum(c["retrieval_method"] == "prf_bridge" for c in case["candidates"])
        assert 1 < n < C
        assert any("similarity_score" in c and c["retrieval_method"] != "prf_bridge" for c in case["candidates"])
    elif name == "hops":
        assert {c["hop_no"] for c in case["candidates"]} == {1, 2, 3, 5} and 0.30 - 0.10 * 3 < 0.0
        assert any(c["hop_no"] == 5 and f > 0.0 for c, f in zip(case["candidates"], case["focused"]))
    elif name.startswith("decay"):
        assert any(c["hop_no"] > 1 for c in case["candidates"])
    elif name == "no_focus":
        assert not case["has_focus"] and not case["path_entities"] and not case["relation_focus"] and any(f > 0.0 for f in case["focused"])
    elif name == "no_path_entities":
        assert not case["path_entities"] and case["relation_focus"]
    elif name in ("keep_1", "keep_2"):
        assert len(out["kept"]) < C and above
    elif name == "keep_all":
        assert sorted(out["kept"]) == list(range(C)) and above
    elif name == "disabled":
        assert out["kept"] == out["order"] and above
    elif name == "unsorted":
        assert 0 not in out["kept"] and (3 in out["kept"] or 5 in out["kept"])
    elif name == "identical_rows":
        assert (1 in out["kept"]) and (4 in out["kept"]) and cos[1, 4] >= 0.9   # keep_m 2: both of the pair stay
        assert len(out["kept"]) == C
    elif name == "zero_row":
        assert not cos[2].any() and 2 in out["kept"]
    elif name == "equal_scores":
        assert len(out["kept"]) < C
    return True


def margin_ok(case):
    thr = case["config"].get("cluster_suppression", {}).get("cos_threshold", 0.90)
    try:
        thr = float(thr)
    except (TypeError, ValueError):
        thr = 0.90
    case["margin"] = case["dim"] * 2.0 ** -23
    cos = cosines64(case)
    iu = np.triu_indices(cos.shape[0], 1)
    return not np.any(np.abs(cos[iu] - thr) <= case["margin"])


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    ns = load_methods(ref)
    cases = build_cases()
    for case in cases:
        if not margin_ok(case):
            raise SystemExit(f"case {case['name']}: a cosine lies within {case['margin']} of the threshold; change the inputs")
        case["expected"] = run_case(ns, case)
        check_property(case, case["expected"])
    text = json.dumps({"rrf_k": 50, "cases": cases}, indent=None, separators=(",", ":"), sort_keys=True)
    if len(sys.argv) > 2 and sys.argv[2] == "--print":
        sys.stdout.write(text)
        return
    for seed in ("1", "4242"):
        env = dict(os.environ, PYTHONHASHSEED=seed)
        other = subprocess.run([sys.executable, os.path.abspath(__file__), ref, "--print"], env=env, check=True,
                               capture_output=True, text=True).stdout
        if other != text:
            a, b = json.loads(text)["cases"], json.loads(other)["cases"]
            bad = [x["name"] for x, y in zip(a, b) if x != y]
            raise SystemExit(f"cases {bad} change under PYTHONHASHSEED={seed}")
    path = os.path.join(HERE, "khop_cases.json")
    with open(path, "w", encoding="utf-8") as f:
        f.write(text + "\n")
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
