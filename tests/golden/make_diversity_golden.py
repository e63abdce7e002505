#!/usr/bin/env python3
"""Golden cases for the diversity scheduler, produced by RUNNING THE REFERENCE's own DiversityScheduler
(retrieval/diversity_scheduler.py) on seeded candidate dicts (build container only, CPU; needs the reference checkout):

  python tests/golden/make_diversity_golden.py <path to the reference checkout>

writes tests/golden/diversity_cases.npz.  Data only, no reference source: per case c<i>_* the inputs (embeddings as
float32, scores, the fields that drive type inference and coverage: tests/diversity_ref.py CASE_ARRAYS) and the
reference's answers (c<i>_kept_ids after dedup, c<i>_selected_ids in selection order, c<i>_type_mask of every input
candidate, c<i>_coverage); per-file arrays strategy, max_candidates, dedup_method, dedup_threshold, quota (0: the plain
form, enable_evidence_quota set to False AFTER construction), diversity_score, dedup_stats, kinds.
utils.logging_utils and utils.config_loader_helper are STAND-INS in sys.modules: nothing pinned here lives in them.

A case is kept only if the float64 restatement (tests/diversity_ref.py) meets no decision closer than 1e-9 on it: a
condition on the INPUT (the rounding bound of the device's similarity is ~1e-13).  The kept set must contain every kind
in KINDS at least once; the script fails otherwise.  Never imported by a test.
"""
import importlib.util
import os
import sys
import types

import numpy as np

if len(sys.argv) < 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import diversity_ref as dr  # noqa: E402

KINDS = ["dedup_replaced", "dedup_dropped", "passthrough", "quota_round_two", "plain", "stopped_short", "zero_norm",
         "no_embedding", "topical", "identical_rows"]
WORDS = ("alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu nu xi omicron pi rho sigma tau upsilon "
         "phi chi psi omega").split()
TOPICS = ["t%d" % i for i in range(9)]


def load_reference():
    ut = types.ModuleType("utils")
    ut.__path__ = []
    lu = types.ModuleType("utils.logging_utils")

    class StructuredLogger:
        def __init__(self, *a, **k):
            pass

        def __getattr__(self, _):
            return lambda *a, **k: None

    lu.StructuredLogger = StructuredLogger
    lu.log_performance = lambda *a, **k: (lambda f: f)
    lu.log_diversity_metrics = lambda *a, **k: None
    ch = types.ModuleType("utils.config_loader_helper")
    ch.load_config_with_fallback = lambda path, fallback, key=None: fallback
    sys.modules.update({"utils": ut, "utils.logging_utils": lu, "utils.config_loader_helper": ch})
    spec = importlib.util.spec_from_file_location("ref_diversity", os.path.join(REF, "retrieval", "diversity_scheduler.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_diversity"] = mod
    spec.loader.exec_module(mod)
    return mod


def make_case(rng, kind):
    C = int(rng.integers(24, 61))
    d = int(rng.choice([8, 16, 32, 64] if C <= 40 else [8, 16, 32]))
    centres = rng.standard_normal((6, d))
    emb = (centres[rng.integers(0, 6, C)] * rng.uniform(0.0, 1.5) + rng.standard_normal((C, d))).astype(np.float32)
    scores = np.round(rng.uniform(0.05, 1.3, C), 6)
    for _ in range(int(rng.integers(3, 9))):   # near-duplicates: some above, some below the dedup threshold
        a, b = rng.integers(0, C, 2)
        if a != b:
            emb[b] = (emb[a] + rng.uniform(0.02, 0.6) * rng.standard_normal(d)).astype(np.float32)
    has = np.ones(C, dtype=bool)
    strategy, method, thr, quota = "hybrid", "hybrid", 0.85, 1
    maxc = int(rng.integers(5, max(6, C // 2)))
    if kind == "passthrough":
        maxc = C + int(rng.integers(0, 5))
    elif kind == "plain":
        quota = 0
    elif kind == "stopped_short":
        quota = int(rng.integers(0, 2))
        scores[rng.permutation(C)[: C - 3]] = np.round(rng.uniform(-14.0, -8.0, C - 3), 6)
        maxc = 8
    elif kind == "zero_norm":
        emb[rng.integers(0, C, 2)] = 0.0
        quota = int(rng.integers(0, 2))
    elif kind == "no_embedding":
        has[rng.permutation(C)[: int(rng.integers(3, C // 2))]] = False
        method = "semantic"
    elif kind == "topical":
        strategy = "topical"
        quota = int(rng.integers(0, 2))
    elif kind == "identical_rows":
        thr, quota = 1.5, int(rng.integers(0, 2))
        a, b = 1, int(rng.integers(2, C))
        emb[b] = emb[a]
        scores[a] = scores[b] = 0.31
        scores[0] = 1.2
        maxc = max(maxc, 6)
    elif kind == "hash":
        method = "hash"
    content, ents, tops = [], [], []
    for j in range(C):
        nw = int(rng.integers(2, 9))
        content.append(" ".join(rng.choice(WORDS, nw)) + f" n{j}")
        ents.append("|".join(f"e{int(x)}" for x in rng.integers(0, 12, int(rng.integers(0, 7)))))
        tops.append("|".join(sorted(set(rng.choice(TOPICS, int(rng.integers(0, 4)))))))
    if C > 5:
        content[4] = content[2]    # one hash duplicate
    src_mask = rng.integers(0, 8, C)
    path_score = np.round(rng.uniform(0.0, 0.6, C), 6)
    ts = np.where(rng.random(C) < 0.7, 1.7e9 + np.round(rng.uniform(0, 120000.0 if rng.random() < 0.5 else 30000.0, C), 3), np.nan)
    source = np.array([("s%d" % int(x)) if rng.random() < 0.8 else "" for x in rng.integers(0, 5, C)])
    arrays = {"emb": emb, "has_emb": has, "ids": np.array([f"note_{j:03d}" for j in range(C)]), "content": np.array(content),
              "scores": scores.astype(np.float64), "path_score": path_score, "src_mask": src_mask.astype(np.int32),
              "entities": np.array(ents), "topics": np.array(tops), "timestamp": ts, "source": source}
    cfg = {"strategy": dr.STRATEGIES.index(strategy), "max_candidates": maxc, "dedup_method": dr.DEDUP_METHODS.index(method),
           "dedup_threshold": thr, "quota": quota}
    return arrays, cfg


def main():
    ref = load_reference()
    rng = np.random.default_rng(20240611)
    out, per_file, kinds_seen, n = {}, {k: [] for k in ("strategy", "max_candidates", "dedup_method", "dedup_threshold", "quota",
                                                       "diversity_score", "dedup_stats", "kinds")}, {k: 0 for k in KINDS}, 0
    plan = (KINDS + ["hash", "base"]) * 4
    rejected = 0
    for kind in plan:
        arrays, cfg = make_case(rng, kind if kind != "base" else "")
        if kind == "quota_round_two":   # mostly untyped candidates: round one leaves room
            few = rng.random(len(arrays["scores"])) < 0.85
            arrays["src_mask"][few] = 0
            arrays["path_score"][few] = np.round(arrays["path_score"][few] * 0.4, 6)
            arrays["scores"][few] = np.round(arrays["scores"][few] * 0.5, 6)
            arrays["entities"][few] = ""
        z = {f"c0_{k}": v for k, v in arrays.items()}
        z.update({k: np.array([v]) for k, v in cfg.items()})
        cands = dr.case_candidates(z, 0)
        config, plain = dr.case_config(z, 0)
        res = dr.restate_case(cands, dr.STRATEGIES[cfg["strategy"]], cfg["max_candidates"], dr.DEDUP_METHODS[cfg["dedup_method"]],
                              cfg["dedup_threshold"], bool(cfg["quota"]))
        if not res["margin"] > dr.MARGIN:
            rejected += 1
            continue
        sch = ref.DiversityScheduler(config)
        if plain:
            sch.diversity_config.enable_evidence_quota = False
        items = sch._convert_to_candidate_items(cands)
        kept, _ = sch.deduplication_processor.deduplicate(items)
        result = sch.schedule_candidates(cands, "q")
        masks = [sum(1 << dr.TYPE_NAMES.index(t) for t in it.evidence_types) for it in items]
        info = res["info"]
        flags = {"dedup_replaced": info["replaced"] > 0, "dedup_dropped": info["dropped"] > 0, "passthrough": info["passthrough"],
                 "quota_round_two": bool(cfg["quota"]) and info["round_two_picks"] > 0,
                 "plain": not cfg["quota"] and not info["passthrough"], "stopped_short": info["stopped_short"],
                 "zero_norm": bool(np.any(~arrays["emb"].any(axis=1))), "no_embedding": not arrays["has_emb"].all(),
                 "topical": cfg["strategy"] == 2 and not info["passthrough"],
                 "identical_rows": kind == "identical_rows" and not info["passthrough"]}
        for k, v in flags.items():
            kinds_seen[k] += int(v)
        for k, v in arrays.items():
            out[f"c{n}_{k}"] = v
        out[f"c{n}_kept_ids"] = np.array([it.id for it in kept])
        out[f"c{n}_selected_ids"] = np.array([it.id for it in result.selected_candidates])
        out[f"c{n}_type_mask"] = np.array(masks, dtype=np.int32)
        cov = result.coverage_metrics
        out[f"c{n}_coverage"] = np.array([cov.get(k, np.nan) for k in ("entity_coverage", "topic_coverage", "source_coverage",
                                                                      "temporal_coverage")])
        for k, v in cfg.items():
            per_file[k].append(v)
        per_file["diversity_score"].append(result.diversity_score)
        st = result.deduplication_stats
        per_file["dedup_stats"].append([st["total"], st["removed"], st["kept"]])
        per_file["kinds"].append(sum(1 << KINDS.index(k) for k, v in flags.items() if v))
        n += 1
    missing = [k for k, v in kinds_seen.items() if v == 0]
    print(f"kept {n} cases, rejected {rejected} by the margin; kinds: {kinds_seen}")
    if missing:
        raise SystemExit(f"no kept case of kind(s) {missing}: change the input generator, not the margin")
    out["n_cases"] = np.array(n)
    out["kind_names"] = np.array(KINDS)
    for k, v in per_file.items():
        out[k] = np.array(v)
    path = os.path.join(HERE, "diversity_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
