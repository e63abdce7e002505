"""CPU tests (no GPU needed) of HDBSCAN topic clustering: the numpy restatement (tests/hdbscan_ref.py) against the stored
results of sklearn and the reference (tests/golden/hdbscan_cases.npz), and the library's host tree stage
(anr_hdbscan_labels, csrc/hdbscan_tree.hpp) against both — through ctypes, and as a stand-alone program under the address
and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import hdbscan_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = hr.load_cases()
CASE_IDS = [c["id"] for c in CASES]


def test_the_golden_file_holds_the_cases_the_checks_rest_on():
    assert len(CASES) >= 8 and sum(c["n_ties"] > 0 for c in CASES) >= 5
    assert any(c["kind"] == "dups" for c in CASES) and any(c["min_samples"] == 1 for c in CASES)
    assert any((c["min_cluster_size"], c["min_samples"], c["eps"]) == (10, 3, 0.0) for c in CASES)
    assert any(c["n"] % 64 and c["d"] % 64 for c in CASES) and any((c["n"], c["d"]) == (2000, 384) for c in CASES)
    assert sum(bool((c["labels"] < 0).all()) for c in CASES) == 1
    for c in CASES:
        assert c["x"].dtype == np.float32 and c["x"].shape == (c["n"], c["d"])
        assert float(c["x"].astype(np.float64).sum()) == c["checksum"]
        assert hr.count_ties(c["w"]) == c["n_ties"]


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_restatement_reproduces_sklearn_bit_for_bit_and_the_labels_under_both_tie_orders(c):
    core = hr.core_distances(c["x"], c["min_samples"])
    assert np.array_equal(core, c["core"])
    src, dst, w = hr.prim_mst(c["x"], core)
    assert np.array_equal(src, c["src"]) and np.array_equal(dst, c["dst"]) and np.array_equal(w, c["w"])
    for order in ("stable", "reversed"):
        assert np.array_equal(hr.labels_from_mst(src, dst, w, c["min_cluster_size"], c["eps"], order), c["labels"]), order


def _lib_labels(src, dst, w, mcs, eps, **kw):
    from anorag_hip.topic_clustering import hdbscan_tree_labels
    return hdbscan_tree_labels(src, dst, w, mcs, eps, **kw)


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_library_tree_stage_gives_the_reference_labels_on_every_golden_tree(c):
    labels, st = _lib_labels(c["src"], c["dst"], c["w"], c["min_cluster_size"], c["eps"], return_stats=True)
    assert labels.dtype == np.int64 and np.array_equal(labels, c["labels"])
    assert st["n_clusters"] == int(c["labels"].max()) + 1 and st["n_noise"] == int((c["labels"] < 0).sum())
    assert st["tied_edges"] == c["n_ties"]


def small_trees():
    """(name, src, dst, w): trees on which the order of equal weights decides, and the smallest ones"""
    out = []
    for n, d, seed in ((200, 3, 6), (257, 5, 7)):
        x = hr.make_rows("lattice", n, d, seed)
        for ms in (1, 3):
            out.append((f"lattice-{n}x{d}-ms{ms}",) + hr.prim_mst(x, hr.core_distances(x, ms)))
    rng = np.random.default_rng(12)
    n = 40
    out.append(("path", np.arange(n - 1), np.arange(1, n), np.round(rng.random(n - 1) * 4) / 4 + 0.25))
    out.append(("star", np.zeros(n - 1, dtype=np.int64), np.arange(1, n), np.round(rng.random(n - 1) * 3) / 2 + 0.5))
    out.append(("all-equal", rng.permutation(n - 1), n - 1 - np.zeros(n - 1, dtype=np.int64), np.full(n - 1, 0.75)))
    out.append(("all-zero", np.arange(n - 1), np.arange(1, n), np.zeros(n - 1)))
    out.append(("two-rows", np.array([0]), np.array([1]), np.array([1.5])))
    x = hr.make_rows("dups", 120, 2, 1)
    out.append(("dups-120x2",) + hr.prim_mst(x, hr.core_distances(x, 3)))
    return [(name, np.asarray(s, dtype=np.int64), np.asarray(t, dtype=np.int64), np.asarray(w, dtype=np.float64))
            for name, s, t, w in out]


TREES = small_trees()


def tree_params(w):
    n = len(w) + 1
    top = float(w.max())
    return [(mcs, eps) for mcs in (2, 5, n + 1) for eps in (0.0, 0.1, 2.0 * top + 1.0)] + [(3, top), (3, float(np.median(w)))]


@pytest.mark.parametrize("name,src,dst,w", TREES, ids=[t[0] for t in TREES])
def test_library_tree_stage_equals_the_restatement_with_the_stable_order(name, src, dst, w):
    n = len(w) + 1
    for mcs, eps in tree_params(w):
        exp = hr.labels_from_mst(src, dst, w, mcs, eps, "stable")
        got = _lib_labels(src, dst, w, mcs, eps)
        assert np.array_equal(got, exp), (mcs, eps)
        if mcs > n:
            assert (got == -1).all()


def test_the_tie_order_decides_somewhere_so_the_stable_order_is_a_choice():
    """on the lattice the labels under the two orders differ: what the library follows is the stable one"""
    differ = 0
    for name, src, dst, w in TREES:
        if not name.startswith("lattice"):
            continue
        for mcs, eps in ((5, 0.1), (5, 0.0), (3, 0.0), (2, 0.0)):
            a = hr.labels_from_mst(src, dst, w, mcs, eps, "stable")
            b = hr.labels_from_mst(src, dst, w, mcs, eps, "reversed")
            if not np.array_equal(a, b):
                differ += 1
                assert np.array_equal(_lib_labels(src, dst, w, mcs, eps), a)
    assert differ > 0


def test_argument_errors_return_minus_one_with_a_message():
    from anorag_hip import _lib
    lib = _lib.load()
    src, dst, w = np.array([0, 1], dtype=np.int64), np.array([1, 2], dtype=np.int64), np.array([1.0, 2.0])
    labels, stats = np.zeros(3, dtype=np.int32), np.zeros(8, dtype=np.int64)

    def call(n, s, t, ww, mcs, eps, lab=labels):
        return lib.anr_hdbscan_labels(n, s.ctypes.data if s is not None else None, t.ctypes.data, ww.ctypes.data, mcs, eps,
                                      lab.ctypes.data if lab is not None else None, stats.ctypes.data)

    assert call(3, src, dst, w, 2, 0.0) == 0
    for args, word in (((1, src, dst, w, 2, 0.0), "at least 2 rows"), ((3, src, dst, w, 1, 0.0), "min_cluster_size"),
                       ((3, src, dst, w, 2, -0.5), "epsilon"), ((3, src, dst, w, 2, float("nan")), "epsilon"),
                       ((3, None, dst, w, 2, 0.0), "null"), ((3, src, dst, w, 2, 0.0, None), "null"),
                       ((3, np.array([0, 3], dtype=np.int64), dst, w, 2, 0.0), "outside"),
                       ((3, np.array([0, -1], dtype=np.int64), dst, w, 2, 0.0), "outside"),
                       ((3, src, dst, np.array([1.0, np.nan]), 2, 0.0), "weight"),
                       ((3, src, dst, np.array([1.0, np.inf]), 2, 0.0), "weight"),
                       ((3, src, dst, np.array([-1.0, 1.0]), 2, 0.0), "weight"),
                       ((3, src, np.array([1, 0], dtype=np.int64), w, 2, 0.0), "cycle")):
        assert call(*args) == -1, word
        assert word in _lib.last_error(), (word, _lib.last_error())
    with pytest.raises(ValueError, match="min_cluster_size"):
        _lib_labels(src, dst, w, 1, 0.0)
    with pytest.raises(ValueError, match="N - 1 edges"):
        _lib_labels(src, dst[:1], w, 2, 0.0)


def test_python_layer_rejects_bad_inputs_before_any_device_work():
    from anorag_hip import topic_clustering as tc
    x = hr.make_rows("gauss", 20, 4, 0)
    with pytest.raises(ValueError, match="above the 16"):
        tc.hdbscan_mst(x, tc.HDBSCAN_MAX_MIN_SAMPLES + 1)
    with pytest.raises(ValueError, match="at least 1"):
        tc.hdbscan_mst(x, 0)
    with pytest.raises(ValueError, match="at least 2 rows"):
        tc.hdbscan_mst(x[:1], 1)
    with pytest.raises(ValueError, match=r"min_samples \(5\) must be at most the number of samples in X \(4\)"):
        tc.hdbscan_mst(x[:4], 5)
    bad = x.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        tc.hdbscan_mst(bad, 3)
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="NaN or infinite"):
        tc.hdbscan_labels(bad, 5, 3)
    with pytest.raises(ValueError, match="min_cluster_size"):
        tc.hdbscan_labels(x, 1)
    with pytest.raises(ValueError, match="N, d"):
        tc.hdbscan_mst(x[0], 3)
    with pytest.raises(NotImplementedError):
        tc.cluster_labels(x, "hdbscan")


def _tree_text(src, dst, w, mcs, eps):
    lines = [f"{len(w) + 1} {mcs} {float(eps).hex()}"]
    lines += [f"{int(a)} {int(b)} {float(c).hex()}" for a, b, c in zip(src, dst, w)]
    return "\n".join(lines) + "\n"


def test_tree_stage_alone_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "hdbscan_tree_test")
    # the sanitizers' runtimes are linked into the program, so it starts in whatever environment the suite runs in
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "ano-rag_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "hdbscan_tree_test.cpp"), "-o", exe], check=True)
    text, expected = [], []
    for name, src, dst, w in TREES:
        for mcs, eps in tree_params(w):
            text.append(_tree_text(src, dst, w, mcs, eps))
            expected.append(hr.labels_from_mst(src, dst, w, mcs, eps, "stable"))
    c = CASES[1]  # the golden with a block of identical rows: zero weights, lambda = inf
    text.append(_tree_text(c["src"], c["dst"], c["w"], c["min_cluster_size"], c["eps"]))
    expected.append(c["labels"])
    text.append("3 2 0x0p+0\n0 1 0x1p+0\n1 0 0x1p+1\n")  # a cycle
    text.append("1 2 0x0p+0\n")                           # a single row
    out = subprocess.run([exe], input="".join(text), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(expected) + 2
    for line, exp in zip(lines, expected):
        f = line.split()
        assert f[0] == "ok" and int(f[1]) == int(exp.max()) + 1
        assert np.array_equal(np.array(f[2:], dtype=np.int64), exp)
    assert lines[-2].startswith("error") and "cycle" in lines[-2]
    assert lines[-1].startswith("error") and "at least 2 rows" in lines[-1]
