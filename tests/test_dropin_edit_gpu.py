"""GPU tests of the drop-in classes' in-place edits: VectorIndex.remove_vectors / update_vectors on an exact single-device
index edit the rows where they are (same index object, results of a rebuilt index), and VectorRetriever.remove_notes /
update_note under the config key anorag_hip.inplace_edits re-encode nothing but the one updated note."""
import numpy as np
import pytest

from oracle import encoder as oenc

pytestmark = pytest.mark.gpu

SIM_TOL = 5e-4       # the drop-in tests' bar on similarities


@pytest.fixture()
def cfg(tmp_path):
    from anorag_hip.compat import config
    config.reset()
    config.set("storage.vector_index_path", str(tmp_path / "vidx"))
    config.set("storage.vector_store_path", str(tmp_path / "vstore"))
    config.set("storage.embedding_cache_path", str(tmp_path / "ecache"))
    config.set("vector_store.index_type", "Flat")
    yield config
    config.reset()


@pytest.fixture()
def model_dir(tmp_path):
    return oenc.make_synthetic_model(str(tmp_path / "bge-small-synth"), layers=2, hidden=128, heads=4,
                                     intermediate=512, pooling="cls", max_pos=128)


def _hits(res):
    return [[(h["index"], h["rank"]) for h in r] for r in res], np.array([[h["similarity"] for h in r] for r in res])


def test_vector_index_edits_in_place_and_equals_a_rebuilt_index(cfg):
    from anorag_hip import FlatIndex
    from vector_store import VectorIndex
    rng = np.random.default_rng(0)
    n, d = 700, 96
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((4, d)).astype(np.float32)
    vi = VectorIndex(d)
    assert vi.create_index() and vi.add_vectors(x, np.arange(n))
    assert type(vi.index) is FlatIndex
    held = vi.index
    drop = np.array([0, 5, 5, 333, n - 1])
    assert vi.remove_vectors(drop) is True
    assert vi.index is held, "the index was rebuilt instead of edited"
    assert vi.index.ntotal == n - 4 and vi.total_vectors == n - 5       # (the reference subtracts what was asked for)
    survivors = np.delete(x, np.unique(drop), axis=0)
    ref = VectorIndex(d)
    assert ref.create_index() and ref.add_vectors(survivors)
    got, want = _hits(vi.search(q, top_k=9)), _hits(ref.search(q, top_k=9))
    assert got[0] == want[0] and np.max(np.abs(got[1] - want[1])) <= SIM_TOL

    ids = np.array([3, 77, n - 5, 77])
    new = rng.standard_normal((4, d)).astype(np.float32)
    new[1] = q[0] * 3.0                                                  # overwritten by the later entry for row 77
    new[3] = q[1] * 2.0                                                  # ... which becomes query 1's best hit
    assert vi.update_vectors(ids, new) is True and vi.index is held
    edited = survivors.copy()
    edited[[3, 77, n - 5]] = new[[0, 3, 2]]
    ref2 = VectorIndex(d)
    assert ref2.create_index() and ref2.add_vectors(edited)
    got, want = _hits(vi.search(q, top_k=9)), _hits(ref2.search(q, top_k=9))
    assert got[0] == want[0] and np.max(np.abs(got[1] - want[1])) <= SIM_TOL
    assert got[0][1][0] == (77, 0) and abs(got[1][1][0] - 1.0) <= 1e-5
    # the class's sentinel on errors: an unknown id changes nothing
    before = vi.index.reconstruct_n(0, vi.index.ntotal)
    assert vi.update_vectors(np.array([2, n]), new[:2]) is False
    assert vi.update_vectors(np.array([2]), new[:2]) is False
    assert np.array_equal(vi.index.reconstruct_n(0, vi.index.ntotal), before)
    assert VectorIndex(d).update_vectors(np.array([0]), new[:1]) is False        # no index yet
    for v in (vi, ref, ref2):
        v.cleanup()


def _retriever(cfg, model_dir, n_notes, seed):
    from vector_store import EmbeddingManager, VectorRetriever
    EmbeddingManager._reset_singleton()
    cfg.set("embedding.model_path", model_dir)
    cfg.set("embedding.max_length", 64)
    cfg.set("embedding.batch_size", 8)
    cfg.set("vector_store.similarity_threshold", 0.0001)
    words = oenc.synthetic_sentences(model_dir, n_notes + 2, seed=seed, min_words=4, max_words=12)
    notes = [{"note_id": f"n{i}", "title": f"t{i}", "content": w, "entities": ["e1"]} for i, w in enumerate(words[:n_notes])]
    return VectorRetriever, words, notes


def _count_encodes(monkeypatch, em):
    """notes / texts handed to the encoder, per call"""
    seen = []
    for name in ("encode_atomic_notes", "encode_texts_device", "encode_texts"):
        if hasattr(em, name):
            orig = getattr(em, name)
            monkeypatch.setattr(em, name, lambda items, *a, _o=orig, _n=name, **k: (seen.append((_n, len(items))), _o(items, *a, **k))[1])
    return seen


def _same_search(a, b, queries):
    ra, rb = a.search(queries, top_k=6), b.search(queries, top_k=6)
    assert [[h["note_id"] for h in r] for r in ra] == [[h["note_id"] for h in r] for r in rb]
    for x, y in zip(ra, rb):
        assert len(x) > 0
        for hx, hy in zip(x, y):
            assert hx["retrieval_info"]["rank"] == hy["retrieval_info"]["rank"]
            assert abs(hx["retrieval_info"]["similarity"] - hy["retrieval_info"]["similarity"]) <= SIM_TOL
            assert hx["content"] == hy["content"]


def test_retriever_edits_in_place_under_the_config_key(cfg, model_dir, monkeypatch):
    from vector_store import EmbeddingManager
    VectorRetriever, words, notes = _retriever(cfg, model_dir, 40, seed=31)
    cfg.set("anorag_hip.inplace_edits", True)
    vr = VectorRetriever()
    assert vr.build_index([dict(n) for n in notes], save_index=False) is True
    held = vr.vector_index.index
    emb0 = vr.note_embeddings.copy()
    rebuilds = []
    orig_build = vr.build_index
    monkeypatch.setattr(vr, "build_index", lambda *a, **k: (rebuilds.append(1), orig_build(*a, **k))[1])
    seen = _count_encodes(monkeypatch, vr.embedding_manager)
    queries = words[:3] + [words[38]]

    assert vr.remove_notes(["n0", "n17", "n39", "missing"]) is True
    assert seen == [] and rebuilds == [], "a removal encoded notes or rebuilt the index"
    assert vr.vector_index.index is held and held.ntotal == 37 and len(vr.atomic_notes) == 37
    assert vr.note_embeddings.shape == (37, 128) and vr.note_id_to_index["n1"] == 0 and "n17" not in vr.note_id_to_index
    assert vr.note_id_to_index["n38"] == 36 and vr.index_to_note_id[36] == "n38"
    kept = [dict(n) for n in notes if n["note_id"] not in ("n0", "n17", "n39")]
    assert np.array_equal(vr.note_embeddings, np.delete(emb0, [0, 17, 39], axis=0))
    if vr.bm25_enabled and vr.tfidf_matrix is not None:
        assert vr.tfidf_matrix.shape[0] == 37

    updated = dict(kept[4], content=words[40], title="rewritten")
    assert vr.update_note(kept[4]["note_id"], dict(updated)) is True
    assert [s for s in seen if s[0] == "encode_atomic_notes"] == [("encode_atomic_notes", 1)] and rebuilds == []
    assert not [s for s in seen if s[0] == "encode_texts_device"], "the update encoded the corpus again"
    assert vr.vector_index.index is held and vr.atomic_notes[4]["title"] == "rewritten"
    kept[4] = updated
    del seen[:]

    fresh = VectorRetriever()
    assert fresh.build_index([dict(n) for n in kept], force_rebuild=True, save_index=False) is True
    _same_search(vr, fresh, queries + [words[40]])
    assert np.max(np.abs(vr.note_embeddings - fresh.note_embeddings)) <= SIM_TOL   # (row 4 was encoded alone, not in a batch)
    assert vr.remove_notes([n["note_id"] for n in kept]) is False               # an empty corpus is no index, as in a rebuild
    vr.cleanup()
    fresh.cleanup()
    EmbeddingManager._reset_singleton()


def test_retriever_without_the_key_still_rebuilds(cfg, model_dir, monkeypatch):
    from vector_store import EmbeddingManager
    VectorRetriever, words, notes = _retriever(cfg, model_dir, 20, seed=32)
    vr = VectorRetriever()
    assert vr.build_index([dict(n) for n in notes], save_index=False) is True
    rebuilds = []
    orig_build = vr.build_index
    monkeypatch.setattr(vr, "build_index", lambda *a, **k: (rebuilds.append(k.get("force_rebuild")), orig_build(*a, **k))[1])
    assert vr.remove_notes(["n3"]) is True and rebuilds == [True]
    assert vr.update_note("n4", dict(notes[4], content=words[21])) is True and rebuilds == [True, True]
    assert len(vr.atomic_notes) == 19 and vr.vector_index.index.ntotal == 19
    vr.cleanup()
    EmbeddingManager._reset_singleton()
