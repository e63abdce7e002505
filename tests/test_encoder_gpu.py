"""GPU parity: the HIP sentence encoder (anr_encoder_*, f16 MFMA operands and activations / f32 accumulate / f32 LayerNorm arithmetic)
against the float32 CPU oracle (transformers forward through the sentence-transformers pipeline) on seeded
random weights of the reference's model shapes.  Tolerance (f16 operands): cosine >= 0.9995 and max abs
difference of the unit-norm embeddings <= 5e-3; the pooled (un-normalised) output within 2 % relative.

On top of that constant bar, the derived one of tests/test_encoder_attention_gpu.py (``_bar``: distance from the float64
transformers forward at most 4 x the f16 emulation's distance, unit-norm and un-normalised, per sentence and per element)
in every test whose two extra CPU forwards in double are small.  Left on the constant bar alone: the two 24-layer XLM-R
large shapes and C4 (12 layers x 256 prefixed queries), whose float64 + emulated CPU forwards are several TFLOP each in
double — minutes per test on 16 threads; test_folded_first_layernorm_equals_the_separate_pass (three 4-layer 768-wide models x 16 K
tokens: the same cost; the fold modes are held to the derived bar by test_fold_modes_on_a_sharp_768_wide_model on 4 K
tokens); and test_concurrent_single_query_encodes_share_forwards, which compares device results with each other."""
import os

import numpy as np
import pytest

import encoder_cases as ec
from oracle import encoder as oenc

pytestmark = pytest.mark.gpu


def _bar(label, d, sents, enc, got, got_raw=None, tokens=None):
    """the derived bar (oracle.encoder.parity_bar <= BAR_FACTOR) for device embeddings of ``sents`` (or of the token batch
    ``tokens`` = (ids, lens)); got_raw None: the un-normalised output is taken from ``enc.encode``"""
    if got_raw is None:
        was = enc._info["normalize_module"]
        enc._info["normalize_module"] = False
        got_raw = enc.encode(sents, batch_size=16, normalize_embeddings=False)
        enc._info["normalize_module"] = was
    ids, lens = tokens if tokens is not None else oenc.tokenize(d, sents)
    ref, ref_raw, emul, emul_raw = ec.references(d, ids, lens, batch_size=64)
    bar = oenc.parity_bar(got, got_raw, emul, emul_raw, ref, ref_raw)
    print(f"RATIO {label}: e_gpu/e_emul l2 {bar['l2']:.2f} l2_raw {bar['l2_raw']:.2f} elem {bar['elem']:.2f} "
          f"elem_raw {bar['elem_raw']:.2f} (e_emul {bar['e_emul']:.2e}, e_gpu {bar['e_gpu']:.2e})")
    assert bar["worst"] <= oenc.BAR_FACTOR, (label, bar)


def _check(tmp_path, sentences=None, n=48, derived_bar=True, **shape):
    from anorag_hip.encoder import SentenceEncoder
    d = oenc.make_synthetic_model(str(tmp_path / "model"), **shape)
    sents = sentences or oenc.synthetic_sentences(d, n)
    ref = oenc.encode(d, sents, batch_size=16, normalize=True)
    enc = SentenceEncoder(d)
    got = enc.encode(sents, batch_size=16, normalize_embeddings=True)
    assert got.shape == ref.shape and got.dtype == np.float32
    cos = np.sum(got * ref, axis=1)
    assert cos.min() >= 0.9995, cos.min()
    assert np.max(np.abs(got - ref)) <= 5e-3
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    if derived_bar:
        _bar(f"{shape}", d, sents, enc, got)
    enc.close()
    return got, ref


def test_minilm_shape_mean_pooling(tmp_path):
    """all-MiniLM-L6-v2 shape: 6 layers, H 384, 12 heads (d_h 32), I 1536, mean pooling."""
    _check(tmp_path, layers=6, hidden=384, heads=12, intermediate=1536, pooling="mean")


def test_bge_base_shape_cls_pooling(tmp_path):
    """bge-base-en shape (reduced depth for test time): H 768, 12 heads (d_h 64), I 3072, CLS pooling."""
    _check(tmp_path, n=24, layers=3, hidden=768, heads=12, intermediate=3072, pooling="cls")


def test_long_and_ragged_sequences(tmp_path):
    """truncation at max_seq_length, several key blocks, batch with very different lengths, empty text."""
    d = oenc.make_synthetic_model(str(tmp_path / "m0"), layers=2, hidden=128, heads=4, intermediate=512, max_pos=128)
    base = oenc.synthetic_sentences(d, 6, seed=3, min_words=1, max_words=5)
    long = oenc.synthetic_sentences(d, 3, seed=4, min_words=150, max_words=200)   # > 128 tokens -> truncated
    sents = base + long + ["a"]
    from anorag_hip.encoder import SentenceEncoder
    ref = oenc.encode(d, sents, batch_size=4, normalize=True)
    enc = SentenceEncoder(d)
    got = enc.encode(sents, batch_size=4, normalize_embeddings=True)
    assert np.sum(got * ref, axis=1).min() >= 0.9995
    # un-normalised output
    ref_raw = oenc.encode(d, sents, batch_size=4, normalize=False)
    enc._info["normalize_module"] = False
    got_raw = enc.encode(sents, batch_size=4, normalize_embeddings=False)
    rel = np.linalg.norm(got_raw - ref_raw, axis=1) / np.linalg.norm(ref_raw, axis=1)
    assert rel.max() <= 0.02, rel.max()
    single = enc.encode(sents[0], normalize_embeddings=False)
    assert single.shape == (128,)
    _bar("long and ragged, H 128", d, sents, enc, got, got_raw)
    enc.close()


def test_xlm_roberta_position_offset(tmp_path):
    """bge-m3 family (XLM-R): position ids start at padding_idx + 1, one token type."""
    _check(tmp_path, n=16, layers=2, hidden=256, heads=4, intermediate=1024, pooling="cls", model_type="xlm-roberta",
           max_pos=128)


def test_mpnet_relative_position_bias(tmp_path):
    """all-mpnet-base-v2 family (the reference's second fallback model, embedding_manager.py:218-219): bucketed
    relative position bias added to the attention scores in every layer, no token types, positions from
    padding_idx + 1; mean pooling.  Sequences longer than one 32-key block exercise far buckets."""
    d = oenc.make_synthetic_model(str(tmp_path / "mp"), layers=3, hidden=256, heads=8, intermediate=1024, pooling="mean",
                                  model_type="mpnet", max_pos=256, rel_bias_std=1.5)
    sents = (oenc.synthetic_sentences(d, 12, seed=5, min_words=2, max_words=12)
             + oenc.synthetic_sentences(d, 6, seed=6, min_words=60, max_words=140))
    from anorag_hip.encoder import SentenceEncoder
    ref = oenc.encode(d, sents, batch_size=6, normalize=True)
    enc = SentenceEncoder(d)
    got = enc.encode(sents, batch_size=6, normalize_embeddings=True)
    cos = np.sum(got * ref, axis=1)
    assert cos.min() >= 0.9995, cos.min()
    assert np.max(np.abs(got - ref)) <= 5e-3
    _bar("mpnet 3 layers, bias table std 1.5", d, sents, enc, got)
    enc.close()


def test_large_batch_takes_the_tiled_gemm_paths(tmp_path):
    """> 5120 tokens in one forward: the 256 x 256 / 256 x 192 LDS-staged GEMM tiles instead of the skinny kernel,
    here with a hidden size whose K depth is not a multiple of 3 k-steps (the two-k-step ring, as for H = 1024 /
    bge-m3), ragged sentence lengths, token and feature tails that do not fill a tile"""
    d = oenc.make_synthetic_model(str(tmp_path / "m"), layers=2, hidden=256, heads=4, intermediate=1024, pooling="mean")
    sents = oenc.synthetic_sentences(d, 230, seed=9, min_words=10, max_words=34)
    from anorag_hip.encoder import SentenceEncoder
    ref = oenc.encode(d, sents, batch_size=230, normalize=True)
    enc = SentenceEncoder(d)
    ids, lens, _ = enc.tokenize(sents)
    assert ids.shape[0] * ((ids.shape[1] + 31) // 32 * 32) > 5120 + 512     # really past the skinny kernel's range
    got = enc.encode(sents, batch_size=230, normalize_embeddings=True)
    cos = np.sum(got * ref, axis=1)
    assert cos.min() >= 0.9995, cos.min()
    assert np.max(np.abs(got - ref)) <= 5e-3
    _bar("large batch, tiled GEMMs", d, sents, enc, got)
    enc.close()


def test_c4_full_shape_bge_base_12_layers_batch256_encode_then_search_1m(tmp_path):
    """BASELINE.json config C4 at its real shape: bge-base-en (12 layers, H 768, 12 heads, I 3072, vocab 30522, CLS
    pooling + normalise, seeded weights), ONE batch of 256 query strings (8-24 words + the bge query prefix,
    SURVEY.md §8d), then top-100 over a 1 M x 768 corpus.  (a) every embedding against the float32 CPU oracle;
    (b) the search of those embeddings against the flat-index oracle run on the SAME embeddings (north_star:
    "results match the reference CPU path on the same embeddings"); (c) the two legs end to end: ids found from the
    device embeddings vs ids found from the oracle's embeddings (f16 MFMA operands move scores by ~1e-3, so this
    is a recall figure, not an identity)."""
    import torch
    from anorag_hip import FlatIndex, METRIC_IP
    from anorag_hip.encoder import SentenceEncoder
    from oracle import flat_index as orc
    d = oenc.make_synthetic_model(str(tmp_path / "bge"), layers=12, hidden=768, heads=12, intermediate=3072,
                                  vocab=30522, pooling="cls", weight_std=0.02)
    prefix = "Represent this sentence for searching relevant passages: "  # embedding_manager.py:551-564
    sents = [prefix + s for s in oenc.synthetic_sentences(d, 256, seed=7, min_words=8, max_words=24)]
    ref = oenc.encode(d, sents, batch_size=256, normalize=True)
    enc = SentenceEncoder(d)
    got = enc.encode(sents, batch_size=256, normalize_embeddings=True)
    cos = np.sum(got * ref, axis=1)
    assert got.shape == (256, 768) and cos.min() >= 0.9995, cos.min()
    assert np.max(np.abs(got - ref)) <= 5e-3
    enc.close()

    dev = torch.device("cuda", 0)
    n, k = 1_000_000, 100
    idx = FlatIndex(768, METRIC_IP, normalize=True)
    idx.reserve(n)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    blocks = []
    for s in range(0, n, 250_000):
        xb = torch.randn((250_000, 768), generator=g, device=dev)
        torch.cuda.synchronize()
        idx.add_device(xb.data_ptr(), xb.shape[0])
        blocks.append(orc.preprocess_vectors(xb.cpu().numpy()))
    D, I = idx.search(got, k)                       # 4 batches of 64
    top = orc.BlockedTopK(orc.preprocess_vectors(got), k + 16, "ip")
    top_ref = orc.BlockedTopK(orc.preprocess_vectors(ref), k, "ip")
    for bi, xb in enumerate(blocks):
        top.push(xb, bi * 250_000)
        top_ref.push(xb, bi * 250_000)
    S, Ir = top.result()
    assert np.array_equal(I, Ir[:, :k]) or all(
        set(I[r]) ^ set(Ir[r, :k]) <= {i for i, s in zip(Ir[r], S[r]) if abs(s - S[r, k - 1]) <= 1e-6} for r in range(256))
    assert np.max(np.abs(D - S[:, :k].astype(np.float32))) <= 1e-4
    _, I_ref_emb = top_ref.result()
    recall = np.mean([len(set(I[r]) & set(I_ref_emb[r])) / k for r in range(256)])
    print(f"C4 end to end: recall@100 of the device-embedding search vs the oracle-embedding search = {recall:.4f}, "
          f"min cosine {cos.min():.7f}")
    assert recall >= 0.99, recall   # measured 0.9976 (round 3)
    idx.close()


@pytest.mark.parametrize("words,model_type,heads", [((3, 12), "bert", 4), ((20, 40), "bert", 4), ((60, 100), "bert", 4),
                                                    ((20, 40), "mpnet", 4), ((20, 40), "xlm-roberta", 2)])
def test_fused_projection_attention_kernel(tmp_path, words, model_type, heads):
    """k_qkv_attn (Q/K/V projection + attention in one kernel: 64-wide heads, sequences padded to 32 / 64 / 128 tokens,
    >= 4096 padded tokens in the forward): ragged lengths (masking inside the tile), a last tile that is not full (the
    token-block count is not a multiple of 8), MPNet's relative position bias, XLM-R positions; same bar as every other
    encoder test.  The sentence-length ranges put the padded length at 32, 64 and 128."""
    from anorag_hip.encoder import SentenceEncoder
    d = oenc.make_synthetic_model(str(tmp_path / "m"), layers=2, hidden=64 * heads, heads=heads, intermediate=256 * heads,
                                  pooling="mean", model_type=model_type, max_pos=128)
    n = 250 if words[1] <= 12 else (141 if words[1] <= 40 else 70)
    sents = oenc.synthetic_sentences(d, n, seed=11, min_words=words[0], max_words=words[1]) + ["a"]
    ref = oenc.encode(d, sents, batch_size=len(sents), normalize=True)
    enc = SentenceEncoder(d)
    ids, lens, _ = enc.tokenize(sents)
    Lp = (ids.shape[1] + 31) // 32 * 32
    assert Lp in (32, 64, 128) and ids.shape[0] * Lp >= 4096 and (ids.shape[0] * Lp // 32) % 8 != 0, (ids.shape, Lp)
    # ONE forward of the whole tokenised batch (encode() would cut the ragged batch into several smaller forwards)
    use_types = enc._info["hf"].get("type_vocab_size", 1) > 1
    got = enc._enc.forward(ids, lens, np.zeros_like(ids) if use_types else None, normalize=True)
    cos = np.sum(got * ref, axis=1)
    assert cos.min() >= 0.9995, cos.min()
    assert np.max(np.abs(got - ref)) <= 5e-3
    got_raw = enc._enc.forward(ids, lens, np.zeros_like(ids) if use_types else None, normalize=False)
    _bar(f"k_qkv_attn {model_type} words {words}", d, sents, enc, got, got_raw, tokens=(ids, lens))
    enc.close()


def test_outlier_features_bge_base_12_layers(tmp_path):
    """The f16 activation / residual stream under OUTLIER FEATURES (trained BERT-family checkpoints carry a few hidden
    dimensions whose LayerNorm gains are tens of times the rest: activations in the tens to hundreds, where f16 resolves
    0.03-0.06): 6 dimensions with gain x 21-39 in every LayerNorm and in the word embeddings, full 12-layer bge-base
    shape.  Same bar as the benign-weight tests."""
    from anorag_hip.encoder import SentenceEncoder
    d = oenc.make_synthetic_model(str(tmp_path / "model"), layers=12, hidden=768, heads=12, intermediate=3072, pooling="cls",
                                  weight_std=0.02, outlier_dims=6, outlier_gain=30.0)
    sents = oenc.synthetic_sentences(d, 40)
    ref = oenc.encode(d, sents, batch_size=16, normalize=True)
    enc = SentenceEncoder(d)
    got = enc.encode(sents, batch_size=16, normalize_embeddings=True)
    cos = np.sum(got * ref, axis=1)
    print(f"outlier features, bge-base 12 layers: min cosine {cos.min():.7f}, max |diff| {np.max(np.abs(got - ref)):.2e}")
    assert cos.min() >= 0.9995, cos.min()
    assert np.max(np.abs(got - ref)) <= 5e-3
    # the outlier dimensions really carry large activations: the un-normalised CLS output on them is >> the rest
    enc._info["normalize_module"] = False
    raw = enc.encode(sents, batch_size=16, normalize_embeddings=False)
    mag = np.sort(np.abs(raw).max(axis=0))   # (measured: 722, 625, 294, 20, 15 ... median 0.31)
    assert mag[-3] >= 100 * np.median(mag) and mag[-1] >= 100.0, (mag[-6:], np.median(mag))
    _bar("outlier features, bge-base 12 layers", d, sents, enc, got, raw)
    enc.close()


def test_outlier_features_xlm_roberta_large_24_layers(tmp_path):
    """the same stress at the bge-m3 shape (XLM-R large: 24 layers, H 1024, 16 heads, I 4096)"""
    _check(tmp_path, n=32, layers=24, hidden=1024, heads=16, intermediate=4096, pooling="cls", model_type="xlm-roberta",
           max_pos=512, weight_std=0.02, outlier_dims=5, outlier_gain=30.0, derived_bar=False)


def test_xlm_roberta_large_shape_24_layers(tmp_path):
    """bge-m3 (the reference's default model, embedding_manager.py:82): XLM-R large shape — 24 layers, H 1024,
    16 heads, I 4096 — full depth, one forward of 48 ragged sentences (small vocabulary: the table size does not
    change the arithmetic)."""
    _check(tmp_path, n=48, layers=24, hidden=1024, heads=16, intermediate=4096, pooling="cls",
           model_type="xlm-roberta", max_pos=512, weight_std=0.02, derived_bar=False)


def test_concurrent_single_query_encodes_share_forwards(tmp_path):
    """The reference's query-time pattern: worker threads that share ONE model and encode a question each
    (main_musique.py:487-494, query/query_processor.py:2761-2766).  Eight threads calling
    EmbeddingManager.encode_queries([q]) must get exactly the one-at-a-time embeddings (the combining queue only merges
    requests whose per-sequence arithmetic is unchanged) at several times the serial throughput.  The queue lives in the
    library (anr_encoder_forward_shared, csrc/combine.hpp, two lanes): measured 3.4-4.3x over seven runs on three boxes
    (0.18-0.22 ms per question against 0.64-0.79 one at a time; VERDICT r3 asked for 4x).  What bounds it is not the
    device: the same queue driven with pre-tokenised queries (tools/shared_forward_perf.py, one ctypes call per question)
    gives 3.6x at 8 threads and 6.3x at 16 — a caller is served by every other forward of its lane, because it comes back
    after the next one has started — and through EmbeddingManager each question also holds the interpreter lock for
    ~0.1 ms of tokenisation and array handling that no other thread can overlap."""
    import threading
    import time
    from anorag_hip import compat
    from vector_store import EmbeddingManager
    md = oenc.make_synthetic_model(str(tmp_path / "bge-base-synth"), layers=12, hidden=768, heads=12, intermediate=3072,
                                   vocab=30522, max_pos=512, pooling="cls", weight_std=0.03)
    cfg = compat.config
    cfg.reset()
    cfg.set("embedding.model_path", md)
    cfg.set("embedding.max_length", 512)
    EmbeddingManager._reset_singleton()
    em = EmbeddingManager()
    qs = oenc.synthetic_sentences(md, 480, seed=9, min_words=6, max_words=18)
    for q in qs[:80]:
        em.encode_queries([q])
    t0 = time.perf_counter()
    serial = [em.encode_queries([q]) for q in qs]
    t_serial = time.perf_counter() - t0
    got = [None] * len(qs)

    def worker(w):
        for j in range(w, len(qs), 8):
            got[j] = em.encode_queries([qs[j]])

    best = None
    for rep in range(3):
        th = [threading.Thread(target=worker, args=(w,)) for w in range(8)]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        for a, b in zip(got, serial):
            assert a.shape == b.shape == (1, 768) and np.array_equal(a, b)       # bit-identical to the one-at-a-time call
    forwards, served = em.model._enc.shared_stats()
    print(f"serial {1e3 * t_serial / len(qs):.3f} ms per query, 8 threads {1e3 * best / len(qs):.3f} ms per query "
          f"({t_serial / best:.1f}x), {served / max(1, forwards):.1f} queries per forward over the whole test")
    assert served == 80 + 4 * len(qs) and forwards < served
    assert t_serial / best >= 3.0, (t_serial, best)
    EmbeddingManager._reset_singleton()
    cfg.reset()


def test_folded_first_layernorm_equals_the_separate_pass(tmp_path, monkeypatch):
    """Large forwards fold a layer's first LayerNorm into the GEMMs around it (EPI_RES_STATS / EPI_FOLD_GELU / EPI_RES_LN in
    csrc/encoder.hip): same embeddings as the path with the LayerNorm pass (ANORAG_ENC_FOLD=0) to well inside the
    encoder's tolerance, and both against the float32 oracle — plain weights, LayerNorm gains / shifts far from 1 / 0 (the
    fold multiplies them into the weights), and outlier features."""
    from anorag_hip.encoder import SentenceEncoder
    for case in ("plain", "gains", "outliers"):
        d = oenc.make_synthetic_model(str(tmp_path / f"bge-{case}"), layers=4, hidden=768, heads=12, intermediate=3072,
                                      vocab=30522, pooling="cls", weight_std=0.03)
        if case != "plain":
            from safetensors.numpy import load_file, save_file
            path = os.path.join(d, "model.safetensors")
            t = load_file(path)
            rng = np.random.default_rng(5)
            for name in list(t):
                if "attention.output.LayerNorm.weight" in name:
                    g = (1.0 + 0.5 * rng.standard_normal(768)).astype(np.float32)
                    if case == "outliers":
                        g[rng.choice(768, 6, replace=False)] *= 25.0
                    t[name] = g
                elif "attention.output.LayerNorm.bias" in name:
                    t[name] = (0.3 * rng.standard_normal(768)).astype(np.float32)
            save_file(t, path)
        sents = oenc.synthetic_sentences(d, 256, seed=3, min_words=20, max_words=44)   # 256 x 64 padded tokens: the tile kernels
        ref = oenc.encode(d, sents, batch_size=256, normalize=True)
        outs = []
        for fold in ("1", "0", "2"):     # 2: residual sums formed in the projections' epilogues (EPI_RES), LayerNorm passes kept
            monkeypatch.setenv("ANORAG_ENC_FOLD", fold)
            enc = SentenceEncoder(d)
            outs.append(enc.encode(sents, batch_size=256, normalize_embeddings=True))
            enc.close()
        for got in outs:
            assert np.sum(got * ref, axis=1).min() >= 0.9995 and np.max(np.abs(got - ref)) <= 5e-3, case
        assert not np.array_equal(outs[0], outs[1]), "the two paths are different arithmetic: identical bits mean the fold did not run"
        assert np.sum(outs[0] * outs[1], axis=1).min() >= 0.99999 and np.max(np.abs(outs[0] - outs[1])) <= 1.5e-3, case
        assert not np.array_equal(outs[2], outs[1])
        assert np.sum(outs[2] * outs[1], axis=1).min() >= 0.99999 and np.max(np.abs(outs[2] - outs[1])) <= 1.5e-3, case
