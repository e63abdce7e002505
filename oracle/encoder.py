"""ORACLE — test infrastructure only (never imported by the product path).

CPU restatement of what the reference gets from ``self.model.encode(...)`` (vector_store/embedding_manager.py:
392-399).  The arithmetic lives in third-party code that is not vendored in the reference and not installed
here: sentence-transformers (>= 2.2.0, requirements.txt:15) on top of transformers / torch.  Restated from
its published pipeline: texts sorted by length (longest first) -> batches -> HF
tokenizer (padding to the longest, truncation to max_seq_length) -> ``AutoModel`` forward (here
``transformers.BertModel`` / ``XLMRobertaModel`` / ``MPNetModel`` in float32 on the CPU, which IS the code sentence-transformers
calls) -> Pooling (masked mean: ``sum(h * mask) / clamp(sum(mask), 1e-9)``, or CLS) -> ``F.normalize(p=2, dim=1)``.

PARITY UNPINNED for real checkpoints: no model weights / vocab exist in the container and the reference has no
test or golden vector for this call; parity is checked on seeded random weights of the
reference's model shapes with a synthetic WordPiece vocabulary.
"""
from __future__ import annotations

import json
import os
from typing import List

import numpy as np


def make_synthetic_model(path: str, *, layers=6, hidden=384, heads=12, intermediate=1536, vocab=2048, max_pos=512,
                         pooling="mean", seed=0, weight_std=0.05, model_type="bert", outlier_dims=0,
                         outlier_gain=30.0, attn_gain=1.0, rel_bias_std=None) -> str:
    """Write an HF/sentence-transformers style model directory with seeded random weights.
    outlier_dims > 0: that many hidden dimensions carry OUTLIER FEATURES, as trained BERT-family checkpoints do — every
    LayerNorm's gain on them is multiplied by outlier_gain (x 20-40) and the word-embedding columns likewise, so their
    activations reach the tens to hundreds while the rest stay O(1) (the stress case for an f16 residual stream).
    attn_gain != 1: the query and key projections (weights and biases) are multiplied by it, so the scaled attention logits
    grow by its square — with weight_std 0.02-0.05 they have std ~0.3 and every softmax is near-uniform; trained checkpoints
    have sharp heads (``attention_logit_stats`` reports the std).  rel_bias_std (MPNet): the relative position bias table is
    drawn again with that std (initializer_range gives it 0.05: a logit moves by 0.05).  The defaults write the files the
    function wrote before these two arguments existed."""
    import torch
    from transformers import BertConfig, BertModel, MPNetConfig, MPNetModel, XLMRobertaConfig, XLMRobertaModel

    os.makedirs(path, exist_ok=True)
    torch.manual_seed(seed)
    words = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    rng = np.random.default_rng(seed)
    alphabet = "abcdefghijklmnopqrstuvwxyz"
    seen = set(words)
    while len(words) < vocab:
        w = "".join(rng.choice(list(alphabet), size=rng.integers(1, 7)))
        if rng.random() < 0.3:
            w = "##" + w
        if w not in seen:
            seen.add(w)
            words.append(w)
    with open(os.path.join(path, "vocab.txt"), "w") as f:
        f.write("\n".join(words) + "\n")
    if model_type == "bert":
        cfg = BertConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads,
                         intermediate_size=intermediate, max_position_embeddings=max_pos, type_vocab_size=2,
                         initializer_range=weight_std, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        model = BertModel(cfg, add_pooling_layer=False)
    elif model_type == "mpnet":  # all-mpnet-base-v2 family: relative position bias shared by all layers
        cfg = MPNetConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads,
                          intermediate_size=intermediate, max_position_embeddings=max_pos + 2, pad_token_id=1,
                          relative_attention_num_buckets=32, initializer_range=weight_std, hidden_dropout_prob=0.0,
                          attention_probs_dropout_prob=0.0)
        model = MPNetModel(cfg, add_pooling_layer=False)
    else:
        cfg = XLMRobertaConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers,
                               num_attention_heads=heads, intermediate_size=intermediate,
                               max_position_embeddings=max_pos + 2, type_vocab_size=1, pad_token_id=1,
                               initializer_range=weight_std, hidden_dropout_prob=0.0,
                               attention_probs_dropout_prob=0.0)
        model = XLMRobertaModel(cfg, add_pooling_layer=False)
    with torch.no_grad():  # non-trivial LayerNorm parameters and biases
        for n, p in model.named_parameters():
            if "LayerNorm.weight" in n:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            elif n.endswith("bias"):
                p.copy_(0.05 * torch.randn_like(p))
        if outlier_dims:
            dims = torch.tensor(np.random.default_rng(seed + 1).choice(hidden, size=int(outlier_dims), replace=False))
            gains = torch.tensor(np.random.default_rng(seed + 2).uniform(0.7, 1.3, int(outlier_dims)) * outlier_gain,
                                 dtype=torch.float32)
            for n, p in model.named_parameters():
                if "LayerNorm.weight" in n:
                    p[dims] *= gains
                elif n.endswith("word_embeddings.weight"):
                    p[:, dims] *= gains
        if attn_gain != 1.0:
            for n, p in model.named_parameters():
                if any(t in n for t in ("attention.self.query.", "attention.self.key.", "attention.attn.q.", "attention.attn.k.")):
                    p.mul_(float(attn_gain))
        if rel_bias_std is not None:
            g = torch.Generator().manual_seed(seed + 3)  # its own stream: nothing else moves
            w = model.encoder.relative_attention_bias.weight
            w.copy_(float(rel_bias_std) * torch.randn(w.shape, generator=g))
    model.eval()
    model.save_pretrained(path, safe_serialization=True)
    with open(os.path.join(path, "tokenizer_config.json"), "w") as f:
        json.dump({"do_lower_case": True}, f)
    with open(os.path.join(path, "modules.json"), "w") as f:
        json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                   {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
                   {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}], f)
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    with open(os.path.join(path, "1_Pooling", "config.json"), "w") as f:
        json.dump({"word_embedding_dimension": hidden, "pooling_mode_cls_token": pooling == "cls",
                   "pooling_mode_mean_tokens": pooling == "mean", "pooling_mode_max_tokens": False}, f)
    with open(os.path.join(path, "sentence_bert_config.json"), "w") as f:
        json.dump({"max_seq_length": max_pos, "do_lower_case": True}, f)
    return path


def _load_hf(model_dir: str, dtype):
    import torch
    from transformers import AutoModel
    with open(os.path.join(model_dir, "1_Pooling", "config.json")) as f:
        cls_pool = json.load(f).get("pooling_mode_cls_token", False)
    with open(os.path.join(model_dir, "config.json")) as f:
        hf = json.load(f)
    model = AutoModel.from_pretrained(model_dir, add_pooling_layer=False).eval().to(dtype or torch.float32)
    return model, hf, cls_pool


def _hf_forward(model, hf, cls_pool, ids, mask, types, normalize):
    import torch
    kw = {"token_type_ids": types} if hf.get("type_vocab_size", 1) > 1 else {}
    with torch.no_grad():
        h = model(input_ids=ids, attention_mask=mask, **kw).last_hidden_state
    if cls_pool:
        emb = h[:, 0]
    else:
        m = mask.unsqueeze(-1).to(h.dtype)
        emb = (h * m).sum(1) / torch.clamp(m.sum(1), min=1e-9)
    if normalize == "both":
        return torch.nn.functional.normalize(emb, p=2, dim=1).numpy(), emb.numpy()
    if normalize:
        emb = torch.nn.functional.normalize(emb, p=2, dim=1)
    return emb.numpy()


def encode(model_dir: str, sentences: List[str], batch_size=32, normalize=True, max_seq_length=None, dtype=None) -> np.ndarray:
    """CPU forward of the model directory through the sentence-transformers pipeline: float32 (the default, float32
    result) or, with dtype=torch.float64, the same transformers forward in double (float64 result)."""
    import torch
    from tokenizers import BertWordPieceTokenizer

    model, hf, cls_pool = _load_hf(model_dir, dtype)
    tok = BertWordPieceTokenizer(os.path.join(model_dir, "vocab.txt"), lowercase=True)
    max_len = max_seq_length or hf["max_position_embeddings"] - (0 if hf["model_type"] == "bert" else 2)
    tok.enable_truncation(max_length=max_len)
    pad = hf.get("pad_token_id", 0) or 0
    out = np.zeros((len(sentences), hf["hidden_size"]), dtype=np.float64 if dtype == torch.float64 else np.float32)
    order = np.argsort([-len(s) for s in sentences], kind="stable")
    for s in range(0, len(sentences), batch_size):
        sel = order[s:s + batch_size]
        encs = tok.encode_batch([sentences[i] for i in sel])
        L = max(len(e.ids) for e in encs)
        ids = torch.full((len(encs), L), pad, dtype=torch.long)
        mask = torch.zeros((len(encs), L), dtype=torch.long)
        types = torch.zeros((len(encs), L), dtype=torch.long)
        for i, e in enumerate(encs):
            ids[i, :len(e.ids)] = torch.tensor(e.ids)
            mask[i, :len(e.ids)] = 1
            types[i, :len(e.ids)] = torch.tensor(e.type_ids)
        out[sel] = _hf_forward(model, hf, cls_pool, ids, mask, types, normalize)
    return out


def tokenize(model_dir: str, sentences: List[str], max_seq_length=None):
    """(ids [n, L] int32 padded with the model's pad id, lengths [n] int32) of the sentences, in the given order: the token
    batch ``encode`` would feed the model if all sentences shared one batch."""
    from tokenizers import BertWordPieceTokenizer
    with open(os.path.join(model_dir, "config.json")) as f:
        hf = json.load(f)
    tok = BertWordPieceTokenizer(os.path.join(model_dir, "vocab.txt"), lowercase=True)
    tok.enable_truncation(max_length=max_seq_length or hf["max_position_embeddings"] - (0 if hf["model_type"] == "bert" else 2))
    encs = tok.encode_batch(list(sentences))
    lens = np.array([len(e.ids) for e in encs], dtype=np.int32)
    ids = np.full((len(encs), int(lens.max())), hf.get("pad_token_id", 0) or 0, dtype=np.int32)
    for i, e in enumerate(encs):
        ids[i, :lens[i]] = e.ids
    return ids, lens


def encode_tokens(model_dir: str, ids, lens, normalize=True, dtype=None, batch_size=None) -> np.ndarray:
    """The transformers forward of ``encode`` on a token batch given directly (ids [n, L], lengths [n]; positions past a
    length are padding and must hold the model's pad id, positions inside one must not — XLM-R and MPNet count positions
    over non-pad ids).  batch_size: rows per forward (None: all in one); the result does not depend on it beyond rounding."""
    import torch
    model, hf, cls_pool = _load_hf(model_dir, dtype)
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.long)
    lens_t = torch.as_tensor(np.asarray(lens), dtype=torch.long)
    n = ids.shape[0]
    outs = []
    for s in range(0, n, batch_size or n):
        sl = slice(s, s + (batch_size or n))
        L = int(lens_t[sl].max())
        mask = (torch.arange(L)[None, :] < lens_t[sl, None]).to(torch.long)
        outs.append(_hf_forward(model, hf, cls_pool, ids[sl, :L], mask, torch.zeros_like(ids[sl, :L]), normalize))
    if normalize == "both":     # (unit-norm, un-normalised) of one pass
        return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])
    return np.concatenate(outs)


# ---- the forward written out: the kernels' intended f16 rounding, and wrong forwards for the mutant tests ----------------

MUTANTS = ("bias_zero", "bias_reversed", "bias_rolled", "bias_query_minus_key", "scale_1.1", "unmasked_pad_key",
           "pos_offset_1", "tanh_gelu", "mean_over_padded_length")


def _tensors(model_dir, dtype):
    import torch
    from safetensors.torch import load_file
    raw = load_file(os.path.join(model_dir, "model.safetensors"))
    t = {}
    for k, v in raw.items():
        k = k.replace("attention.self.query", "q").replace("attention.self.key", "k").replace("attention.self.value", "v")
        k = k.replace("attention.attn.q", "q").replace("attention.attn.k", "k").replace("attention.attn.v", "v")
        k = k.replace("attention.attn.o", "o").replace("attention.output.dense", "o")
        k = k.replace("attention.output.LayerNorm", "ln1").replace("attention.LayerNorm", "ln1")
        k = k.replace("intermediate.dense", "ffn1").replace("output.dense", "ffn2").replace("output.LayerNorm", "ln2")
        t[k] = v.to(dtype)
    return t


def _relative_buckets(L: int, num_buckets=32, max_distance=128):
    """bucket[query][key] of transformers' MPNetEncoder.relative_position_bucket (relative position = key - query)"""
    import math
    import torch
    pos = torch.arange(L, dtype=torch.long)
    n = -(pos[None, :] - pos[:, None])
    half = num_buckets // 2
    ret = (n < 0).to(torch.long) * half
    n = torch.abs(n)
    max_exact = half // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (half - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, half - 1))
    return ret + torch.where(n < max_exact, n, large)


def forward_tokens(model_dir: str, ids, lens, normalize=True, dtype=None, f16=False, mutant=None, stats=None,
                   batch_size=None) -> np.ndarray:
    """The same forward as ``encode_tokens`` written out in torch from the safetensors file (BERT / XLM-R / MPNet post-LN
    blocks, masked softmax, erf-GELU, masked-mean or CLS pooling), float64 by default.  With f16 False and no mutant it
    equals the transformers forward to rounding (tests/test_encoder_mutants_cpu.py holds it to 1e-6 in float64).
    f16=True — see ``encode_f16_emulated``.  mutant: one of MUTANTS, a deliberately wrong forward.  stats: a dict that
    normalize="both": the pair (unit-norm embeddings, un-normalised pooled outputs) of one pass.  The dict receives, from layer 0, ``logit_std`` (std of the scaled logits + bias over real query / key pairs) and
    ``argmax_key_block`` ([rows] 32-key block that holds each real query's largest logit, heads concatenated) with
    ``key_blocks`` (blocks its sequence has)."""
    import torch
    dtype = dtype or torch.float64
    assert mutant is None or mutant in MUTANTS, mutant
    with open(os.path.join(model_dir, "config.json")) as f:
        hf = json.load(f)
    with open(os.path.join(model_dir, "1_Pooling", "config.json")) as f:
        cls_pool = json.load(f).get("pooling_mode_cls_token", False)
    t = _tensors(model_dir, dtype)
    H, heads, eps = hf["hidden_size"], hf["num_attention_heads"], hf.get("layer_norm_eps", 1e-12)
    dh = H // heads
    pos_offset = 0 if hf["model_type"] == "bert" else int(hf.get("pad_token_id", 1)) + 1
    if mutant == "pos_offset_1":
        pos_offset = 1
    r = (lambda x: x.to(torch.float16).to(dtype)) if f16 else (lambda x: x)
    ln = lambda x, p: torch.nn.functional.layer_norm(x, (H,), t[p + ".weight"], t[p + ".bias"], eps)  # noqa: E731
    lin = lambda x, p: x @ r(t[p + ".weight"]).T + t[p + ".bias"]                                      # noqa: E731
    table = t.get("encoder.relative_attention_bias.weight")       # [buckets][heads]
    if table is not None:
        if mutant == "bias_zero":
            table = torch.zeros_like(table)
        elif mutant == "bias_reversed":
            table = table.flip(0)
        elif mutant == "bias_rolled":
            table = table.roll(1, 0)
    scale = (1.1 if mutant == "scale_1.1" else 1.0) / float(np.sqrt(dh))
    ids_all = torch.as_tensor(np.asarray(ids), dtype=torch.long)
    lens_all = torch.as_tensor(np.asarray(lens), dtype=torch.long)
    n = ids_all.shape[0]
    outs = []
    for s0 in range(0, n, batch_size or n):
        lens_t = lens_all[s0:s0 + (batch_size or n)]
        L = int(lens_t.max())
        idb = ids_all[s0:s0 + (batch_size or n), :L]
        B = idb.shape[0]
        real = torch.arange(L)[None, :] < lens_t[:, None]                       # [B][L]
        keymask = real.clone()
        if mutant == "unmasked_pad_key":                                        # one padding key of the shortest sentence
            b = int(torch.argmin(lens_t))
            assert int(lens_t[b]) < L, "the mutant needs a sentence shorter than its batch"
            keymask[b, int(lens_t[b])] = True
        x = t["embeddings.word_embeddings.weight"][idb] + t["embeddings.position_embeddings.weight"][pos_offset + torch.arange(L)]
        if "embeddings.token_type_embeddings.weight" in t:
            x = x + t["embeddings.token_type_embeddings.weight"][0]
        x = r(ln(x, "embeddings.LayerNorm"))
        bias = None
        if table is not None:
            bk = _relative_buckets(L, hf.get("relative_attention_num_buckets", 32))
            if mutant == "bias_query_minus_key":
                bk = bk.T
            bias = table[bk].permute(2, 0, 1)[None]                             # [1][heads][query][key]
        for li in range(hf["num_hidden_layers"]):
            p = f"encoder.layer.{li}."
            split = lambda y: y.view(B, L, heads, dh).transpose(1, 2)           # noqa: E731
            q, k, v = (split(r(lin(x, p + nm))) for nm in ("q", "k", "v"))
            sc = q @ k.transpose(-1, -2) * scale
            if bias is not None:
                sc = sc + bias
            if stats is not None and li == 0 and s0 == 0:
                pair = real[:, None, :, None] & real[:, None, None, :]
                stats["logit_std"] = float(sc[pair.expand_as(sc)].std())
                am = sc.masked_fill(~real[:, None, None, :], -float("inf")).argmax(-1) // 32      # [B][heads][L]
                rows = real[:, None, :].expand_as(am)
                stats["argmax_key_block"] = am[rows].numpy()
                stats["key_blocks"] = ((lens_t + 31) // 32)[:, None, None].expand_as(am)[rows].numpy()
            sc = sc.masked_fill(~keymask[:, None, None, :], -float("inf"))
            e = torch.exp(sc - sc.max(-1, keepdim=True).values)
            ctx = r((r(e) @ v) / e.sum(-1, keepdim=True))
            ctx = ctx.transpose(1, 2).reshape(B, L, H)
            x = r(ln(x + r(lin(ctx, p + "o")), p + "ln1"))
            h1 = lin(x, p + "ffn1")
            h1 = torch.nn.functional.gelu(h1, approximate="tanh" if mutant == "tanh_gelu" else "none")
            x = ln(x + r(lin(r(h1), p + "ffn2")), p + "ln2")
            if li + 1 < hf["num_hidden_layers"]:
                x = r(x)                                                        # the last LayerNorm feeds the pooling in f32
        if cls_pool:
            emb = x[:, 0]
        else:
            m = real.unsqueeze(-1).to(dtype)
            den = torch.full_like(m.sum(1), float(L)) if mutant == "mean_over_padded_length" else m.sum(1)
            emb = (x * m).sum(1) / den
        outs.append((torch.nn.functional.normalize(emb, p=2, dim=1).numpy(), emb.numpy()))
    unit, raw = (np.concatenate([o[i] for o in outs]) for i in (0, 1))
    return (unit, raw) if normalize == "both" else (unit if normalize else raw)


def encode_f16_emulated(model_dir: str, ids, lens, normalize=True, dtype=None, batch_size=None) -> np.ndarray:
    """A CPU statement of the rounding the device encoder INTENDS (csrc/encoder.hip): the arithmetic of
    ``forward_tokens`` in float64 (or ``dtype``) with a value rounded to f16 at each place where the kernels hold f16 —
      * every Linear's weight (k_pack_weight; biases, LayerNorm parameters and the relative-bias table stay f32),
      * the embedding LayerNorm's output and every later LayerNorm's output (the activations every GEMM reads, which are
        also the residual stream; k_embed_ln*, k_layernorm*) except the last one, which the pooling reads in f32,
      * the Q, K and V projections' outputs (EPI_ACT / EPI_VT; in k_qkv_attn the f16 fragments staged in LDS),
      * the un-normalised softmax probabilities exp(s - max) fed to the P.V product (pf0 / pf1 in k_attention); their
        sum is taken over the unrounded values and divides the product afterwards,
      * the attention context, the output projection and FFN-down results (`delta`) before the residual add, and the
        GELU output.
    Not modelled (what the factor 4 of the tests' bar is for): MFMA accumulation order and f32 accumulators, __expf and
    the GELU polynomial (|error| <= 6e-5), f32 LayerNorm statistics, the running maximum of the online softmax (rounding
    to f16 is relative, so which maximum the exponent is taken against does not change it), and the folded-LayerNorm paths
    (ANORAG_ENC_FOLD 1 / 2), which round u = x + projection once instead of x and the projection separately."""
    return forward_tokens(model_dir, ids, lens, normalize=normalize, dtype=dtype, f16=True, batch_size=batch_size)


def parity_bar(got, got_raw, emul, emul_raw, ref, ref_raw) -> dict:
    """The encoder tests' bar: the device result's distance from the float64 reference as a multiple of the f16
    emulation's distance from it.  got / emul / ref: unit-norm embeddings [n, H]; *_raw: the un-normalised pooled outputs.
    Returns the four ratios (a result passes when all are <= 4) and the distances they are made of:
      l2, l2_raw — max over sentences of ||x[s] - ref[s]||_2 (raw: relative to ||ref_raw[s]||), device over emulation;
      elem, elem_raw — max over elements of |x - ref| (raw: rows divided by ||ref_raw[s]||), device over emulation."""
    ref, ref_raw = np.asarray(ref, np.float64), np.asarray(ref_raw, np.float64)
    nr = np.linalg.norm(ref_raw, axis=1, keepdims=True)
    out = {}
    for key, g, e, rf, sc in (("", got, emul, ref, 1.0), ("_raw", got_raw, emul_raw, ref_raw, nr)):
        dg, de = (np.asarray(g, np.float64) - rf) / sc, (np.asarray(e, np.float64) - rf) / sc
        out["e_gpu" + key], out["e_emul" + key] = np.linalg.norm(dg, axis=1).max(), np.linalg.norm(de, axis=1).max()
        out["d_gpu" + key], out["d_emul" + key] = np.abs(dg).max(), np.abs(de).max()
        out["l2" + key] = out["e_gpu" + key] / out["e_emul" + key]
        out["elem" + key] = out["d_gpu" + key] / out["d_emul" + key]
    out["worst"] = max(out["l2"], out["l2_raw"], out["elem"], out["elem_raw"])
    return out


BAR_FACTOR = 4.0   # margin over the emulation's own error for what it does not model (encode_f16_emulated's docstring)


def synthetic_sentences(model_dir: str, n: int, seed=7, min_words=3, max_words=24) -> List[str]:
    with open(os.path.join(model_dir, "vocab.txt")) as f:
        words = [w.strip() for w in f if w.strip() and not w.startswith("[") and not w.startswith("##")]
    rng = np.random.default_rng(seed)
    return [" ".join(rng.choice(words, size=rng.integers(min_words, max_words + 1))) for _ in range(n)]
