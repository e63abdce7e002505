"""The inputs of the sharp encoder parity cases, shared by tests/test_encoder_attention_gpu.py (the device against the
bar) and tests/test_encoder_mutants_cpu.py (proof that the bar, on the same inputs, fails a subtly wrong forward).

"Sharp" models: one or two layers (attention is not diluted by depth), query / key projections x ATTN_GAIN (at H 256; x sqrt(256 / H) elsewhere: the
logits of random weights grow with H) so that the scaled logits have std 2-4 (the CPU test asserts the figure), MPNet's relative bias table drawn with std 1.5, and an FFN
in GELU's negative tail (FFN-up bias shifted by FFN_BIAS_SHIFT, FFN-down weights x FFN_DOWN_GAIN): there erf- and
tanh-GELU differ by up to 4.7e-4 on outputs of ~1e-2 whose f16 rounding is ~1e-6, which is what lets the bar tell
them apart (with the plain FFN the tanh mutant sat at 0.2 x the emulation's error: unseparable).

Token batches are built directly (ids [B, L], lengths): [CLS] random-ids [SEP], padding = the model's pad id; ids are drawn
from 5.. so that no real token is the pad id (XLM-R / MPNet count positions over non-pad ids)."""
import os

import numpy as np

from oracle import encoder as oenc

ATTN_GAIN = 2.2
REL_BIAS_STD = 1.5
FFN_BIAS_SHIFT = -2.5
FFN_DOWN_GAIN = 30.0
VOCAB = 512


def sharp_model(path, *, model_type="bert", hidden=256, heads=4, layers=2, max_pos=128, pooling="mean", seed=0, scale_weights=False):
    """scale_weights: weight std 0.05 sqrt(256 / H) instead of a smaller attention gain — logits AND the FFN's
    pre-activations keep the spread they have at H 256 (needed at H 768, where the FFN otherwise leaves GELU's tail)"""
    from safetensors.numpy import load_file, save_file
    d = oenc.make_synthetic_model(str(path), layers=layers, hidden=hidden, heads=heads, intermediate=4 * hidden, vocab=VOCAB,
                                  max_pos=max_pos, pooling=pooling, seed=seed, model_type=model_type,
                                  weight_std=0.05 * (float(np.sqrt(256.0 / hidden)) if scale_weights else 1.0),
                                  attn_gain=ATTN_GAIN * (1.0 if scale_weights else float(np.sqrt(256.0 / hidden))),
                                  rel_bias_std=REL_BIAS_STD if model_type == "mpnet" else None)
    f = os.path.join(d, "model.safetensors")
    t = load_file(f)
    for k in list(t):
        if k.endswith("intermediate.dense.bias"):
            t[k] = (t[k] + FFN_BIAS_SHIFT).astype(np.float32)
        elif k.endswith(".output.dense.weight") and "attention" not in k:
            t[k] = (t[k] * FFN_DOWN_GAIN).astype(np.float32)
    save_file(t, f)
    return d


def token_batch(lens, model_type, seed=1):
    """ids [B, max(lens)] int32, lens int32: [CLS] random [SEP], pad id after"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int32)
    pad = 0 if model_type == "bert" else 1
    ids = np.full((len(lens), int(lens.max())), pad, dtype=np.int32)
    for b, n in enumerate(lens):
        ids[b, :n] = rng.integers(5, VOCAB, size=n)
        ids[b, 0], ids[b, n - 1] = 2, 3
    return ids, lens


def _cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


# name -> (model keywords, lengths, expected dispatch branch).  Token-block counts (B * Lp / 32) of the fused cases: 131, 134,
# 140, 134, 140 — all >= 128 (>= 4096 padded tokens), none a multiple of 8.
CASES = {
    # k_qkv_attn<1|2|4>: lengths at the edges of the 32-key blocks and of the padded length
    "fused_bert_Lp32": (dict(model_type="bert"), _cycle([2, 31, 32, 17], 131), "k_qkv_attn<1>"),
    "fused_mpnet_Lp64": (dict(model_type="mpnet"), _cycle([2, 31, 32, 33, 63, 64], 67), "k_qkv_attn<2>"),
    "fused_xlmr_Lp128": (dict(model_type="xlm-roberta"), _cycle([2, 31, 32, 33, 64, 65, 127, 128], 35), "k_qkv_attn<4>"),
    "fused_bert_all_full_Lp64": (dict(model_type="bert"), [64] * 67, "k_qkv_attn<2>"),          # no masking at all
    "fused_mpnet_row0_long_Lp128": (dict(model_type="mpnet"), [128] + _cycle([2, 5, 9, 20], 34), "k_qkv_attn<4>"),
    # k_attention<64> from the non-fused side of each condition, on the sentences of a fused case
    "attn64_few_blocks": (dict(model_type="xlm-roberta"), _cycle([2, 31, 32, 33, 64, 65, 127, 128], 20), "k_attention<64> skinny"),
    "attn64_Lp96": (dict(model_type="mpnet"), _cycle([2, 31, 32, 33, 63, 64], 67) + [96], "k_attention<64> tiled"),
    # 5-16 key blocks through the online rescale
    "attn32_long": (dict(model_type="bert", hidden=128, heads=4, max_pos=512), [2, 129, 200, 257, 320, 384, 449, 511, 512],
                    "k_attention<32> tiled"),
    "attn64_long_mpnet": (dict(model_type="mpnet", max_pos=512), [130, 255, 256, 300, 480, 512], "k_attention<64> skinny"),
    "attn128_h256": (dict(model_type="xlm-roberta", heads=2, max_pos=512), [2, 129, 190, 384, 512], "k_attention<128> skinny"),
    "attn128_h512": (dict(model_type="bert", hidden=512, heads=4, max_pos=256), [33, 160, 161, 256], "k_attention<128> skinny"),
    # hidden size with KB % 4 != 0: k_embed_ln_wave, k_layernorm_wave and the LDS-free k_gemm
    "h96_wave_kernels": (dict(model_type="bert", hidden=96, heads=3), _cycle([2, 31, 32, 33, 80, 7], 14), "k_attention<32> simple"),
    # ANORAG_ENC_FOLD 0 / 1 / 2 (the test runs all three on these inputs)
    "fold_768": (dict(model_type="bert", hidden=768, heads=12, pooling="cls", scale_weights=True), _cycle([32, 17, 31, 9], 136), "k_qkv_attn<1>"),
}


def expected_branch(hidden, heads, B, L):
    """the attention / GEMM branch enqueue_forward (csrc/encoder.hip) takes for this shape, restated from its conditions"""
    dh, KB, Lp = hidden // heads, hidden // 16, (L + 31) // 32 * 32
    TB = B * Lp // 32
    if KB % 4:
        gemm = "simple"             # launch_gemm: KB % ANR_GEMM_S != 0 -> k_gemm<2, 4>; KB % 4 != 0 -> the *_wave LayerNorms
    else:
        gemm = "skinny" if TB <= 120 else "tiled"
    if dh == 64 and Lp in (32, 64, 128) and KB % 2 == 0 and TB >= 128 and gemm != "skinny":
        return f"k_qkv_attn<{Lp // 32}>"
    return f"k_attention<{dh}> {gemm}"


def build_case(name, tmp_path):
    kw, lens, branch = CASES[name]
    kw = dict(kw)
    d = sharp_model(os.path.join(str(tmp_path), name), **kw)
    ids, lens = token_batch(lens, kw["model_type"])
    assert expected_branch(kw.get("hidden", 256), kw.get("heads", 4), ids.shape[0], ids.shape[1]) == branch, name
    return d, ids, lens, branch, kw


def references(d, ids, lens, batch_size=None):
    """(ref, ref_raw, emul, emul_raw): the float64 forward and the f16 emulation, unit-norm and un-normalised"""
    import torch
    ref, ref_raw = oenc.encode_tokens(d, ids, lens, normalize="both", dtype=torch.float64, batch_size=batch_size)  # transformers
    emul, emul_raw = oenc.encode_f16_emulated(d, ids, lens, normalize="both", batch_size=batch_size)
    return ref, ref_raw, emul, emul_raw
