"""CPU proof that the encoder parity bar (oracle.encoder.parity_bar: the distance from the float64 transformers forward
as a multiple of the f16 emulation's distance, at most BAR_FACTOR = 4) would fail a subtly wrong kernel: on the model and
token batch of every case of tests/test_encoder_attention_gpu.py each wrong forward of oracle.encoder.MUTANTS — MPNet bias
table zeroed / reversed / rolled by one bucket / indexed by query - key, softmax scale x 1.1, one padding key of the
shortest sentence left unmasked, position offset 1 instead of 2 (XLM-R / MPNet), tanh-GELU for erf-GELU, mean pooling that
divides by the padded length — lands above the bar.  A mutant that a model cannot express is not run on it (bias: MPNet
only; position offset: not BERT; unmasked key: needs a ragged batch; pooling: mean-pooled models).  It also checks the
emulation itself: with rounding off it IS the transformers forward (<= 1e-6), and the float64 reference at batch size 1
equals the full batch (<= 1e-6), which is the padding invariance the device cases rely on."""
import numpy as np
import pytest

import encoder_cases as ec
from oracle import encoder as oenc


def _applicable(mutant, kw, lens):
    if mutant.startswith("bias_"):
        return kw["model_type"] == "mpnet"
    if mutant == "pos_offset_1":
        return kw["model_type"] != "bert"
    if mutant == "unmasked_pad_key":
        return int(np.min(lens)) < int(np.max(lens))
    if mutant == "mean_over_padded_length":
        return kw.get("pooling", "mean") == "mean" and int(np.min(lens)) < int(np.max(lens))
    return True


@pytest.mark.parametrize("name", list(ec.CASES))
def test_every_mutant_is_above_the_bar(tmp_path, name):
    d, ids, lens, branch, kw = ec.build_case(name, tmp_path)
    ref, ref_raw, emul, emul_raw = ec.references(d, ids, lens)
    st = {}
    own, own_raw = oenc.forward_tokens(d, ids, lens, normalize="both", stats=st)
    # the written-out forward with all rounding off is the transformers forward
    assert np.linalg.norm(own - ref, axis=1).max() <= 1e-6 and np.abs(own_raw - ref_raw).max() <= 1e-6 * np.abs(ref_raw).max()
    # sharp: the scaled logits of layer 0 have std 2-4
    print(f"{name}: branch {branch}, logit std {st['logit_std']:.2f}, e_emul {np.linalg.norm(emul - ref, axis=1).max():.2e}")
    assert 2.0 <= st["logit_std"] <= 4.0, st["logit_std"]
    if int(np.max(lens)) > 128:
        # several key blocks: the running maximum of the online softmax grows late for some rows (largest logit in the
        # sequence's last key block) and is set at once for others (largest logit in block 0)
        blk, nblk = st["argmax_key_block"], st["key_blocks"]
        multi = nblk >= 5
        assert np.sum(multi & (blk == nblk - 1)) >= 32 and np.sum(multi & (blk == 0)) >= 32
    for mutant in oenc.MUTANTS:
        if not _applicable(mutant, kw, lens):
            continue
        got, got_raw = oenc.forward_tokens(d, ids, lens, normalize="both", mutant=mutant)
        bar = oenc.parity_bar(got, got_raw, emul, emul_raw, ref, ref_raw)
        print(f"  {mutant:26s} l2 {bar['l2']:8.1f}  l2_raw {bar['l2_raw']:8.1f}  elem {bar['elem']:8.1f}  elem_raw {bar['elem_raw']:8.1f}")
        assert bar["worst"] > oenc.BAR_FACTOR, (name, mutant, bar)
    # the emulation passes its own bar by construction (ratio 1): the bar is not vacuous in the other direction
    assert oenc.parity_bar(emul, emul_raw, emul, emul_raw, ref, ref_raw)["worst"] == 1.0


@pytest.mark.parametrize("name", ["fused_xlmr_Lp128", "fused_mpnet_row0_long_Lp128", "attn32_long"])
def test_float64_reference_is_padding_invariant(tmp_path, name):
    import torch
    d, ids, lens, _, _ = ec.build_case(name, tmp_path)
    full = oenc.encode_tokens(d, ids, lens, dtype=torch.float64)
    one = oenc.encode_tokens(d, ids, lens, dtype=torch.float64, batch_size=1)
    assert np.abs(full - one).max() <= 1e-6


def test_the_old_bar_passed_and_the_new_bar_fails_the_recorded_mutants(tmp_path):
    """The three wrong forwards that passed cosine >= 0.9995 / max |diff| <= 5e-3 on test_mpnet_relative_position_bias's
    old inputs (bias table zeroed / reversed / rolled by one bucket) fail the new bar on its inputs of today (the same
    sentences, rel_bias_std 1.5)."""
    d = oenc.make_synthetic_model(str(tmp_path / "mp"), layers=3, hidden=256, heads=8, intermediate=1024, pooling="mean",
                                  model_type="mpnet", max_pos=256, rel_bias_std=1.5)
    sents = (oenc.synthetic_sentences(d, 12, seed=5, min_words=2, max_words=12)
             + oenc.synthetic_sentences(d, 6, seed=6, min_words=60, max_words=140))
    ids, lens = oenc.tokenize(d, sents)
    ref, ref_raw, emul, emul_raw = ec.references(d, ids, lens)
    for mutant in ("bias_zero", "bias_reversed", "bias_rolled"):
        got, got_raw = oenc.forward_tokens(d, ids, lens, normalize="both", mutant=mutant)
        bar = oenc.parity_bar(got, got_raw, emul, emul_raw, ref, ref_raw)
        print(f"{mutant}: worst ratio {bar['worst']:.1f}")
        assert bar["worst"] > oenc.BAR_FACTOR, (mutant, bar)


def test_default_synthetic_model_is_unchanged_by_the_new_arguments(tmp_path):
    from safetensors.numpy import load_file
    import os
    a = oenc.make_synthetic_model(str(tmp_path / "a"), layers=1, hidden=64, heads=2, intermediate=128, vocab=64, max_pos=32,
                                  model_type="mpnet")
    b = oenc.make_synthetic_model(str(tmp_path / "b"), layers=1, hidden=64, heads=2, intermediate=128, vocab=64, max_pos=32,
                                  model_type="mpnet", attn_gain=1.0, rel_bias_std=None)
    c = oenc.make_synthetic_model(str(tmp_path / "c"), layers=1, hidden=64, heads=2, intermediate=128, vocab=64, max_pos=32,
                                  model_type="mpnet", attn_gain=2.0, rel_bias_std=1.5)
    ta, tb, tc = (load_file(os.path.join(x, "model.safetensors")) for x in (a, b, c))
    changed = {k for k in ta if not np.array_equal(ta[k], tc[k])}
    assert all(np.array_equal(ta[k], tb[k]) for k in ta)
    assert changed == {k for k in ta if ".attn.q." in k or ".attn.k." in k or "relative_attention_bias" in k}
    q = next(k for k in ta if k.endswith("attn.q.weight"))
    assert np.array_equal(tc[q], ta[q] * np.float32(2.0))
    assert abs(tc["encoder.relative_attention_bias.weight"].std() - 1.5) < 0.3
