"""GPU parity of the sentence encoder's attention on SHARP shallow models (tests/encoder_cases.py: one or two layers,
scaled logits of std 2-4, MPNet bias table of std 1.5, an FFN in GELU's tail), against a bar that is derived, not chosen:

    ref  = the float64 transformers forward on the same tokens,
    emul = oracle.encoder.encode_f16_emulated: the same forward with a value rounded to f16 wherever the kernels hold f16,
    bar  : max_s ||got[s] - ref[s]|| <= 4 max_s ||emul[s] - ref[s]||  and  max |got - ref| <= 4 max |emul - ref|,
           on the unit-norm embedding and on the un-normalised pooled output relative to ||ref[s]||.

tests/test_encoder_mutants_cpu.py proves on the same inputs that a missing / reversed / rolled / transposed relative
bias, a softmax scale off by 10 %, one unmasked padding key, a position offset off by one, tanh-GELU and a mean over the
padded length all land ABOVE this bar.  Every test prints its branch and its ratios e_gpu / e_emul (DESIGN.md §6 has the
table).  Token batches go straight to DeviceEncoder.forward: one forward per case, the shape decides the branch.

Dispatch branch in anr_encoder_forward* (enqueue_forward, csrc/encoder.hip) -> test that asserts it ran
(by restating the branch condition on the shape: encoder_cases.expected_branch):
    k_qkv_attn<1>                         test_case_within_bar[fused_bert_Lp32], test_fold_modes_on_a_sharp_768_wide_model
    k_qkv_attn<2>                         test_case_within_bar[fused_mpnet_Lp64], [fused_bert_all_full_Lp64]
    k_qkv_attn<4>                         test_case_within_bar[fused_xlmr_Lp128], [fused_mpnet_row0_long_Lp128]
    k_attention<64>, TB < 128 / skinny    test_case_within_bar[attn64_few_blocks] (rows of fused_xlmr_Lp128), [attn64_long_mpnet]
    k_attention<64>, Lp = 96, tiled GEMMs test_case_within_bar[attn64_Lp96] (fused_mpnet_Lp64's rows + one of 96 tokens)
    k_attention<32>, 5-16 key blocks      test_case_within_bar[attn32_long] (128 token blocks: tiled GEMMs)
    k_attention<128>                      test_case_within_bar[attn128_h256], [attn128_h512]
    k_embed_ln_wave, k_layernorm_wave,
      k_gemm<2, 4> (KB % 4 != 0)          test_case_within_bar[h96_wave_kernels]
    k_embed_ln, k_layernorm<*>            every other case (KB % 4 == 0)
    k_gemm_skinny_qkv / k_gemm_skinny     the "skinny" cases; B = 1 forwards of test_alone_equals_inside_a_ragged_batch
    k_gemm_pp / k_gemm_lds                the "tiled" cases and the fused ones (output projection, FFN)
    ANORAG_ENC_FOLD 0 / 1 / 2             test_fold_modes_on_a_sharp_768_wide_model (1 and 2 must differ from 0 in bits)
    anr_encoder_forward_shared            test_alone_equals_inside_a_ragged_batch (bit-identical to the plain call)
    check_forward_args (host)             test_zero_length_rows_are_rejected_on_the_host (no kernel is started)
Left without a test here: anr_encoder_forward_dev (same enqueue_forward, other output pointer: tests/test_dropin_gpu.py);
k_embed_ln_wave / k_layernorm_wave for H > 1024 (the same kernels as H = 96, only longer loops); the developer
switches ANORAG_GEMM_SIMPLE / NOSKINNY / NARROW / SKINNY_MAX."""
import numpy as np
import pytest

import encoder_cases as ec
from oracle import encoder as oenc

pytestmark = pytest.mark.gpu


def _forward_both(d, ids, lens):
    """(unit-norm, un-normalised) device results of ONE forward each of the whole token batch"""
    from anorag_hip.encoder import SentenceEncoder
    enc = SentenceEncoder(d)
    types = np.zeros_like(ids) if enc._info["hf"].get("type_vocab_size", 1) > 1 else None
    got = enc._enc.forward(ids, lens, types, normalize=True)
    got_raw = enc._enc.forward(ids, lens, types, normalize=False)
    enc.close()
    return got, got_raw


def _assert_bar(label, got, got_raw, refs, rows=slice(None)):
    ref, ref_raw, emul, emul_raw = (x[rows] for x in refs)
    bar = oenc.parity_bar(got, got_raw, emul, emul_raw, ref, ref_raw)
    print(f"RATIO {label}: e_gpu/e_emul l2 {bar['l2']:.2f} l2_raw {bar['l2_raw']:.2f} elem {bar['elem']:.2f} "
          f"elem_raw {bar['elem_raw']:.2f} (e_emul {bar['e_emul']:.2e}, e_gpu {bar['e_gpu']:.2e})")
    assert bar["worst"] <= oenc.BAR_FACTOR, (label, bar)
    assert np.allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    return bar


@pytest.mark.parametrize("name", [n for n in ec.CASES if n != "fold_768"])
def test_case_within_bar(tmp_path, name):
    d, ids, lens, branch, kw = ec.build_case(name, tmp_path)     # asserts that the shape takes the branch it is named for
    Lp = (ids.shape[1] + 31) // 32 * 32
    if branch.startswith("k_qkv_attn"):
        tb = ids.shape[0] * Lp // 32
        assert ids.shape[0] * Lp >= 4096 and tb % 8 != 0, (ids.shape, Lp)
    print(f"BRANCH {name}: {branch}, B {ids.shape[0]}, L {ids.shape[1]}, Lp {Lp}")
    got, got_raw = _forward_both(d, ids, lens)
    _assert_bar(name, got, got_raw, ec.references(d, ids, lens))


@pytest.mark.parametrize("name", ["fused_xlmr_Lp128", "attn64_long_mpnet"])
def test_padding_ids_do_not_matter(tmp_path, name):
    """the same sentences with the padding ids replaced by random valid ids: within the bar of the same reference"""
    d, ids, lens, branch, _ = ec.build_case(name, tmp_path)
    noisy = ids.copy()
    rng = np.random.default_rng(3)
    pad = np.arange(ids.shape[1])[None, :] >= lens[:, None]
    noisy[pad] = rng.integers(5, ec.VOCAB, size=int(pad.sum()))
    assert pad.sum() > 0 and not np.array_equal(noisy, ids)
    got, got_raw = _forward_both(d, noisy, lens)
    _assert_bar(f"{name} random padding ids ({branch})", got, got_raw, ec.references(d, ids, lens))


def test_alone_equals_inside_a_ragged_batch(tmp_path):
    """rows of the fused 128-token case forwarded alone (B = 1: other padded length, the skinny kernels and k_attention<64>
    instead of k_qkv_attn<4>): each within the bar of the batch's reference row; through the combining queue the single
    forward is bit-identical to the plain call (the queue only merges requests whose arithmetic is unchanged)"""
    from anorag_hip.encoder import SentenceEncoder
    d, ids, lens, _, _ = ec.build_case("fused_xlmr_Lp128", tmp_path)
    refs = ec.references(d, ids, lens)
    enc = SentenceEncoder(d)
    rows = [0, 1, 2, 3, 4, 5, 6, 7]          # lengths 2, 31, 32, 33, 64, 65, 127, 128
    got, got_raw = [], []
    for b in rows:
        one, n = ids[b:b + 1, :lens[b]], lens[b:b + 1]
        assert ec.expected_branch(256, 4, 1, int(lens[b])) == "k_attention<64> skinny"
        got.append(enc._enc.forward(one, n, None, normalize=True))
        got_raw.append(enc._enc.forward(one, n, None, normalize=False))
        assert np.array_equal(enc._enc.forward(one, n, None, normalize=True, shared=True), got[-1])
    enc.close()
    _assert_bar("rows of fused_xlmr_Lp128 alone", np.concatenate(got), np.concatenate(got_raw), refs, rows=rows)


def test_fold_modes_on_a_sharp_768_wide_model(tmp_path, monkeypatch):
    """ANORAG_ENC_FOLD 0 / 1 / 2 on one sharp bge-base-wide model (2 layers, 136 sequences of <= 32 tokens: 136 token
    blocks, all three GEMMs on the 8-wave tile kernel): each within the bar of the same reference; 1 and 2 are different
    arithmetic from 0, so identical bits would mean the fold did not run"""
    d, ids, lens, branch, _ = ec.build_case("fold_768", tmp_path)
    assert ids.shape[0] * 32 // 32 >= 128
    refs = ec.references(d, ids, lens)
    outs = {}
    for fold in ("0", "1", "2"):
        monkeypatch.setenv("ANORAG_ENC_FOLD", fold)
        outs[fold] = _forward_both(d, ids, lens)
        _assert_bar(f"fold_768 ANORAG_ENC_FOLD={fold} ({branch})", *outs[fold], refs)
    assert not np.array_equal(outs["1"][0], outs["0"][0]) and not np.array_equal(outs["2"][0], outs["0"][0])


def test_zero_length_rows_are_rejected_on_the_host(tmp_path):
    """a row of length 0 would divide by l = 0 in the attention kernels: anr_encoder_forward* refuse it (and a negative or
    too long one) in check_forward_args, before any launch"""
    from anorag_hip.encoder import SentenceEncoder
    d, ids, lens, _, _ = ec.build_case("attn64_few_blocks", tmp_path)
    enc = SentenceEncoder(d)
    for bad in (0, -1, ids.shape[1] + 1):
        wrong = lens.copy()
        wrong[3] = bad
        for shared in (False, True):
            with pytest.raises(Exception, match="out of range"):
                enc._enc.forward(ids, wrong, None, normalize=True, shared=shared)
    enc.close()
