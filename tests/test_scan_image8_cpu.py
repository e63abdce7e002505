"""The 8-bit scan image (ANR_OPT_SCAN_BITS 8) on the CPU: known answers of the numpy restatement (tests/scan_image8.py) that
tests/test_scan_image8_gpu.py pins the device against, and the resources of the 8-bit scan kernel in the built library."""
import os

import numpy as np
import pytest

import scan_image8 as s8
from codeobj import kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "ano-rag_amd", "anorag_hip", "libanorag_hip.so")


def _row(vals):
    x = np.zeros((1, 32), dtype=np.float32)
    x[0, :len(vals)] = vals
    return x


def test_scale_is_absmax_over_127_rounded_up_to_an_f16():
    # 127 / 127 = 1 exactly: no step up
    assert s8.scales(_row([127.0, -3.0]))[0, 0] == np.float16(1.0)
    # 1 / 127 = 0.0078740157 -> f16 0.00787354 (rounded down): 0.00787354 * 127 < 1, so one step up
    s = s8.scales(_row([1.0]))[0, 0]
    assert s.view(np.uint16) == np.float16(1.0 / 127).view(np.uint16) + 1
    assert float(s) * 127 >= 1.0 and float(np.nextafter(s, np.float16(0))) * 127 < 1.0
    # an all-zero group keeps s = 0 and code 0; the group after it is independent
    x = np.zeros((1, 64), dtype=np.float32)
    x[0, 40] = -2.5
    c, s = s8.codes(x)
    assert s[0, 0] == 0 and not c[0, 0].any()
    assert s[0, 1] > 0 and c[0, 1, 8] == -127


def test_codes_round_half_to_even_at_group_edges():
    # s = 1: x / s = 0.5, 1.5, 2.5, -0.5 -> 0, 2, 2, -0 (ties to even), the group maximum at the last dimension
    x = _row([0.5, 1.5, 2.5, -0.5] + [0.0] * 27 + [127.0])
    c, s = s8.codes(x)
    assert s[0, 0] == 1.0
    assert c[0, 0, :4].tolist() == [0, 2, 2, 0] and c[0, 0, 31] == 127
    assert s8.decode(x)[0, :4].tolist() == [0.0, 2.0, 2.0, 0.0]


def test_values_at_the_f16_limits_stay_finite():
    x = _row([65504.0, -65504.0, 65472.0, 1.0])
    c, s = s8.codes(x)
    assert s[0, 0] == np.float16(516.0)
    # 516 * 127 = 65532 would round to infinity: the code is held at floor(65504 / 516) = 126 (f16(65016) = 65024)
    assert c[0, 0, :3].tolist() == [126, -126, 126]
    v = s8.decode(x)
    assert np.isfinite(v).all() and v[0, 0] == 65024.0 and v[0, 3] == 0.0
    # a tiny group: the scale is the smallest subnormal f16 (2^-24), the codes are what that resolution allows
    tiny = _row([6.0e-6, -3.0e-6])
    c, s = s8.codes(tiny)
    assert float(s[0, 0]) == 2.0 ** -24 and c[0, 0, :2].tolist() == [101, -50]
    assert abs(s8.decode(tiny)[0, 0] - 6.0e-6) <= float(s[0, 0]) / 2


def test_decode_is_one_rounding_of_scale_times_code():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((64, 96)).astype(np.float32)
    c, s = s8.codes(x)
    want = (s.astype(np.float64)[:, :, None] * c).astype(np.float16).astype(np.float32).reshape(64, -1)[:, :96]
    assert s8.decode(x).tobytes() == want.tobytes()
    assert np.abs(c).max() <= 127


def test_error_norm_of_unit_rows():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2000, 768)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    e = s8.error_norm(x)
    assert 0.004 < e < 0.0075            # ~1.7x the 12-bit image's ~0.0038
    assert s8.error_norm(x[:0]) == 0.0


@pytest.fixture(scope="module")
def md():
    if not os.path.exists(SO):
        pytest.skip("libanorag_hip.so not built")
    return kernel_metadata(SO)


def test_the_eight_bit_scan_keeps_three_waves_per_simd_without_scratch(md):
    """k_scan8 (the 10 M-row headline's image): <= 152 registers, so three waves per SIMD and a shadow side kernel's wave
    fit on a SIMD; no scratch; both the streaming and the cache-resident form"""
    picked = {n: k for n, k in md.items() if "k_scan8ILb0ELi8ELi768" in n}
    assert len(picked) == 2, sorted(picked)
    for name, k in picked.items():
        assert k[".max_flat_workgroup_size"] == 768, name
        assert k[".vgpr_count"] <= 152, (name, k[".vgpr_count"])
        assert k.get(".private_segment_fixed_size", 0) == 0 and k.get(".vgpr_spill_count", 0) == 0, name
    assert any(n.endswith("ELb1EEEvNS_10ScanParamsE") for n in picked)   # non-temporal loads
    assert any(n.endswith("ELb0EEEvNS_10ScanParamsE") for n in picked)
