"""The 8-bit scan's k-loop is pipelined by hand (DESIGN.md §4 "Round 16"): the decoded operand of the coming k-block lives
across every MFMA.  Every k_scan8 instantiation must still run three waves per SIMD (<= 168 vector registers), spill nothing
and declare no LDS of its own (its only LDS is the dynamic block launch_scan sizes: the query image and the ladder, 100.5 KiB
at 768 dimensions, which is what leaves room for a neighbour on the CU).  Read from the BUILT library, as
tests/test_shadow_kernels_cpu.py does."""
import os

import pytest

from codeobj import kernel_metadata

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "..", "ano-rag_amd", "anorag_hip", "libanorag_hip.so")

MAX_VGPRS = 168  # 512 registers per SIMD lane / 3 waves, in allocation granules of 8


@pytest.fixture(scope="module")
def scan8():
    if not os.path.exists(SO):
        pytest.skip("libanorag_hip.so not built")
    out = {n: k for n, k in kernel_metadata(SO).items() if "k_scan8I" in n}
    assert out, "no k_scan8 kernel in the library"
    return out


def test_every_instantiation_is_there_and_only_the_shipped_form(scan8):
    # DENSE x CH {4, 8} x STREAM, all with 768-thread blocks; the developer A/B kernels are not in a shipped library
    want = {f"_ZN3anr7k_scan8ILb{d}ELi{ch}ELi768ELb{s}EEEvNS_10ScanParamsE" for d in (0, 1) for ch in (4, 8) for s in (0, 1)}
    assert set(scan8) == want, sorted(set(scan8) ^ want)


def test_three_waves_per_simd_no_scratch_no_static_lds(scan8):
    for name, k in scan8.items():
        assert k[".max_flat_workgroup_size"] == 768, name
        assert k[".vgpr_count"] <= MAX_VGPRS, (name, k[".vgpr_count"])
        assert k.get(".agpr_count", 0) == 0, name          # MFMA results in ordinary registers (-amdgpu-mfma-vgpr-form)
        assert k.get(".private_segment_fixed_size", 0) == 0, name
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
        assert k[".group_segment_fixed_size"] == 0, name
        assert k[".sgpr_count"] <= 104, (name, k[".sgpr_count"])
