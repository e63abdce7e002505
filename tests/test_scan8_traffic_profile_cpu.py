"""The committed PMC traffic figure of the headline scan (profiles/r*_pmc_traffic_k_scan.json, what `bench.py --full`
reports) must describe the current kernel source and the 8-bit image the 10 M-row headline scans, at about the algorithmic
bytes (DESIGN.md §4 "Round 8": the scale words once came from HBM several times per tile)."""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from scan_source_hash import scan_source_sha256  # noqa: E402


def _latest():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic_k_scan.json")))
    assert files, "no committed traffic profile"
    with open(files[-1]) as f:
        return json.load(f)


def test_the_traffic_profile_matches_the_scan_source():
    p = _latest()
    assert p["kernel_source_region"] == "k_scan"
    assert p["kernel_source_sha256"] == scan_source_sha256()


def test_the_traffic_profile_is_the_eight_bit_scan_at_the_algorithmic_bytes():
    p = _latest()
    assert p["kernel"].startswith("k_scan8<false")
    assert p["bytes_per_stored_value"] == 1.0625
    assert p["algorithmic_bytes_per_launch"] == p["rows"] * p["dim"] * 1.0625
    t = (2 * p["FETCH_SIZE_KiB_per_launch"] + p["WRITE_SIZE_KiB_per_launch"]) * 1024
    assert abs(t - p["traffic_bytes_per_launch"]) < 1.0
    assert 0.99 <= p["traffic_over_algorithmic"] <= 1.02
