"""CPU model of the exact index's certificate over the magnitude sweep (tests/magnitude_cases.py).

oracle.flat_index restates the kernels' bound (certificate_eps) and the scan's arithmetic (scan_scores: a float32 fma chain
in k order, the MFMA's numerics, plus the float32 row bias for L2).  For every case and every scan image (16, 12, 8 bits)
the two premises the certificate rests on are checked on ALL (query, row) pairs:
  1. |scan score - exact rank| <= eps without the conversion term;
  2. (L2) that error plus the error of the k-th rank the kernel derives from the float32 distance and the float32 ||q||^2
     it holds, 0.5 * (||q||^2 - dist), is <= eps.
Premise 2 is what far_queries-l2 broke before the conversion term 3e-8 (||q||^2 + |dist|) existed: f16-exact data, so eps
was the accumulation term alone (0.0157 at ||q|| = 1024, ||x|| = 1), against a conversion error of up to a quarter spacing
of a distance near 2^20 plus a quarter spacing of ||q||^2 (0.047).  The 'convert' mutant keeps that case as the regression.
Mutants: the model with one term dropped must violate a premise somewhere in the sweep — every term is needed by a case.
The excuse caps of magnitude_cases.check_exact are conditions on the inputs and are checked here, from the oracle alone."""
import functools

import numpy as np
import pytest

import magnitude_cases as mc
import scan_image8 as s8
from oracle import flat_index as orc

BITS = (16, 12, 8)


def _worst(num, den):
    """max of num / den with 0 / 0 = 0 (an exact scan under a zero bound holds)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(num == 0, 0.0, num / den), initial=0.0))


@functools.lru_cache(maxsize=None)
def _report(name):
    """near-tie counts, and per image the worst ratio (error / eps) of both premises for the formula and for each mutant"""
    x, q, metric, normalize, k = mc.case(name)
    xm, qm = mc.preprocess(x, normalize), mc.preprocess(q, normalize)
    s64 = orc.exact_scores(qm, xm, metric)
    rep = {"ties": mc.near_tie_queries(s64, k, metric), "metric": metric, "bits": {}}
    rep["usable"] = bool(np.abs(xm).max() <= mc.F16_MAX)
    if not rep["usable"]:
        return rep
    Dr, Ir = orc.flat_search(qm, xm, k, metric, scores=s64)
    del s64
    rank = orc.exact_ranks(xm, qm, metric)
    conv = np.zeros(len(qm))
    if metric == "l2":
        qn2 = (qm.astype(np.float64) ** 2).sum(axis=1).astype(np.float32).astype(np.float64)   # what k_prepq keeps
        kth_dev = 0.5 * (qn2 - Dr[:, k - 1].astype(np.float64))
        conv = np.abs(kth_dev - rank[np.arange(len(qm)), Ir[:, k - 1]])
    for bits in BITS:
        img = s8.decode(xm) if bits == 8 else None
        stats = orc.certificate_stats(xm, bits, img)
        assert stats[2]
        scan = orc.scan_scores(xm, qm, metric, bits, img)
        err = np.abs(scan.astype(np.float64) - rank).max(axis=1)           # NaN for a query whose f16 image overflows
        out = {"refused": [], "ratio": {}}
        for drop in (None,) + orc.EPS_TERMS:
            kw = dict(metric=metric, bits=bits, image=img, drop=drop, stats=stats)
            base = orc.certificate_eps(xm, qm, kth=None, **kw)
            full = orc.certificate_eps(xm, qm, kth=Dr[:, k - 1] if metric == "l2" else None, **kw)
            live = np.isfinite(full)
            if drop is None:
                out["refused"] = [int(i) for i in np.nonzero(~live)[0]]
                assert np.isfinite(err[live]).all()
            out["ratio"][drop] = (_worst(err[live], base[live]),
                                  _worst(err[live] + conv[live], full[live]) if metric == "l2" else 0.0)
        rep["bits"][bits] = out
    return rep


@pytest.mark.parametrize("name", mc.NAMES)
def test_near_ties_stay_within_the_excuse_cap(name):
    anywhere, boundary = _report(name)["ties"]
    print(f"{name}: {anywhere} of {mc.NQ} queries with a float32 near-tie among the best k + 1 ({boundary} at the k-th)")
    assert anywhere <= mc.EXCUSE_CAP[name]


@pytest.mark.parametrize("name", mc.NAMES)
def test_the_certificate_premises_hold_on_every_pair(name):
    rep = _report(name)
    assert rep["usable"] == (name not in mc.ROWS_OUT_OF_RANGE)      # beyond the f16 range the index scans nothing
    if not rep["usable"]:
        return
    for bits in BITS:
        out = rep["bits"][bits]
        # a query whose f16 image overflows has eps = inf (or NaN = 0 * inf on f16-exact rows): never certified
        assert out["refused"] == (list(mc.OUT_OF_RANGE_QUERIES) if name in mc.QUERIES_OUT_OF_RANGE else []), out["refused"]
        r1, r2 = out["ratio"][None]
        print(f"{name} bits {bits}: max |scan - rank| / eps = {r1:.3g}, with the L2 conversion {r2:.3g}")
        assert r1 <= 1.0, (name, bits, r1)
        assert r2 <= 1.0, (name, bits, r2)


@pytest.mark.parametrize("term", orc.EPS_TERMS)
def test_every_term_of_eps_is_needed_by_a_case(term):
    """the formula with `term` dropped violates a premise on at least one case of the sweep"""
    broken = []
    for name in mc.NAMES:
        rep = _report(name)
        if not rep["usable"] or (term in ("bias", "convert") and rep["metric"] != "l2"):
            continue
        worst = max(max(rep["bits"][b]["ratio"][term]) for b in BITS)
        if worst > 1.0:
            broken.append((name, round(worst, 2)))
    print(f"without {term}: {broken}")
    assert broken, f"no case of the sweep needs the term {term}: a case is missing"
    if term == "convert":
        assert "far_queries-l2" in [n for n, _ in broken]        # the regime that made the term necessary
