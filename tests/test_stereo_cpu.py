"""Frame::ComputeStereoMatches oracle (oracle/orb_stereo_oracle.cpp) against an independent
pure-Python restatement of reference src/Frame.cc:1102-1358 (tests/stereo_ref.py), on synthetic EuRoC-shaped stereo pairs.

The reference ships no stereo fixtures, so parity with the real reference is
unpinned; this pins the C restatement against a second, loop-by-loop reading of the source.
"""
from __future__ import annotations

import numpy as np
import pytest

from stereo_ref import python_stereo

EUROC_B = 0.110074  # Examples/Stereo/EuRoC.yaml: Camera.bf / fx


def _extract_pair(oracle, synth, seed, nf=1200, w=752, h=480, dmin=4, dmax=48):
    left, right, _ = synth.stereo_pair(w, h, seed=seed, dmin=dmin, dmax=dmax)
    exl, exr = oracle.OracleExtractor(nf, 1.2, 8, 20, 7), oracle.OracleExtractor(nf, 1.2, 8, 20, 7)
    kl, dl, _ = exl(left, (0, 0))
    kr, dr, _ = exr(right, (0, 0))
    pl = [exl.level_padded(l) for l in range(8)]
    pr = [exr.level_padded(l) for l in range(8)]
    return kl, dl, kr, dr, pl, pr, exl.params()


@pytest.mark.parametrize("seed,bf", [(200, 47.90639384423901), (231, 47.90639384423901), (232, 8.0)])
def test_stereo_oracle_matches_python(oracle, synth, seed, bf):
    kl, dl, kr, dr, pl, pr, p = _extract_pair(oracle, synth, seed)
    ur, dp, kept = oracle.compute_stereo_matches(kl, dl, kr, dr, pl, pr, p["scale"], p["inv_scale"], bf, EUROC_B)
    pur, pdp, pkept = python_stereo(kl, dl, kr, dr, pl, pr, p["scale"], p["inv_scale"], bf, EUROC_B)
    assert kept == pkept == int((ur >= 0).sum())
    assert np.array_equal(ur.view(np.uint32), pur.view(np.uint32))
    assert np.array_equal(dp.view(np.uint32), pdp.view(np.uint32))
    if bf > 40:
        assert kept > 100  # the synthetic pair has real stereo structure


def test_stereo_oracle_quality(oracle, synth):
    """Kept matches recover the generator's disparity (per 16-row x 64-col block) to ~1 px."""
    left, right, disp = synth.stereo_pair(752, 480, seed=200)
    kl, dl, kr, dr, pl, pr, p = _extract_pair(oracle, synth, 200)
    ur, dp, kept = oracle.compute_stereo_matches(kl, dl, kr, dr, pl, pr, p["scale"], p["inv_scale"],
                                                 47.90639384423901, EUROC_B)
    good = np.flatnonzero(ur >= 0)
    truth = disp[(kl["y"][good] // 16).astype(int), (kl["x"][good] // 64).astype(int)]
    err = np.abs((kl["x"][good] - ur[good]) - truth)
    assert np.median(err) < 1.0


def test_stereo_oracle_edge_cases(oracle, synth):
    kl, dl, kr, dr, pl, pr, p = _extract_pair(oracle, synth, 200)
    # no right keypoints: nothing matches (and no cull on an empty set)
    ur, dp, kept = oracle.compute_stereo_matches(kl, dl, kr[:0], dr[:0], pl, pr, p["scale"], p["inv_scale"],
                                                 47.9, EUROC_B)
    assert kept == 0 and (ur == -1).all() and (dp == -1).all()
    # right == left: SAD 0 everywhere, so the median cull (SAD >= 1.5*1.4*0) drops every match
    ur, dp, kept = oracle.compute_stereo_matches(kl, dl, kl, dl, pl, pl, p["scale"], p["inv_scale"], 47.9, EUROC_B)
    assert kept == 0 and (ur == -1).all()
    # top rows identical, the rest a real pair: zero-disparity matches take the 0.01 clamp and survive
    left, right, _ = synth.stereo_pair(752, 480, seed=200)
    right[:160] = left[:160]
    exl, exr = oracle.OracleExtractor(1200, 1.2, 8, 20, 7), oracle.OracleExtractor(1200, 1.2, 8, 20, 7)
    kl, dl, _ = exl(left, (0, 0))
    kr, dr, _ = exr(right, (0, 0))
    pl = [exl.level_padded(l) for l in range(8)]
    pr = [exr.level_padded(l) for l in range(8)]
    ur, dp, kept = oracle.compute_stereo_matches(kl, dl, kr, dr, pl, pr, p["scale"], p["inv_scale"], 47.9, EUROC_B)
    pur, pdp, pkept = python_stereo(kl, dl, kr, dr, pl, pr, p["scale"], p["inv_scale"], 47.9, EUROC_B)
    assert kept == pkept > 0 and np.array_equal(ur, pur) and np.array_equal(dp, pdp)
    assert (ur == (kl["x"].astype(np.float64) - 0.01).astype(np.float32)).any()
