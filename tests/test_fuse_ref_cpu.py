"""Pins tests/fuse_ref.py, the Python restatement of ORBmatcher::Fuse's search (reference
src/ORBmatcher.cc:1356-1506) that the GPU tests compare against: on the hand-built cases of fuse_cases.py,
whose expected values follow from the reference's statements; its float arithmetic against the C++
isInFrustum oracle; and the properties of the main scene that keep the GPU tests from passing vacuously."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import fuse_cases
import fuse_ref as ref
import fuse_scenes

CASES = fuse_cases.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_built(case):
    _, kf, pts, th, want_idx, want_dist, want_reason = case
    idx, dist, reason, _ = ref.fuse_search([kf], pts, th)
    assert reason[0].tolist() == want_reason, [ref.REASONS[r] for r in reason[0]]
    assert idx[0].tolist() == want_idx
    assert dist[0].tolist() == want_dist


def test_hand_built_levels():
    by_name = {c[0]: c for c in CASES}
    for name, level in (("level_clamp0", 0), ("level_clamp7", 7), ("octave", 3), ("tie_column", 4)):
        _, kf, pts, th, *_ = by_name[name]
        assert ref.fuse_search([kf], pts, th)[3]["level"][0, 0] == level, name


def test_get_features_in_area_early_returns():
    """src/KeyFrame.cc:853-868: each of the four early returns, on a grid that has a keypoint in every
    corner cell (a clamped window would find one)."""
    kf = fuse_cases.make_kf([(2.0, 2.0, 0, 0, -1.0), (633.0, 2.0, 0, 0, -1.0), (2.0, 473.0, 0, 0, -1.0),
                             (633.0, 473.0, 0, 0, -1.0)])
    grid = ref.assign_features_to_grid(kf)
    assert ref.get_features_in_area(kf, grid, 2.0, 2.0, 3.0) == [0]
    assert ref.get_features_in_area(kf, grid, 700.0, 2.0, 3.0) == []    # nMinCellX >= mnGridCols
    assert ref.get_features_in_area(kf, grid, -50.0, 2.0, 3.0) == []    # nMaxCellX < 0
    assert ref.get_features_in_area(kf, grid, 2.0, 700.0, 3.0) == []    # nMinCellY >= mnGridRows
    assert ref.get_features_in_area(kf, grid, 2.0, -50.0, 3.0) == []    # nMaxCellY < 0
    # without a level filter and with the strict |d| < r: 3 px away is outside a radius of 3
    assert ref.get_features_in_area(kf, grid, 5.0, 2.0, 3.0) == []
    assert ref.get_features_in_area(kf, grid, 4.5, 2.0, 3.0) == [0]


def test_fma32_rounds_once():
    """a * b + c whose double sum lands on a float32 midpoint only through its own rounding: rounding the
    double sum again gives the wrong neighbour; fma32 gives the exactly rounded value."""
    f32 = np.float32
    a, b = f32(1 + 2.0 ** -12), f32(1 + 2.0 ** -12)   # a * b = 1 + 2^-11 + 2^-24: a float32 midpoint
    c = f32(2.0 ** -60)                               # lifts the exact sum just above the midpoint
    twice = f32(float(a) * float(b) + float(c))       # the double sum drops c: the tie rounds to even
    exact = ref.round_fraction_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))
    assert exact == np.nextafter(twice, f32(2)) and ref.fma32(a, b, c) == exact
    assert ref.fma32(a, b, f32(-2.0 ** -60)) == twice
    v = ref.fma32(np.array([a, 2, 3], f32), np.array([b, 5, 7], f32), np.array([c, 1, -1], f32))
    assert v.dtype == np.float32 and v.tolist() == [float(exact), 11.0, 20.0]
    assert ref.round_fraction_f32(Fraction(2) ** -150) == 0 and ref.round_fraction_f32(Fraction(5, 2 ** 151)) == f32(2.0 ** -149)
    assert ref.round_fraction_f32(Fraction(2) ** 128) == f32(np.inf)


def test_arithmetic_matches_frustum_oracle(pkg, oracle):
    """Points that pass every test of Fuse and of isInFrustum: the reference's u, v, ur and predicted level
    equal the C++ oracle's (oracle/orb_frustum_oracle.cpp, the same contraction rules) bit for bit."""
    sc = fuse_scenes.make_scene(n_kfs=1, n_points=2500, seed=5, n_clutter=0, p_obs=0.0)
    kf, pts = sc["kfs"][0], sc["points"]
    _, _, reason, det = ref.fuse_search([kf], pts, 3.0)
    ff = pkg.frustum_frame(kf.Tcw, kf.Ow, (kf.fx, kf.fy, kf.cx, kf.cy), kf.mbf,
                           (kf.mnMinX, kf.mnMaxX, kf.mnMinY, kf.mnMaxY), fuse_scenes.SCALE, fuse_scenes.NLEVELS)
    o = oracle.is_in_frustum(ff, pts.pos, pts.normal, pts.min_dist, pts.max_dist, 0.5)
    both = (reason[0] >= ref.EMPTY_WINDOW) & (o["track_in_view"] != 0)
    assert both.sum() >= 1000, both.sum()
    proj = np.stack([det["u"][0], det["v"][0], det["ur"][0]], axis=1)[both]
    assert np.array_equal(proj.view(np.uint32), o["track_proj"][both].view(np.uint32))
    assert np.array_equal(det["level"][0][both], o["track_level"][both])
    assert len(np.unique(det["level"][0][both])) >= 4


def test_main_scene_conditions():
    """3 keyframes, 300 points, seed 0: every reason code occurs and at least 30 % of the unskipped jobs
    fuse; with ties and both chi-square branches exercised."""
    sc = fuse_scenes.make_scene(n_kfs=3, n_points=300, seed=0)
    idx, dist, reason, _ = ref.fuse_search(sc["kfs"], sc["points"], 3.0, sc["skip"])
    counts = np.bincount(reason.ravel(), minlength=len(ref.REASONS))
    assert (counts > 0).all(), dict(zip(ref.REASONS, counts))
    unskipped = reason != ref.SKIPPED
    assert (reason == ref.FUSED).sum() >= 0.3 * unskipped.sum()
    assert np.array_equal(idx >= 0, reason == ref.FUSED) and (dist[reason == ref.FUSED] <= ref.TH_LOW).all()
    assert (dist[reason == ref.ABOVE_TH_LOW] > ref.TH_LOW).all() and (dist[reason == ref.ABOVE_TH_LOW] < 256).all()
    for kf in sc["kfs"]:
        assert (kf.mvuRight >= 0).any() and (kf.mvuRight < 0).any()
    # A wider radius only turns empty windows into gated-out candidates: the chi-square gates (2.45 and 2.79
    # sigma of the keypoint's octave) are tighter than th = 3 scale factors of the predicted level.
    idx4, _, reason4, _ = ref.fuse_search(sc["kfs"], sc["points"], 4.0, sc["skip"])
    assert np.array_equal(idx4, idx)
    assert (reason4 == ref.EMPTY_WINDOW).sum() < (reason == ref.EMPTY_WINDOW).sum()
