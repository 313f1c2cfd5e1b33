"""Pins tests/sim3_projection_ref.py, the Python restatement of loop closing's three Sim3 searches (reference
src/ORBmatcher.cc:496-619, :621-733, :1547-1651) that the GPU tests compare against, and the scenes of
tests/sim3_projection_scenes.py: the hand-built cases, whose expected values follow from the reference's
statements; the Fuse form against tests/fuse_ref.py with its chi-square gate switched off; and the properties
that keep the GPU tests from passing vacuously."""
from __future__ import annotations

import numpy as np
import pytest

import fuse_ref
import sim3_projection_ref as ref
import sim3_projection_scenes as scenes

CASES = scenes.hand_cases()
MAIN_SEED = 0


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_built(case):
    _, kf, pts, jobs, want_idx, want_reason = case
    r = ref.run_jobs([kf], jobs, pts)
    for b in range(len(jobs)):
        s = slice(int(r["offsets"][b]), int(r["offsets"][b + 1]))
        assert r["reason"][s].tolist() == want_reason[b], (b, [ref.REASONS[x] for x in r["reason"][s]])
        assert r["best_idx"][s].tolist() == want_idx[b], b
        assert r["nmatches"][b] == sum(x >= 0 for x in want_idx[b])


def check_not_vacuous(r, claim: bool, what):
    counts = np.bincount(r["reason"], minlength=len(ref.REASONS))
    assert (counts > 0).all(), (what, dict(zip(ref.REASONS, counts)))
    if not claim:
        return
    displaced, depth = ref.displacement(r)
    matched = int((r["best_idx"] >= 0).sum())
    print(f"{what}: {matched} matched, {int(displaced.sum())} displaced, longest chain {int(depth.max())}")
    assert matched >= 60 and displaced.sum() >= 0.1 * matched, (what, matched, int(displaced.sum()))
    assert depth.max() >= 3, (what, int(depth.max()))


@pytest.mark.parametrize("mode", [ref.CLAIM_PROJECT, ref.CLAIM_INVZ, ref.FUSE])
def test_main_scene_conditions(mode):
    """Every reason code occurs; in the claim forms at least 10 % of the matched points took a keypoint that
    was not their first choice (an earlier point had claimed it) and some chain of such displacements is at
    least three points long.  With and without the skip / taken0 flags."""
    sc = scenes.make_scene(MAIN_SEED)
    j = scenes.three_mode_jobs(sc)[mode]
    kf, P = sc["kf"], sc["points"]
    r = ref._search(kf, j["Tcw"], j["Ow"], P, 0, P.n, mode, j["th"], j["ratio"], sc["skip"],
                    None if mode == ref.FUSE else sc["taken0"])
    check_not_vacuous(r, mode != ref.FUSE, f"mode {mode}")
    assert np.array_equal(r["best_idx"] >= 0, r["reason"] == ref.MATCHED)
    assert r["nmatches"] == (r["best_idx"] >= 0).sum()
    if mode != ref.FUSE:
        m = r["matched"]
        assert (m[sc["taken0"] != 0] == -1).all() and (m >= 0).sum() == r["nmatches"]
        assert np.array_equal(np.sort(r["best_idx"][r["best_idx"] >= 0]), np.flatnonzero(m >= 0))
        plain = ref._search(kf, j["Tcw"], j["Ow"], P, 0, P.n, mode, j["th"], j["ratio"], None, None)
        check_not_vacuous(dict(plain, reason=np.append(plain["reason"], ref.SKIPPED)), True, f"mode {mode}, no flags")
        assert not np.array_equal(plain["best_idx"], r["best_idx"])


def test_ratio_changes_the_result():
    sc = scenes.make_scene(MAIN_SEED)
    kf, P = sc["kf"], sc["points"]
    j = scenes.three_mode_jobs(sc)[0]
    a = ref.search_by_projection(kf, j["Tcw"], j["Ow"], P, 0, P.n, j["th"], 1.0)
    b = ref.search_by_projection(kf, j["Tcw"], j["Ow"], P, 0, P.n, j["th"], 1.5)
    assert b["nmatches"] > a["nmatches"] and (a["best_dist"][a["best_idx"] >= 0] <= 50).all()
    assert ((b["best_dist"] > 50) & (b["best_dist"] <= 75)).any()


@pytest.mark.parametrize("n_kps", [12, 11])
def test_chain(n_kps):
    """Twelve identical points over twelve (eleven) identical keypoints in one window: point i takes the i-th
    keypoint of GetFeaturesInArea's scan, the twelfth point of eleven keypoints nothing."""
    kf, pts, jobs = scenes.chain_scene(12, n_kps)
    scan = fuse_ref.get_features_in_area(kf, fuse_ref.assign_features_to_grid(kf), 320.0, 240.0, 8.0)
    assert len(scan) == n_kps and scan != sorted(scan) and scan != sorted(scan, reverse=True)
    r = ref.run_jobs([kf], jobs, pts)
    assert r["best_idx"].tolist() == (scan + [-1])[:12]
    assert r["nmatches"][0] == n_kps and (r["best_dist"][:n_kps] == 0).all()


def test_project_against_invz():
    sc, jobs, i = scenes.project_vs_invz_scene()
    r = ref.run_jobs([sc["kf"]], jobs, sc["points"])
    o = r["offsets"]
    a, b = r["best_idx"][o[0]:o[1]], r["best_idx"][o[1]:o[2]]
    assert a[i] != b[i] and sc["kf"].N - 1 in (a[i], b[i]) and -1 in (a[i], b[i]), (a[i], b[i])
    ua, ub = r["per_job"][0]["u"][i], r["per_job"][1]["u"][i]
    assert ua != ub and abs(float(ua) - float(ub)) == float(np.spacing(min(ua, ub)))


def test_fuse_form_against_fuse_ref():
    """The Fuse form is fuse_ref's search without the chi-square gate and u_R: with mvInvLevelSigma2 = 0 the
    gate of fuse_ref never rejects, and the two restatements agree on every point."""
    sc = scenes.make_scene(MAIN_SEED)
    kf, P = sc["kf"], sc["points"]
    j = scenes.three_mode_jobs(sc)[ref.FUSE]
    r = ref.fuse(kf, j["Tcw"], j["Ow"], P, 0, P.n, j["th"], sc["skip"])
    from orbslam3_amd.keyframe import Frame
    kf2 = Frame(kf.mvKeysUn, kf.mDescriptors, j["Tcw"], scenes.CAMERA, kf.mvScaleFactors, scenes.WIDTH, scenes.HEIGHT,
                Ow=j["Ow"], inv_level_sigma2=np.zeros(len(kf.mvScaleFactors), np.float32),
                log_scale_factor=kf.mfLogScaleFactor)
    idx, dist, reason, _ = fuse_ref.fuse_search([kf2], P, j["th"], sc["skip"][None, :])
    assert np.array_equal(idx[0], r["best_idx"]) and np.array_equal(dist[0], r["best_dist"])
    assert np.array_equal(reason[0] == fuse_ref.FUSED, r["reason"] == ref.MATCHED)


def test_sim3_pose():
    """Tcw = [R | t / s], Ow = -R^T (t / s), float32: the projection does not depend on the map scale."""
    from orbslam3_amd.matcher import sim3_pose
    sc = scenes.make_scene(MAIN_SEED)
    T = sc["T"]
    Tcw, Ow = sim3_pose(T[:, :3], 2.0 * T[:, 3], 2.0)
    assert Tcw.dtype == np.float32 and Ow.dtype == np.float32 and Tcw.shape == (3, 4) and Ow.shape == (3,)
    assert np.array_equal(Tcw, T.astype(np.float32))   # a power of two scales exactly
    assert np.allclose(Ow, -T[:, :3].T @ T[:, 3], atol=1e-6)
