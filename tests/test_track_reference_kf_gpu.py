"""Tracking::TrackReferenceKeyFrame on the device (tracking.TrackReferenceKeyFrame /
orb_track_reference_kf_device, reference src/Tracking.cc:3931-4000) against the same steps composed on the
CPU: SearchByBoW from tests/bow_search_ref.py, PoseOptimization's graph as orb_tracking_pose_edges_device
documents it (oracle.tracking_chain.pose_graph), oracle.pose_optimization, and a numpy outlier discard.

Bar: matches, graph, outlier flags, the discard's counts and the status word exact; the pose within
PoseOptimization's 1e-6."""
from __future__ import annotations

import numpy as np
import pytest

import bow_search_ref as ref
from bow_search_scenes import device_keyframe

pytestmark = pytest.mark.gpu

FAIL_BOW, FAIL_MAP = 8, 16
POSE_LAST = np.array([0, 0, 0, 0, 0, 0, 1.0])  # mLastFrame.GetPose(): the scene's last frame sits at the origin


def _setup(pkg, synth, observed_zero=False, **scene_kw):
    """(device inputs, host frames, expected result) for one scene."""
    import torch
    from oracle import oracle, tracking_chain
    sc = synth.tracking_chain_scene(n_points=400, seed=81, clutter=80, **scene_kw)
    voc = synth.SyntheticVocabulary(201)
    C, L = pkg.Frame(**sc["cur"]), pkg.Frame(**sc["last"])
    mp = L.map_points
    usable = np.asarray(mp["valid"], np.uint8)
    observed = np.zeros(L.N, np.uint8) if observed_zero else np.asarray(mp["observed"], np.uint8)
    xyz = np.asarray(mp["xyz"], np.float32)

    def as_kf(F, flags):
        return pkg.KeyFrame(F.mvKeysUn, F.mDescriptors, F.Tcw, (F.fx, F.fy, F.cx, F.cy), F.mvScaleFactors,
                            sc["level_sigma2"], has_mappoint=flags, feat_vec=voc.transform(F.mDescriptors))
    ref_kf, cur_kf = as_kf(L, usable), as_kf(C, None)
    # expected: the reference's steps in order
    n, m = ref.search_by_bow_kf(ref_kf, cur_kf, usable, 0.7, True)
    exp = dict(n_match=n, m_raw=m)
    if n < 15:  # :3946-3950
        exp.update(status=FAIL_BOW, match=m, n_edges=0, pose=POSE_LAST, n_kept=0, n_map=0)
    else:
        fr, e, kp = tracking_chain.pose_graph(C, POSE_LAST, sc["level_sigma2"], m, xyz)
        P, O, I = oracle.pose_optimization(fr, e)
        md = m.copy()
        md[kp[O]] = -1  # :3973-3989
        kept = md >= 0
        n_map = int((observed[md[kept]] != 0).sum())  # :3990-3992
        exp.update(match=md, n_edges=len(e), edges=e, edge_kp=kp, outlier=O, pose=P[0], inliers=int(I[0]),
                   n_kept=int(kept.sum()), n_map=n_map, status_map=FAIL_MAP if n_map < 10 else 0)
    # device staging: capacities past the counts
    cap_k, cap_f = L.N + 21, C.N + 38
    dev = torch.device("cuda")

    def up(a, dt, pad, fill):
        a = np.asarray(a, dt)
        return torch.from_numpy(np.concatenate([a, np.full((pad,) + a.shape[1:], fill, dt)])).to(dev)
    d = dict(ref=device_keyframe(pkg, ref_kf, cap_k), cur_bow=device_keyframe(pkg, cur_kf, cap_f),
             point_ok=up(usable, np.uint8, cap_k - L.N, 1), observed=up(observed, np.uint8, cap_k - L.N, 1),
             xyz=up(xyz, np.float32, cap_k - L.N, 1.0))
    kps, desc, counts = d["cur_bow"]._keep[:3]
    ur = None if C.mvuRight is None else up(C.mvuRight, np.float32, cap_f - C.N, 100.0).reshape(1, cap_f)
    d["cur"] = pkg.DeviceFrame(kps, desc, counts, 0, C.Tcw, sc["cur"]["camera"], C.mvScaleFactors, sc["level_sigma2"],
                               int(C.mnMaxX), int(C.mnMaxY), C.mbf, ur)
    return d, C, exp, sc


def _run(pkg, d, imu=False):
    trk = pkg.TrackReferenceKeyFrame(d["cur"].cap, imu=imu)
    return trk.track(d["ref"], d["point_ok"], d["observed"], d["xyz"], d["cur_bow"], d["cur"], POSE_LAST).sync()


def _check_graph(r, exp, C):
    assert r["n_match"] == exp["n_match"]
    assert int(r["frame"][0]["n_edges"]) == exp["n_edges"]
    assert np.array_equal(r["edges"].view(np.uint8), exp["edges"].view(np.uint8))
    assert np.array_equal(r["edge_kp"], exp["edge_kp"])
    assert np.array_equal(r["outlier"], exp["outlier"])
    assert np.array_equal(r["match"][:C.N], exp["match"]) and (r["match"][C.N:] == -1).all()
    assert (r["n_kept"], r["n_map"], r["inliers"]) == (exp["n_kept"], exp["n_map"], exp["inliers"])
    err = np.abs(r["pose"] - exp["pose"]).max()
    print(f"n_match {r['n_match']}, edges {exp['n_edges']}, outliers {int(exp['outlier'].sum())}, kept {r['n_kept']}, "
          f"map {r['n_map']}, pose error {err:.3e}")
    assert err < 1e-6


def test_tracked(pkg, oracle, synth):
    d, C, exp, sc = _setup(pkg, synth)
    assert exp["n_match"] >= 50 and exp["outlier"].sum() > 0 and exp["n_map"] < exp["n_kept"]
    r = _run(pkg, d)
    _check_graph(r, exp, C)
    assert r["status"] == exp["status_map"] == 0
    # the fallback tracked: the pose moved from the last frame's to the truth
    t = sc["pose7_true"]
    assert np.abs(r["pose"][:3] - t[:3]).max() < 0.01 < np.abs(POSE_LAST[:3] - t[:3]).max()


def test_too_few_bow_matches(pkg, oracle, synth):
    """tracked_frac 0.08: SearchByBoW finds fewer than 15 -> ORB_TRACK_REF_FAIL_BOW, no graph, the pose is the
    input pose and the matches stay as the search left them."""
    d, C, exp, _ = _setup(pkg, synth, tracked_frac=0.08)
    assert 0 < exp["n_match"] < 15
    r = _run(pkg, d)
    assert r["status"] == FAIL_BOW == exp["status"]
    assert r["n_match"] == exp["n_match"] and int(r["frame"][0]["n_edges"]) == 0 and len(r["edges"]) == 0
    assert np.array_equal(r["pose"], POSE_LAST)
    assert np.array_equal(r["match"][:C.N], exp["m_raw"])
    assert (r["n_kept"], r["n_map"], r["inliers"]) == (0, 0, 0)


def test_no_observed_map_points_and_imu(pkg, oracle, synth):
    """Every matched map point without observations: nmatchesMap 0 < 10 -> ORB_TRACK_REF_FAIL_MAP; with an IMU
    sensor the final test is skipped (src/Tracking.cc:3996-3997) and the same frame counts as tracked."""
    d, C, exp, _ = _setup(pkg, synth, observed_zero=True)
    assert exp["n_map"] == 0 and exp["status_map"] == FAIL_MAP and exp["n_kept"] >= 10
    r = _run(pkg, d)
    _check_graph(r, exp, C)
    assert r["status"] == FAIL_MAP
    r = _run(pkg, d, imu=True)
    _check_graph(r, exp, C)
    assert r["status"] == 0
