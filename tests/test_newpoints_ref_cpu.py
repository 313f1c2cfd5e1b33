"""CPU tests of CreateNewMapPoints' triangulation half that need no GPU: the restatement
(tests/newpoints_ref.py) on the hand-built cases against values worked out by hand, the decisiveness cap of
the random scene, the kernel's 4x4 null-vector routine (csrc/orb_svd4.h) compiled for the host against the
accuracy bound the GPU test sets, and the new entries' host-side argument rejection."""
from __future__ import annotations

import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import newpoints_ref as ref
import newpoints_scenes as scenes

ROOT = pathlib.Path(__file__).resolve().parents[1]
BUILD = ROOT / "build" / "tests"
CASES = scenes.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_case_against_hand_values(case):
    rows = ref.truth_all(case.kf1, case.kf2s, case.m12, case.prm, case.n_matches)
    status = np.array([[t["status"] for t in row] for row in rows])
    resolved, taken, order = ref.resolve(status)
    assert resolved.tolist() == case.status
    assert [[t["from_stereo"] for t in row] for row in rows] == case.from_stereo
    assert [[t["branch"] for t in row] for row in rows] == case.branch
    for (p, i), want in case.x3d.items():
        got = rows[p][i]["x3d"]
        assert np.linalg.norm(got - np.array(want)) <= 1e-4 * want[2], (p, i, got, want)
    # wide margins: the float32 gates at the rounded position agree with the float64 walk
    for p, row in enumerate(rows):
        for i, t in enumerate(row):
            assert t["margin"] > 5e-5  # (the band between 0.9996 and 0.9998 allows 1e-4 at the most)
            if t["x3d"] is not None:
                assert ref.gates32(case.kf1, case.kf2s[p], i, int(case.m12[p, i]), t["x3d"].astype(np.float32),
                                   case.prm) == t["status"]
    # creation order: p ascending, then idx1 ascending; an idx1 at most once
    assert order == sorted(order) and len({i for _, i in order}) == len(order)
    assert all(resolved[p, i] == ref.NP_OK and taken[i] == p for p, i in order)


def test_hand_cases_reach_every_status():
    reached = {s for c in CASES for row in c.status for s in row}
    assert reached == set(range(13))
    branches = {b for c in CASES for row in c.branch for b in row}
    assert branches == set(range(5))


def test_record_by_hand():
    """UpdateNormalAndDepth of a point 5 m in front of keyframe 1 (octave 2) seen from 0.5 m to the right."""
    kf1 = scenes.make_kf(scenes.T0, [scenes.obs(scenes.T0, (0, 0, 5.0), octave=2)])
    Ta = scenes.pose((0.5, 0, 0))
    kf2 = scenes.make_kf(Ta, [scenes.obs(Ta, (0, 0, 5.0))])
    normal, mn, mx = ref.record64(kf1, kf2, 0, (0, 0, 5.0))
    d2 = np.hypot(0.5, 5.0)
    assert np.allclose(normal, [(-0.5 / d2) / 2, 0, (1 + 5.0 / d2) / 2], atol=1e-12)
    assert np.isclose(mx, 5.0 * 1.44, rtol=1e-6) and np.isclose(mn, 5.0 * 1.44 / 1.2 ** 7, rtol=1e-6)


def test_random_scene_decisive_share():
    """At most 2 % of the matched jobs may have a cos-parallax comparison within 1e-5 of a tie (float64): the
    seed is chosen so that this holds, and the branches and outcomes the GPU tests rely on are all present."""
    sc = scenes.random_truth()
    matched, decisive = sc["matched"], sc["decisive"]
    share = 1.0 - decisive.sum() / matched.sum()
    branch = np.array([[t["branch"] for t in row] for row in sc["truth"]])
    status = np.array([[t["status"] for t in row] for row in sc["truth"]])
    print(f"{int(matched.sum())} matched jobs, {100 * share:.2f} % non-decisive; branches "
          f"{np.bincount(branch[matched], minlength=5).tolist()}; statuses {np.bincount(status[matched], minlength=12).tolist()}")
    assert matched.sum() >= 600 and share <= 0.02
    assert all((branch[matched] == b).sum() >= 20 for b in (ref.BRANCH_TRI, ref.BRANCH_STEREO1, ref.BRANCH_STEREO2))
    assert (status == ref.NP_OK).sum() >= 300
    resolved, taken, order = ref.resolve(status)
    assert (resolved == ref.NP_TAKEN).sum() >= 50 and len(order) > 256  # the scan crosses blocks and pairs
    assert len({p for p, _ in order}) == len(sc["kf2s"])


def test_host_svd4_accuracy():
    """The kernel's null-vector routine, compiled for the host, on the A of every triangulated job of the random
    scene: its error against the float64 SVD of the same float32 A is at most 4x that of LAPACK's float32 sgesdd, in
    the maximum and in the median (the bound of tests/test_newpoints_gpu.py)."""
    sc = scenes.random_truth()
    As = np.array([t["A"] for row in sc["truth"] for t in row if t["A"] is not None], np.float32)
    assert len(As) >= 100
    xh = np.zeros((len(As), 4), np.float32)
    ref.host_svd4().svd4_null_vectors(np.ascontiguousarray(As).ctypes.data, len(As), xh.ctypes.data)
    assert np.allclose(np.linalg.norm(xh.astype(np.float64), axis=1), 1.0, atol=1e-5)
    X = xh[:, :3] / xh[:, 3:4]
    Ow1 = ref.center(sc["kf1"])
    err = ref.triangulation_errors(As, X, Ow1)
    yard = ref.triangulation_errors(As, ref.yardstick_x3d(As), Ow1)
    print(f"{len(As)} matrices: host Jacobi max {err.max():.3e} median {np.median(err):.3e}; "
          f"sgesdd float32 max {yard.max():.3e} median {np.median(yard):.3e}")
    assert err.max() <= 4 * yard.max() and np.median(err) <= 4 * np.median(yard)
    # the exact cases: a diagonal A gives the unit vector of its smallest entry
    d = np.diag([-1.0, -1.5, 2.0, 2.0]).astype(np.float32)[None]
    out = np.zeros((1, 4), np.float32)
    ref.host_svd4().svd4_null_vectors(d.ctypes.data, 1, out.ctypes.data)
    assert out.tolist() == [[1.0, 0.0, 0.0, 0.0]]


def test_entries_reject_bad_arguments(pkg):
    """No device work: NULL handles, views, parameters and outputs give ORB_ERR_ARG."""
    from orbslam3_amd import _lib
    lib = _lib.load()
    assert lib.orb_create_new_map_points(None, None, None, 1, None, None, None, None) == _lib.ORB_ERR_ARG
    assert lib.orb_create_new_map_points_device(None, None, None, 1, None, None, None, None, None) == _lib.ORB_ERR_ARG
    assert {"orb_create_new_map_points", "orb_create_new_map_points_device"} <= set(_lib.header_symbols()) & set(_lib.PROTOTYPES)
    assert pkg.keyframe.NEWPOINT_DTYPE.itemsize == 48
    assert ctypes.sizeof(pkg.keyframe.NewPointsKfExtra) == 96 and ctypes.sizeof(pkg.keyframe.NewPointsOut) == 48
