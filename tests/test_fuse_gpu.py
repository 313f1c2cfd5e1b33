"""GPU parity of ORBmatcher::Fuse's search (k_fuse_grid / k_fuse_search, reference src/ORBmatcher.cc:
1356-1506) against the Python restatement tests/fuse_ref.py (pinned by test_fuse_ref_cpu.py).

Bar: best_idx and best_dist equal the restatement bit for bit -- on the main scene (one and three keyframes,
mono and stereo, with and without skip flags, th 3 and 4), on the hand-built cases, on the shapes where the
kernel can go wrong (point counts around the 256-point block, empty / one-cell / off-grid keyframes, a
keyframe past the LDS-staged capacity), on the device entry with padded capacity and a flagged count, and
argument rejection.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import fuse_cases
import fuse_ref as ref
import fuse_scenes

pytestmark = pytest.mark.gpu

_SCENES: dict = {}


def main_scene(stereo: bool, th: float, with_skip: bool):
    """The main scene and its restatement for one parameter set, computed once."""
    key = (stereo, th, with_skip)
    if key not in _SCENES:
        sc = fuse_scenes.make_scene(n_kfs=3, n_points=300, seed=0, stereo=stereo)
        skip = sc["skip"] if with_skip else None
        _SCENES[key] = (sc, skip, ref.fuse_search(sc["kfs"], sc["points"], th, skip))
    return _SCENES[key]


def subset(points, n):
    from orbslam3_amd.keyframe import FusePoints
    return FusePoints(points.pos[:n], points.normal[:n], points.min_dist[:n], points.max_dist[:n], points.desc[:n])


def assert_equal(got, want, what=""):
    (gi, gd), (wi, wd) = got, want[:2]
    assert gi.dtype == np.int32 and gd.dtype == np.int32 and gi.shape == wi.shape
    assert np.array_equal(gd, wd), f"{what}: {int((gd != wd).sum())} differing best_dist"
    assert np.array_equal(gi, wi), f"{what}: {int((gi != wi).sum())} differing best_idx"


@pytest.mark.parametrize("th", [3.0, 4.0])
@pytest.mark.parametrize("with_skip", [False, True])
@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("n_kfs", [1, 3])
def test_main_scene(pkg, n_kfs, stereo, with_skip, th):
    sc, skip, want = main_scene(stereo, th, with_skip)
    got = pkg.ORBmatcher().Fuse(sc["kfs"][:n_kfs], sc["points"], th, None if skip is None else skip[:n_kfs])
    fused = int((want[0][:n_kfs] >= 0).sum())
    print(f"{n_kfs} keyframes, stereo {stereo}, skip {with_skip}, th {th}: {fused} fused")
    assert fused >= 60 * n_kfs
    assert_equal(got, (want[0][:n_kfs], want[1][:n_kfs]))


CASES = fuse_cases.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_built(pkg, case):
    _, kf, pts, th, want_idx, want_dist, _ = case
    idx, dist = pkg.ORBmatcher().Fuse(kf, pts, th)
    assert dist[0].tolist() == want_dist and idx[0].tolist() == want_idx
    assert_equal((idx, dist), ref.fuse_search([kf], pts, th))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_point_counts(pkg, n):
    """Point counts around the 256-point block (jobs are independent: the restatement's first n columns)."""
    sc, skip, want = main_scene(True, 3.0, True)
    idx, dist = pkg.ORBmatcher().Fuse(sc["kfs"][:2], subset(sc["points"], n), 3.0, skip[:2, :n])
    assert idx.shape == (2, n)
    assert_equal((idx, dist), (want[0][:2, :n], want[1][:2, :n]))
    idx2, _ = pkg.ORBmatcher().Fuse([], subset(sc["points"], n))  # no keyframe: nothing launched
    assert idx2.shape == (0, n)


def test_best_dist_optional(pkg):
    sc, skip, want = main_scene(True, 3.0, True)
    lib, m = pkg._lib.load(), pkg.ORBmatcher()
    views = (pkg.keyframe.FuseKfView * 1)(sc["kfs"][0].fuse_view())
    idx = np.full(300, -7, np.int32)
    rc = lib.orb_fuse(m._handle(), views, 1, ctypes.byref(sc["points"].view()), None, 3.0, idx.ctypes.data, None)
    assert rc == 0
    want_noskip = main_scene(True, 3.0, False)[2]
    assert np.array_equal(idx, want_noskip[0][0])


def test_degenerate_keyframes(pkg):
    """A keyframe without keypoints, one whose keypoints all fall in one grid cell, and one whose keypoints
    all round to cells outside the grid, side by side in one call."""
    rng = np.random.default_rng(3)
    pts = [fuse_cases.point(316 + 0.25 * i, 236 + 0.25 * ((7 * i) % 32), ones=int(rng.integers(0, 40))) for i in range(32)]
    P = fuse_cases.points_of(*pts)
    empty = fuse_cases.make_kf([])
    one_cell = fuse_cases.make_kf([(316 + 8 * rng.random(), 236 + 8 * rng.random(), int(rng.integers(0, 2)),
                                    int(rng.integers(0, 40)), -1.0) for _ in range(40)])
    outside = fuse_cases.make_kf([(636.0 + 3 * rng.random(), 476.0 + 3 * rng.random(), 0, 0, -1.0) for _ in range(10)]
                                 + [(-6.0, 240.0, 0, 0, -1.0)])
    grid = ref.assign_features_to_grid(one_cell)
    assert len(grid[32][24]) == 40 and sum(len(c) for col in ref.assign_features_to_grid(outside) for c in col) == 0
    kfs = [empty, one_cell, outside]
    want = ref.fuse_search(kfs, P, 3.0)
    assert (want[0][1] >= 0).sum() >= 16 and (want[0][[0, 2]] == -1).all() and (want[1][[0, 2]] == 256).all()
    assert_equal(pkg.ORBmatcher().Fuse(kfs, P, 3.0), want)


def test_large_keyframe_global_path(pkg):
    """One keyframe of ~4,000 keypoints (past the 2,048 records the search kernel stages in LDS: the
    global-memory walk runs) against 5,000 points: the reverse direction's shape in small."""
    sc = fuse_scenes.make_scene(n_kfs=1, n_points=5000, seed=11, n_clutter=200, p_obs=0.9, skip_fraction=0.05)
    kf = sc["kfs"][0]
    assert 3500 <= kf.N <= 16384, kf.N
    want = ref.fuse_search(sc["kfs"], sc["points"], 3.0, sc["skip"])
    print(f"{kf.N} keypoints, {int((want[0] >= 0).sum())} of 5000 fused")
    assert (want[0] >= 0).sum() >= 1000
    assert_equal(pkg.ORBmatcher().Fuse(sc["kfs"], sc["points"], 3.0, sc["skip"]), want)


def device_frame(pkg, kf, cap, count=None):
    """kf as frame 0 of device arrays of capacity `cap`, with junk past the count."""
    import torch
    rng = np.random.default_rng(cap)
    pad = cap - kf.N
    k = np.concatenate([kf.mvKeysUn, kf.mvKeysUn[rng.integers(0, kf.N, pad)]])
    d = np.concatenate([kf.mDescriptors, kf.mDescriptors[rng.integers(0, kf.N, pad)]])  # junk that would match
    ur = np.concatenate([kf.mvuRight, rng.uniform(0, 640, pad).astype(np.float32)])

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    return pkg.DeviceFrame(up(k.view(np.float32).reshape(1, cap, 7)), up(d.reshape(1, cap, 32)),
                           up(np.array([[kf.N if count is None else count, 0]], np.int32)), 0, kf.Tcw,
                           (kf.fx, kf.fy, kf.cx, kf.cy), kf.mvScaleFactors, kf.mvScaleFactors * kf.mvScaleFactors,
                           fuse_scenes.WIDTH, fuse_scenes.HEIGHT, bf=kf.mbf, u_right=up(ur.reshape(1, cap)))


def test_device_entry(pkg):
    """Capacity past the counts with junk in the padding; a negative and an over-cap count give -1 / 256 for
    that keyframe only."""
    import torch
    sc, skip, want = main_scene(True, 3.0, True)
    kfs, pts = sc["kfs"], sc["points"]
    frames = [device_frame(pkg, kfs[0], 512), device_frame(pkg, kfs[1], 400, count=-3),
              device_frame(pkg, kfs[2], 384), device_frame(pkg, kfs[1], 400, count=401)]
    Ow = np.stack([kfs[0].Ow, kfs[1].Ow, kfs[2].Ow, kfs[1].Ow])
    tensors = tuple(torch.from_numpy(a).cuda() for a in (pts.pos, pts.normal, pts.min_dist, pts.max_dist, pts.desc))
    sk = np.concatenate([skip, skip[1:2]])
    idx, dist = pkg.ORBmatcher().FuseDevice(frames, tensors, 3.0, torch.from_numpy(sk).cuda(), Ow=Ow,
                                            log_scale_factor=kfs[0].mfLogScaleFactor)
    torch.cuda.synchronize()
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert_equal((idx[[0, 2]], dist[[0, 2]]), (want[0][[0, 2]], want[1][[0, 2]]))
    assert (idx[[1, 3]] == -1).all() and (dist[[1, 3]] == 256).all()
    # no skip flags, one keyframe
    idx1, dist1 = pkg.ORBmatcher().FuseDevice(frames[:1], tensors, 3.0, Ow=Ow[:1], log_scale_factor=kfs[0].mfLogScaleFactor)
    torch.cuda.synchronize()
    want1 = main_scene(True, 3.0, False)[2]
    assert_equal((idx1.cpu().numpy(), dist1.cpu().numpy()), (want1[0][:1], want1[1][:1]))


def test_argument_rejection(pkg):
    sc, _, _ = main_scene(True, 3.0, True)
    lib, m = pkg._lib.load(), pkg.ORBmatcher()
    kf, pts = sc["kfs"][0], sc["points"]
    ARG = pkg._lib.ORB_ERR_ARG
    idx = np.zeros(300, np.int32)

    def call(view, pv, th=3.0, n_kfs=1, out=idx.ctypes.data, handle=None):
        arr = (pkg.keyframe.FuseKfView * 1)(view)
        return lib.orb_fuse(m._handle() if handle is None else handle, arr, n_kfs, ctypes.byref(pv), None, th, out, None)

    assert call(kf.fuse_view(), pts.view()) == 0
    assert lib.orb_fuse(None, None, 1, ctypes.byref(pts.view()), None, 3.0, idx.ctypes.data, None) == ARG
    assert lib.orb_fuse(m._handle(), None, 1, ctypes.byref(pts.view()), None, 3.0, idx.ctypes.data, None) == ARG
    assert call(kf.fuse_view(), pts.view(), n_kfs=-1) == ARG
    assert call(kf.fuse_view(), pts.view(), out=None) == ARG
    for th in (0.0, -1.0, float("nan"), float("inf")):
        assert call(kf.fuse_view(), pts.view(), th=th) == ARG
    pv = pts.view()
    pv.n = -1
    assert call(kf.fuse_view(), pv) == ARG
    pv.n = (1 << 20) + 1
    assert call(kf.fuse_view(), pv) == ARG
    pv = pts.view()
    pv.normal = None
    assert call(kf.fuse_view(), pv) == ARG
    for field, value in (("n", -1), ("n", 16385), ("nlevels", 0), ("nlevels", 13), ("desc", None), ("scale_factors", None)):
        v = kf.fuse_view()
        setattr(v.frame, field, value)
        assert call(v, pts.view()) == ARG, field
    v = kf.fuse_view()
    v.inv_level_sigma2 = None
    assert call(v, pts.view()) == ARG
    v = kf.fuse_view()
    v.log_scale_factor = 0.0
    assert call(v, pts.view()) == ARG
    assert b"Fuse" in lib.orb_last_error()
    # an empty point set or no keyframe is ORB_OK whatever else is passed
    pv = pts.view()
    pv.n = 0
    assert lib.orb_fuse(m._handle(), None, 0, ctypes.byref(pts.view()), None, 3.0, None, None) == 0
    assert call(kf.fuse_view(), pv, out=None) == 0
    # the device entry: no keyframe array, too many keyframes, a capacity past 16384, unaligned descriptors,
    # a bad th (checked on the host before anything is enqueued; the pointers are device tensors)
    import torch
    from orbslam3_amd.keyframe import FusePointsView
    from orbslam3_amd.tracking import FrameDeviceView, FuseKfDeviceView
    assert lib.orb_fuse_device(m._handle(), None, 1, ctypes.byref(pts.view()), None, 3.0, idx.ctypes.data, None, None) == ARG
    frame = device_frame(pkg, kf, 512)
    tensors = tuple(torch.from_numpy(a).cuda() for a in (pts.pos, pts.normal, pts.min_dist, pts.max_dist, pts.desc))
    out = torch.full((300,), -7, dtype=torch.int32, device="cuda")

    def dview(**over):
        v = (FuseKfDeviceView * 1)()
        ctypes.memmove(ctypes.byref(v[0].frame), ctypes.byref(frame.view()), ctypes.sizeof(FrameDeviceView))
        v[0].Ow[:] = [float(x) for x in kf.Ow]
        v[0].inv_level_sigma2 = frame.mvInvLevelSigma2.ctypes.data
        v[0].log_scale_factor = kf.mfLogScaleFactor
        for k, val in over.items():
            setattr(v[0].frame, k, val)
        return v

    def dcall(v, desc_offset=0, th=3.0, n_kfs=1):
        pv = FusePointsView(300, *[t.data_ptr() for t in tensors[:4]], tensors[4].data_ptr() + desc_offset)
        return lib.orb_fuse_device(m._handle(), v, n_kfs, ctypes.byref(pv), None, th, out.data_ptr(), None, None)

    assert dcall(dview(cap=16385)) == ARG
    assert dcall(dview(cap=0)) == ARG
    assert dcall(dview(desc=frame.view().desc + 1)) == ARG
    assert dcall(dview(), desc_offset=1) == ARG
    assert dcall(dview(), n_kfs=65536) == ARG
    assert dcall(dview(), th=0.0) == ARG
    torch.cuda.synchronize()
    assert (out == -7).all()  # nothing was launched by the rejected calls
    assert dcall(dview()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), main_scene(True, 3.0, False)[2][0][0])
