"""GPU parity of loop closing's Sim3 searches (k_s3p_grid / k_s3p_search / k_s3p_resolve, reference
src/ORBmatcher.cc:496-619, :621-733, :1547-1651) against the Python restatement tests/sim3_projection_ref.py
(pinned by test_sim3_projection_ref_cpu.py).

Bar: every output integer -- matched, nmatches, best_idx, best_dist -- equals the restatement's, in every case.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import sim3_projection_ref as ref
import sim3_projection_scenes as scenes

pytestmark = pytest.mark.gpu

_CACHE: dict = {}


def main_scene():
    if "main" not in _CACHE:
        _CACHE["main"] = scenes.make_scene(0)
    return _CACHE["main"]


def assert_equal(got, want, what=""):
    for k in ("nmatches", "matched", "best_dist", "best_idx"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == np.int32 and g.shape == w.shape, (what, k, g.shape, w.shape)
        assert np.array_equal(g, w), f"{what}: {int((g != w).sum())} differing {k}"


def check(pkg, kfs, jobs, points, skip=None, taken0=None, what=""):
    """One host call against the restatement; returns (got, want)."""
    want = ref.run_jobs(kfs, jobs, points, skip, taken0)
    got = pkg.ORBmatcher().SearchByProjectionSim3(kfs, jobs, points, skip, taken0)
    assert_equal(got, want, what)
    return got, want


def concat_points(a, b):
    from orbslam3_amd.keyframe import FusePoints
    return FusePoints(*[np.concatenate([getattr(a, k), getattr(b, k)]) for k in ("pos", "normal", "min_dist", "max_dist", "desc")])


@pytest.mark.parametrize("flags", [False, True])
def test_three_modes(pkg, flags):
    sc = main_scene()
    jobs = scenes.three_mode_jobs(sc)
    n = sc["points"].n
    skip = np.tile(sc["skip"], 3) if flags else None
    taken0 = np.tile(sc["taken0"], (3, 1)) if flags else None
    got, want = check(pkg, [sc["kf"]], jobs, sc["points"], skip, taken0)
    print("nmatches", got["nmatches"].tolist())
    assert (want["nmatches"] >= 60).all() and (got["matched"][2] == -1).all()
    for b in (0, 1):  # the claims changed the result: the scene's displaced points
        assert ref.displacement(want["per_job"][b])[0].sum() >= 0.1 * want["nmatches"][b]
    assert n == 300


def test_flags_change_the_result(pkg):
    """skip and taken0 honoured: both runs equal the restatement, and they differ."""
    sc = main_scene()
    jobs = scenes.three_mode_jobs(sc)[:2]
    a, _ = check(pkg, [sc["kf"]], jobs, sc["points"])
    b, _ = check(pkg, [sc["kf"]], jobs, sc["points"], np.tile(sc["skip"], 2), np.tile(sc["taken0"], (2, 1)))
    assert (b["matched"][:, sc["taken0"] != 0] == -1).all() and (a["matched"][:, sc["taken0"] != 0] >= 0).any()
    assert (b["best_idx"][np.tile(sc["skip"], 2) != 0] == -1).all()
    assert not np.array_equal(a["best_idx"], b["best_idx"])


def test_project_against_invz(pkg):
    sc, jobs, i = scenes.project_vs_invz_scene()
    got, want = check(pkg, [sc["kf"]], jobs, sc["points"])
    n = sc["points"].n
    assert got["best_idx"][i] != got["best_idx"][n + i]


@pytest.mark.parametrize("n_kps", [12, 11])
def test_chain(pkg, n_kps):
    """A chain longer than any kept list: point i takes the i-th keypoint of the scan."""
    kf, pts, jobs = scenes.chain_scene(12, n_kps)
    got, want = check(pkg, [kf], jobs, pts)
    assert got["nmatches"][0] == n_kps and (got["best_idx"][:n_kps] >= 0).all() and (got["best_idx"][n_kps:] == -1).all()
    assert len(set(got["best_idx"][:n_kps].tolist())) == n_kps


CASES = scenes.hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_built(pkg, case):
    _, kf, pts, jobs, want_idx, _ = case
    got, _ = check(pkg, [kf], jobs, pts)
    o = got["offsets"]
    for b in range(len(jobs)):
        assert got["best_idx"][o[b]:o[b + 1]].tolist() == want_idx[b], b


def test_ratio(pkg):
    sc = main_scene()
    j = scenes.three_mode_jobs(sc)[0]
    jobs = [dict(j, ratio=1.0), dict(j, ratio=1.5), dict(j, mode=ref.CLAIM_INVZ, ratio=1.0)]
    got, _ = check(pkg, [sc["kf"]], jobs, sc["points"])
    assert got["nmatches"][1] > got["nmatches"][0]


def test_empty_and_gated_jobs(pkg):
    """A job without points and a job whose points all lie behind its camera, beside a plain one."""
    sc = main_scene()
    j = scenes.three_mode_jobs(sc)[1]
    behind = np.concatenate([np.eye(3), [[0.0], [0.0], [-100.0]]], axis=1).astype(np.float32)
    jobs = [dict(j, first=7, count=0), dict(j, Tcw=behind), j, dict(j, mode=ref.FUSE, Tcw=behind), dict(j, first=300, count=0)]
    got, want = check(pkg, [sc["kf"]], jobs, sc["points"])
    assert got["nmatches"].tolist() == [0, 0, int(want["nmatches"][2]), 0, 0] and got["nmatches"][2] > 60
    # nothing but empty jobs; no job at all
    got, _ = check(pkg, [sc["kf"]], [jobs[0], jobs[4]], sc["points"])
    assert got["best_idx"].shape == (0,) and (got["matched"] == -1).all()
    got = pkg.ORBmatcher().SearchByProjectionSim3([sc["kf"]], [], sc["points"])
    assert got["matched"].shape == (0, sc["kf"].N)


@pytest.mark.parametrize("n_clutter,cut", [(2000, 2048), (8300, None)])
def test_large_keyframe(pkg, n_clutter, cut):
    """More than 2,048 keypoints (the search reads the keyframe's records from global memory) against the same
    scene cut to 2,048 (the LDS path); more than 8,192 (the claims live in the job's matched row)."""
    for cap in (None, cut) if cut else (None,):
        sc = scenes.make_scene(4, n_points=200, n_clutter=n_clutter, kf_cap=cap)
        assert (sc["kf"].N > (2048 if cut else 8192)) if cap is None else sc["kf"].N == cut
        jobs = scenes.three_mode_jobs(sc)
        got, want = check(pkg, [sc["kf"]], jobs, sc["points"], np.tile(sc["skip"], 3), np.tile(sc["taken0"], (3, 1)),
                          what=f"N = {sc['kf'].N}")
        assert (want["nmatches"] >= 40).all()
        assert ref.displacement(want["per_job"][0])[0].sum() >= 5


def batch_scene():
    """Two keyframes, one pool holding both windows, five jobs: three share keyframe 0, two keyframe 1; poses
    from Sim3s of different scales; all three modes."""
    if "batch" not in _CACHE:
        a, b = main_scene(), scenes.make_scene(5, n_points=150)
        pool = concat_points(a["points"], b["points"])
        pa, pa2, pb = (scenes.candidate_pose(a["T"], 1.25), scenes.candidate_pose(a["T"], 0.8),
                       scenes.candidate_pose(b["T"], 1.1))
        jobs = [scenes.job(0, 0, 300, ref.CLAIM_INVZ, 8.0, 1.5, pa), scenes.job(1, 300, 150, ref.CLAIM_PROJECT, 5.0, 1.0, pb),
                scenes.job(0, 0, 300, ref.CLAIM_PROJECT, 3.0, 1.5, pa2), scenes.job(0, 30, 257, ref.FUSE, 4.0, 1.0, pa),
                scenes.job(1, 310, 31, ref.CLAIM_INVZ, 8.0, 1.5, pb)]
        kfs = [a["kf"], b["kf"]]
        T = sum(j["count"] for j in jobs)
        rng = np.random.default_rng(9)
        skip = (rng.random(T) < 0.05).astype(np.uint8)
        stride = max(k.N for k in kfs)
        taken0 = (rng.random((len(jobs), stride)) < 0.04).astype(np.uint8)
        _CACHE["batch"] = (kfs, jobs, pool, skip, taken0, ref.run_jobs(kfs, jobs, pool, skip, taken0))
    return _CACHE["batch"]


def test_batch_equals_single_calls(pkg):
    kfs, jobs, pool, skip, taken0, want = batch_scene()
    m = pkg.ORBmatcher()
    got = m.SearchByProjectionSim3(kfs, jobs, pool, skip, taken0)
    assert_equal(got, want, "batched")
    o = got["offsets"]
    for b, j in enumerate(jobs):
        one = m.SearchByProjectionSim3(kfs, [j], pool, skip[o[b]:o[b + 1]], taken0[b:b + 1])
        assert np.array_equal(one["matched"][0], got["matched"][b]) and one["nmatches"][0] == got["nmatches"][b], b
        assert np.array_equal(one["best_idx"], got["best_idx"][o[b]:o[b + 1]]), b
        assert np.array_equal(one["best_dist"], got["best_dist"][o[b]:o[b + 1]]), b


def device_frame(pkg, kf, cap, count=None):
    """kf as frame 0 of device arrays of capacity `cap`, with junk past the count."""
    import torch
    rng = np.random.default_rng(cap)
    pad = cap - kf.N
    k = np.concatenate([kf.mvKeysUn, kf.mvKeysUn[rng.integers(0, kf.N, pad)]])
    d = np.concatenate([kf.mDescriptors, kf.mDescriptors[rng.integers(0, kf.N, pad)]])  # junk that would match

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    return pkg.DeviceFrame(up(k.view(np.float32).reshape(1, cap, 7)), up(d.reshape(1, cap, 32)),
                           up(np.array([[kf.N if count is None else count, 0]], np.int32)), 0, kf.Tcw,
                           (kf.fx, kf.fy, kf.cx, kf.cy), kf.mvScaleFactors, kf.mvScaleFactors * kf.mvScaleFactors,
                           scenes.WIDTH, scenes.HEIGHT)


def test_device_entry(pkg):
    """The device entry equals the host entry (capacity past the counts, junk in the padding); a negative and an
    over-cap count give empty results for the jobs of those keyframes and leave the others intact."""
    import torch
    kfs, jobs, pool, skip, taken0, want = batch_scene()
    frames = [device_frame(pkg, kfs[0], 512), device_frame(pkg, kfs[1], 400), device_frame(pkg, kfs[1], 400, count=-3),
              device_frame(pkg, kfs[0], 512, count=513)]
    jobs = jobs + [dict(jobs[1], kf=2), dict(jobs[0], kf=3), dict(jobs[3], kf=3)]
    stride = 512
    tensors = tuple(torch.from_numpy(a).cuda() for a in (pool.pos, pool.normal, pool.min_dist, pool.max_dist, pool.desc))
    extra = sum(j["count"] for j in jobs[5:])
    sk = np.concatenate([skip, np.zeros(extra, np.uint8)])
    tk = np.zeros((len(jobs), stride), np.uint8)
    tk[:5, :taken0.shape[1]] = taken0
    got = pkg.ORBmatcher().SearchByProjectionSim3Device(frames, jobs, tensors, torch.from_numpy(sk).cuda(),
                                                        torch.from_numpy(tk).cuda(), stride=stride,
                                                        log_scale_factor=kfs[0].mfLogScaleFactor)
    torch.cuda.synchronize()
    got = {k: (v.cpu().numpy() if k != "offsets" else v) for k, v in got.items()}
    T = int(want["offsets"][-1])
    head = dict(matched=got["matched"][:5, :taken0.shape[1]], nmatches=got["nmatches"][:5], best_idx=got["best_idx"][:T],
                best_dist=got["best_dist"][:T])
    assert_equal(head, want, "device")
    assert (got["matched"][:5, taken0.shape[1]:] == -1).all()
    assert (got["matched"][5:] == -1).all() and (got["nmatches"][5:] == 0).all()
    assert (got["best_idx"][T:] == -1).all() and (got["best_dist"][T:] == 256).all()


def test_error_codes(pkg):
    """Out-of-range nlevels / capacities / counts / job fields: an error code, and nothing launched or written."""
    import torch
    from orbslam3_amd.keyframe import FusePointsView, Sim3ProjKfView
    from orbslam3_amd.tracking import FrameDeviceView, Sim3ProjKfDeviceView
    sc = main_scene()
    kf, pts = sc["kf"], sc["points"]
    lib, m = pkg._lib.load(), pkg.ORBmatcher()
    ARG, CAP = pkg._lib.ORB_ERR_ARG, pkg._lib.ORB_ERR_CAPACITY
    job = scenes.three_mode_jobs(sc)[0]
    N, n = kf.N, pts.n
    matched, cnt = np.full(N, -7, np.int32), np.full(1, -7, np.int32)
    idx, dist = np.full(n, -7, np.int32), np.full(n, -7, np.int32)

    def call(view=None, pv=None, n_kfs=1, n_jobs=1, stride=N, handle=True, **over):
        arr, _ = m._sim3_jobs([dict(job, **{k: v for k, v in over.items() if k in job})], 1)
        for k, v in over.items():
            if k not in job:
                setattr(arr[0], k, v)
        kv = (Sim3ProjKfView * 1)(view if view is not None else Sim3ProjKfView(kf.view(), kf.mfLogScaleFactor))
        return lib.orb_sim3_projection(m._handle() if handle else None, kv, n_kfs, arr, n_jobs,
                                       ctypes.byref(pts.view() if pv is None else pv), None, None, stride,
                                       matched.ctypes.data, cnt.ctypes.data, idx.ctypes.data, dist.ctypes.data)

    def kview(lsf=None, **over):
        v = Sim3ProjKfView(kf.view(), kf.mfLogScaleFactor if lsf is None else lsf)
        for k, val in over.items():
            setattr(v.frame, k, val)
        return v

    assert call(handle=False) == ARG
    assert call(n_kfs=-1) == ARG and call(n_jobs=-1) == ARG
    assert call(n_kfs=1025) == CAP and call(n_jobs=65536) == CAP
    assert call(stride=N - 1) == CAP and call(stride=0) == ARG
    assert call(kview(n=16385), stride=20000) == CAP and call(kview(n=-1)) == CAP
    for over in (dict(nlevels=0), dict(nlevels=13), dict(scale_factors=None), dict(desc=None), dict(kps_un=None)):
        assert call(kview(**over)) == ARG, over
    assert call(kview(lsf=0.0)) == ARG
    pv = pts.view()
    pv.n = (1 << 20) + 1
    assert call(pv=pv) == ARG
    pv = pts.view()
    pv.normal = None
    assert call(pv=pv) == ARG
    for over in (dict(kf=1), dict(kf=-1), dict(first=-1), dict(count=-1), dict(first=1, count=n), dict(first=n + 1, count=0),
                 dict(mode=3), dict(mode=-1), dict(th=0.0), dict(th=float("nan")), dict(th=float("inf")),
                 dict(ratio_hamming=0.0), dict(ratio_hamming=5.12), dict(ratio_hamming=float("nan"))):
        assert call(**over) == ARG, over
    assert b"Sim3 projection" in lib.orb_last_error()
    assert call(mode=ref.FUSE, ratio_hamming=float("nan")) == 0   # (Fuse does not read ratioHamming)
    matched[:], cnt[:], idx[:], dist[:] = -7, -7, -7, -7
    assert call(ratio_hamming=5.12) == ARG
    assert (matched == -7).all() and (cnt == -7).all() and (idx == -7).all() and (dist == -7).all()
    assert call() == 0
    want = ref.run_jobs([kf], [job], pts)
    assert np.array_equal(matched, want["matched"][0]) and cnt[0] == want["nmatches"][0]
    assert np.array_equal(idx, want["best_idx"]) and np.array_equal(dist, want["best_dist"])

    # the device entry: capacities, alignment, null arrays -- checked on the host before anything is enqueued
    frame = device_frame(pkg, kf, 512)
    tensors = tuple(torch.from_numpy(a).cuda() for a in (pts.pos, pts.normal, pts.min_dist, pts.max_dist, pts.desc))
    out = [torch.full((k,), -7, dtype=torch.int32, device="cuda") for k in (512, 1, n, n)]

    def dcall(stride=512, desc_offset=0, n_jobs=1, **over):
        v = (Sim3ProjKfDeviceView * 1)()
        ctypes.memmove(ctypes.byref(v[0].frame), ctypes.byref(frame.view()), ctypes.sizeof(FrameDeviceView))
        v[0].log_scale_factor = kf.mfLogScaleFactor
        for k, val in over.items():
            setattr(v[0].frame, k, val)
        arr, _ = m._sim3_jobs([job], 1)
        pv = FusePointsView(n, *[t.data_ptr() for t in tensors[:4]], tensors[4].data_ptr() + desc_offset)
        return lib.orb_sim3_projection_device(m._handle(), v, 1, arr, n_jobs, ctypes.byref(pv), None, None, stride,
                                              *[t.data_ptr() for t in out], None)

    assert dcall(cap=16385, stride=20000) == CAP and dcall(cap=0) == CAP and dcall(stride=511) == CAP
    assert dcall(desc=frame.view().desc + 1) == ARG and dcall(desc_offset=1) == ARG
    assert dcall(n=None) == ARG and dcall(nlevels=13) == ARG and dcall(n_jobs=65536) == CAP
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in out)  # nothing was launched by the rejected calls
    assert dcall() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy()[:N], want["matched"][0]) and out[1].item() == want["nmatches"][0]
    assert np.array_equal(out[2].cpu().numpy(), want["best_idx"]) and np.array_equal(out[3].cpu().numpy(), want["best_dist"])
