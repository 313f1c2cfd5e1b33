"""GPU tests of the triangulation half of LocalMapping::CreateNewMapPoints (k_np_triangulate / k_np_resolve /
k_np_emit, reference src/LocalMapping.cc:626-910) against tests/newpoints_ref.py (pinned by
test_newpoints_ref_cpu.py) on tests/newpoints_scenes.py.

Bars:
  branch, from_stereo    equal the float64 restatement on every hand case and every decisive random job
  stereo x3D             |dx| <= 1e-6 (|x| + |Ow|) against float64 (three-term float sums)
  triangulated x3D       error = |x - x64| / |x64 - Ow1| against the float64 SVD of the same float32 A; the
                         kernel's maximum and median over the scene at most 4x those of LAPACK's float32 sgesdd
                         (scipy.linalg.svd; np.linalg.svd computes float32 input in double).  Measured on the
                         MI355X: kernel max 1.128e-06 median 1.283e-07, sgesdd max 6.564e-06 median 5.297e-07
                         over 511 jobs
  gates after x3D        the float32 restatement at the device's x3D gives the device's status for every job
  resolve                taken_by, TAKEN, order and count of the records as the restatement's resolve of the
                         device's statuses; normal to 1e-6 absolute, distances to 1e-6 relative
  chain                  SearchForTriangulationDevice -> CreateNewMapPointsDevice with no host copy equals the
                         host entry on the downloaded matches
  early stop             the records with p < 1 equal a call with one neighbour
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import newpoints_ref as ref
import newpoints_scenes as scenes

pytestmark = pytest.mark.gpu

CASES = scenes.cases()
_OUT: dict = {}


def run(pkg, kf1, kf2s, m12, prm, n_matches=None):
    return pkg.ORBmatcher(0.6, False).CreateNewMapPoints(kf1, kf2s, m12, n_matches, prm.inertial, prm.far_points,
                                                         float(prm.th_far_points), float(prm.ratio_factor))


def random_out(pkg):
    """The device's result on the random scene, computed once."""
    if not _OUT:
        sc = scenes.random_truth()
        _OUT.update(run(pkg, sc["kf1"], sc["kf2s"], sc["m12"], sc["prm"]))
    return scenes.random_truth(), _OUT


def untaken(status):
    return np.where(status == ref.NP_TAKEN, ref.NP_OK, status)


def device_branch(status, from_stereo):
    """What a status / from_stereo pair says about the branch: none, low parallax, triangulated or stereo."""
    if status == ref.NP_NO_MATCH:
        return "none"
    if status == ref.NP_LOW_PARALLAX:
        return "low"
    return "stereo" if from_stereo else "tri"


BRANCH_NAME = {ref.BRANCH_NONE: "none", ref.BRANCH_LOW: "low", ref.BRANCH_TRI: "tri", ref.BRANCH_STEREO1: "stereo",
               ref.BRANCH_STEREO2: "stereo"}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_built(pkg, case):
    out = run(pkg, case.kf1, case.kf2s, case.m12, case.prm, case.n_matches)
    assert out["status"].tolist() == case.status
    assert out["from_stereo"].tolist() == case.from_stereo
    rows = ref.truth_all(case.kf1, case.kf2s, case.m12, case.prm, case.n_matches)
    for p, row in enumerate(rows):
        for i, t in enumerate(row):
            assert device_branch(out["status"][p, i], out["from_stereo"][p, i]) == BRANCH_NAME[t["branch"]]
            if t["x3d"] is not None:  # (also tells stereo 1 from stereo 2: their unprojections differ)
                scale = np.linalg.norm(t["x3d"]) + np.linalg.norm(ref.center(case.kf1))
                assert np.linalg.norm(out["x3d"][p, i] - t["x3d"]) <= 2e-6 * max(scale, 1.0), (p, i)
    for (p, i), want in case.x3d.items():
        assert np.linalg.norm(out["x3d"][p, i] - np.array(want)) <= 1e-4 * want[2]
    resolved, taken, order = ref.resolve(untaken(out["status"]))
    assert out["taken_by"].tolist() == taken.tolist()
    assert [(int(r["p"]), int(r["idx1"])) for r in out["new"]] == order
    assert [int(r["idx2"]) for r in out["new"]] == [int(case.m12[p, i]) for p, i in order]


def test_branch_and_from_stereo(pkg):
    sc, out = random_out(pkg)
    bad = []
    for p, row in enumerate(sc["truth"]):
        for i, t in enumerate(row):
            if sc["decisive"][p, i] or not sc["matched"][p, i]:
                got = device_branch(out["status"][p, i], out["from_stereo"][p, i])
                if got != BRANCH_NAME[t["branch"]] or int(out["from_stereo"][p, i]) != t["from_stereo"]:
                    bad.append((p, i, got, t["branch"]))
    print(f"{int(sc['decisive'].sum())} decisive jobs of {int(sc['matched'].sum())} matched")
    assert not bad, bad[:10]


def test_stereo_x3d(pkg):
    sc, out = random_out(pkg)
    n, worst = 0, 0.0
    for p, row in enumerate(sc["truth"]):
        for i, t in enumerate(row):
            if sc["decisive"][p, i] and t["from_stereo"] and t["x3d"] is not None:
                kf = sc["kf1"] if t["branch"] == ref.BRANCH_STEREO1 else sc["kf2s"][p]
                d = np.linalg.norm(out["x3d"][p, i].astype(np.float64) - t["x3d"])
                bound = 1e-6 * (np.linalg.norm(t["x3d"]) + np.linalg.norm(ref.center(kf)))
                worst = max(worst, d / bound)
                n += 1
    print(f"{n} stereo points, worst error {worst:.3f} of the bound")
    assert n >= 100 and worst <= 1.0


def test_triangulated_x3d(pkg):
    sc, out = random_out(pkg)
    As, X = [], []
    for p, row in enumerate(sc["truth"]):
        for i, t in enumerate(row):
            if sc["decisive"][p, i] and t["branch"] == ref.BRANCH_TRI and t["x3d"] is not None:
                As.append(t["A"])
                X.append(out["x3d"][p, i])
    Ow1 = ref.center(sc["kf1"])
    err = ref.triangulation_errors(As, np.array(X), Ow1)
    yard = ref.triangulation_errors(As, ref.yardstick_x3d(As), Ow1)
    print(f"{len(As)} triangulated jobs: kernel max {err.max():.3e} median {np.median(err):.3e}; "
          f"sgesdd float32 max {yard.max():.3e} median {np.median(yard):.3e}")
    assert len(As) >= 400
    assert err.max() <= 4 * yard.max() and np.median(err) <= 4 * np.median(yard)


def test_gates_after_x3d(pkg):
    """Every job that reached the gates: the float32 restatement at the device's x3D gives the device's status."""
    sc, out = random_out(pkg)
    status = untaken(out["status"])
    n, bad = 0, []
    for p, kf2 in enumerate(sc["kf2s"]):
        for i in range(sc["kf1"].N):
            if status[p, i] >= ref.NP_Z1:
                n += 1
                want = ref.gates32(sc["kf1"], kf2, i, int(sc["m12"][p, i]), out["x3d"][p, i], sc["prm"])
                if want != status[p, i]:
                    bad.append((p, i, int(status[p, i]), want))
            else:
                assert not out["x3d"][p, i].any()
    print(f"{n} jobs through the gates, statuses {np.bincount(status.reshape(-1), minlength=12).tolist()}")
    assert n >= 600 and not bad, bad[:10]


def test_resolve_and_records(pkg):
    sc, out = random_out(pkg)
    resolved, taken, order = ref.resolve(untaken(out["status"]))
    assert np.array_equal(out["status"], resolved) and np.array_equal(out["taken_by"], taken)
    new = out["new"]
    assert len(new) == len(order) > 256 and (resolved == ref.NP_TAKEN).sum() >= 50
    assert [(int(r["p"]), int(r["idx1"])) for r in new] == order
    for r, (p, i) in zip(new, order):
        assert int(r["idx2"]) == int(sc["m12"][p, i]) and int(r["from_stereo"]) == int(out["from_stereo"][p, i])
        assert np.array_equal(r["x3d"], out["x3d"][p, i])
        normal, mn, mx = ref.record64(sc["kf1"], sc["kf2s"][p], i, r["x3d"])
        assert np.abs(r["normal"] - normal).max() <= 1e-6
        assert abs(r["min_dist"] - mn) <= 1e-6 * mn and abs(r["max_dist"] - mx) <= 1e-6 * mx


def test_early_stop_prefix(pkg):
    """The records with p < 1 equal a call with the first neighbour alone; likewise p < 2."""
    sc, out = random_out(pkg)
    for k in (1, 2):
        part = run(pkg, sc["kf1"], sc["kf2s"][:k], sc["m12"][:k], sc["prm"])
        prefix = out["new"][out["new"]["p"] < k]
        assert len(prefix) >= 100 and part["new"].tobytes() == prefix.tobytes()
        assert np.array_equal(untaken(part["status"]), untaken(out["status"][:k]))


def test_chain_device_entry(pkg, synth):
    """One small C3-style keyframe group: stereo extraction, stereo matching, BoW, SearchForTriangulationDevice
    and CreateNewMapPointsDevice on one stream with no host copy in between; equal to the host entry on the
    downloaded matches and features."""
    import torch
    n = 3
    bf, b = 47.90639384423901, 0.110074
    L, R, Tcw, _ = synth.stereo_sequence(n, seed=214)
    voc = synth.dbow_vocabulary(10, 6, seed=61)
    scale, sigma2 = synth.scale_tables()
    exl = pkg.ORBextractor(600, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=4)
    exr = pkg.ORBextractor(600, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=4)
    out_l = exl.extract_batch_device(torch.from_numpy(L).cuda(), (0, 0))
    out_r = exr.extract_batch_device(torch.from_numpy(R).cuda(), (0, 0))
    u, depth, _ = pkg.compute_stereo_matches_batch_device(exl, exr, out_l, out_r, bf, b)
    bow = pkg.ORBVocabulary(voc).transform_frames_device(out_l[1], out_l[2], 4)
    dev = [pkg.DeviceKeyFrame(out_l, bow, f, Tcw[f], synth.EUROC_K, scale, sigma2, u_right=u, mb=b, mbf=bf, depth=depth)
           for f in range(n)]
    m = pkg.ORBmatcher(0.6, False)
    m12, cnt = m.SearchForTriangulationDevice(dev[2], dev[:2], False)
    got = m.CreateNewMapPointsDevice(dev[2], dev[:2], m12, cnt)
    torch.cuda.synchronize()
    # the host entry on the downloaded features and matches
    kps, counts = out_l[0].cpu().numpy(), out_l[2].cpu().numpy()
    un, dn = u.cpu().numpy(), depth.cpu().numpy()
    host = []
    for f in range(n):
        N = int(counts[f, 0])
        k = np.ascontiguousarray(kps[f, :N]).view(np.uint8).reshape(N, 28).view(pkg.KEYPOINT_DTYPE).reshape(N)
        host.append(pkg.KeyFrame(k, np.zeros((N, 32), np.uint8), Tcw[f], synth.EUROC_K, scale, sigma2, u_right=un[f, :N],
                                 mb=b, mbf=bf, depth=dn[f, :N]))
    N1 = host[2].N
    hm12, hcnt = m12.cpu().numpy()[:, :N1], cnt.cpu().numpy()
    want = m.CreateNewMapPoints(host[2], host[:2], hm12, hcnt)
    new = m.newpoints_records(got["records"], got["n_new"])
    print(f"{int((hm12 >= 0).sum())} matches, {len(new)} new points, statuses "
          f"{np.bincount(want['status'].reshape(-1), minlength=13).tolist()}")
    assert (hm12 >= 0).sum() >= 50 and len(want["new"]) >= 10
    assert np.array_equal(got["status"].cpu().numpy()[:, :N1], want["status"])
    assert (got["status"].cpu().numpy()[:, N1:] == ref.NP_NO_MATCH).all()
    assert np.array_equal(got["x3d"].cpu().numpy()[:, :N1], want["x3d"])
    assert np.array_equal(got["from_stereo"].cpu().numpy()[:, :N1], want["from_stereo"])
    assert np.array_equal(got["taken_by"].cpu().numpy()[:N1], want["taken_by"])
    assert new.tobytes() == want["new"].tobytes()


def test_argument_rejection(pkg):
    sc = scenes.random_truth()
    lib, m = pkg._lib.load(), pkg.ORBmatcher(0.6, False)
    K = pkg.keyframe
    ARG = pkg._lib.ORB_ERR_ARG
    kf1, kf2 = sc["kf1"], sc["kf2s"][0]
    C = kf1.N
    bufs = [np.zeros(C, np.int32), np.zeros((C, 3), np.float32), np.zeros(C, np.uint8), np.zeros(C, np.int32),
            np.zeros(C, K.NEWPOINT_DTYPE), np.full(1, -7, np.int32)]
    out = K.NewPointsOut(*[a.ctypes.data for a in bufs])
    prm = K.NewPointsParams(0, 0, 0.0, 1.8)
    m12 = np.ascontiguousarray(sc["m12"][:1])

    def call(v1=None, v2=None, n=1, prm=prm, matches=m12, out=out, handle=None):
        v1 = kf1.newpoints_view() if v1 is None else v1
        v2 = (K.NewPointsKf * 1)(kf2.newpoints_view() if v2 is None else v2)
        return lib.orb_create_new_map_points(m._handle() if handle is None else handle, ctypes.byref(v1), v2, n,
                                             None if prm is None else ctypes.byref(prm),
                                             None if matches is None else matches.ctypes.data, None,
                                             None if out is None else ctypes.byref(out))

    assert call() == 0 and bufs[5][0] > 100
    assert call(prm=None) == ARG and call(out=None) == ARG and call(matches=None) == ARG
    assert call(n=-1) == ARG and call(n=1025) == ARG
    o2 = K.NewPointsOut(*[a.ctypes.data for a in bufs])
    o2.records = None
    assert call(out=o2) == ARG
    for field, value in (("n", -1), ("n", (1 << 20) + 1), ("nlevels", 0), ("nlevels", 13), ("kps_un", None),
                         ("scale_factors", None), ("level_sigma2", None)):
        v = kf2.newpoints_view()
        setattr(v.view, field, value)
        assert call(v2=v) == ARG, field
    v = kf1.newpoints_view()
    v.extra.depth = None  # u_right without mvDepth
    assert call(v1=v) == ARG
    bad = m12.copy()
    bad[0, 0] = kf2.N  # a match past the neighbour's N
    assert call(matches=bad) == ARG
    assert b"CreateNewMapPoints" in lib.orb_last_error()
    # no neighbour: ORB_OK, no points
    assert call(n=0) == 0 and bufs[5][0] == 0 and (bufs[3] == -1).all()
