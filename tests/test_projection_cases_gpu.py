"""The hand-built SearchByProjection scenes (tests/projection_cases.py) on every form of the kernels:
the host calls (ORBmatcher.SearchByProjectionFrame / SearchByProjection: wave-per-point candidates, the
host-built grid, capacity growth), the single device calls (orb_search_by_projection_frame_device /
_local_device: the grid and the points prepared on the device) and, for the frame overload, the tracking
chain's batch forms (LDS-staged and thread-per-point candidates, one launch per stage).  Assignments and
count equal tests/projection_ref.py bit for bit; a failure names the cases involved.  That a scene reaches
the path it is meant for is shown on the reference's diagnostics by test_projection_cases_cpu.py."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import projection_cases as cases
import projection_ref as ref

pytestmark = pytest.mark.gpu
reference = cases.reference

DEVICE_CAP = 16384   # the device forms' keypoint limit
FRAME_DEVICE = [n for n in cases.FRAME_GROUPS if n not in ("frame_large_16385", "frame_large_65537")]


def assert_same(name, form, g, r, n, got):
    got = np.asarray(got)
    assert got.shape == r.assign.shape, f"{name}/{form}: {got.shape}"
    bad = np.flatnonzero(got != r.assign)
    if len(bad) == 0 and n == r.n:
        return
    lines = []
    for j in bad[:8]:
        who = sorted({i for i, p in enumerate(r.points) if p.match == j or any(c == j for c, _ in p.cands)} |
                     ({int(got[j])} if 0 <= got[j] < len(g.names) else set()))
        lines.append(f"  keypoint {j}: point {got[j]}, reference {r.assign[j]}; cases: " +
                     "; ".join(f"[{i}] {g.names[i]} ({ref.REASONS[r.points[i].reason]})" for i in who[:6]))
    raise AssertionError(f"{name}/{form}: count {n} vs reference {r.n}, {len(bad)} keypoints differ\n" + "\n".join(lines))


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_host_form(pkg, name):
    g, C, X, r = reference(pkg, name)
    p = g.params
    if g.kind == "frame":
        n, got = pkg.ORBmatcher(0.9, p["check_ori"]).SearchByProjectionFrame(C, X, p["th"], p["mono"])
    else:
        n, got = pkg.ORBmatcher(p["ratio"], True).SearchByProjection(C, X, p["th"], p["far"], p["th_far"], p["taken"])
    assert_same(name, "host", g, r, n, got)


def _up(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def device_frame(pkg, F, Tcw=None, pad=37, cap=None):
    """F on the device with capacity past its count; the padding holds junk the kernels must not read."""
    rng = np.random.default_rng(F.N + 1)
    pad = pad if cap is None else cap - F.N
    cap_f = F.N + pad
    junk = np.zeros(pad, cases.KEYPOINT_DTYPE)
    junk["x"], junk["y"] = rng.uniform(0, 640, pad), rng.uniform(0, 480, pad)
    junk["octave"] = rng.integers(0, 8, pad)
    k = np.concatenate([F.mvKeysUn, junk])
    d = np.concatenate([F.mDescriptors, rng.integers(0, 256, (pad, 32), dtype=np.uint8)])
    ur = None if F.mvuRight is None else _up(np.concatenate([F.mvuRight, np.full(pad, 100, np.float32)]).reshape(1, cap_f),
                                             np.float32)
    return pkg.DeviceFrame(_up(k.view(np.float32).reshape(1, cap_f, 7), np.float32), _up(d.reshape(1, cap_f, 32), np.uint8),
                           _up(np.array([[F.N, 0]]), np.int32), 0, F.Tcw if Tcw is None else Tcw, (F.fx, F.fy, F.cx, F.cy),
                           F.mvScaleFactors, cases.LEVEL_SIGMA2, int(F.mnMaxX), int(F.mnMaxY), F.mbf, ur)


def device_last(pkg, L, pad=11):
    last = device_frame(pkg, L, pad=pad)
    mp = L.map_points

    def padded(a, v):
        a = np.asarray(a)
        return np.concatenate([a, np.full((pad,) + a.shape[1:], v, a.dtype)])
    return pkg.DeviceLastPoints(last, _up(padded(mp["valid"], 1), np.uint8), _up(padded(mp["observed"], 1), np.uint8),
                                _up(padded(mp["xyz"], 1.0), np.float32), _up(padded(mp["desc"], 0), np.uint8))


def garbage_outputs(cap):
    import torch
    return (torch.full((cap,), 123456, dtype=torch.int32, device="cuda"),
            torch.full((1,), -7, dtype=torch.int32, device="cuda"))


def check_device_result(name, form, g, r, N, d_m, d_n):
    import torch
    torch.cuda.synchronize()
    m = d_m.cpu().numpy()
    assert (m[N:] == -1).all(), f"{name}/{form}: match rows past the count are not -1"
    assert_same(name, form, g, r, int(d_n.item()), m[:N])


@pytest.mark.parametrize("name", FRAME_DEVICE)
def test_frame_device_form(pkg, name):
    import torch
    g, C, L, r = reference(pkg, name)
    assert C.N + 37 <= DEVICE_CAP
    p = g.params
    cur, last = device_frame(pkg, C), device_last(pkg, L)
    d_m, d_n = garbage_outputs(cur.cap)
    m = pkg.ORBmatcher(0.9, p["check_ori"])
    st = torch.cuda.current_stream()
    pkg._lib.check(pkg._lib.load().orb_search_by_projection_frame_device(
        m._handle(), ctypes.byref(cur.view()), ctypes.byref(last.view()), float(p["th"]), int(p["mono"]), d_m.data_ptr(),
        d_n.data_ptr(), ctypes.c_void_p(st.cuda_stream)), "orb_search_by_projection_frame_device")
    check_device_result(name, "device", g, r, C.N, d_m, d_n)


def local_frame_8193(pkg):
    """The claims group in a frame of 8,193 keypoints (clutter below every window, put in front of the
    group's keypoints): the device grid's cell lists leave LDS."""
    g = cases.group("local_claims")
    s = cases.LocalScene(240)
    s.clutter(8193 - len(g.cur["keys_un"]))
    c = s.cur()
    n0 = len(c["keys_un"])
    cur = dict(g.cur, keys_un=np.concatenate([c["keys_un"], g.cur["keys_un"]]),
               descriptors=np.concatenate([c["descriptors"], g.cur["descriptors"]]),
               u_right=np.concatenate([c["u_right"], g.cur["u_right"]]))
    taken = np.concatenate([np.zeros(n0, np.uint8), g.params["taken"]])
    return g._replace(cur=cur, params=dict(g.params, taken=taken), expected_match={}), n0


@pytest.mark.parametrize("name", list(cases.LOCAL_GROUPS) + ["local_claims in 8193 keypoints"])
def test_local_device_form(pkg, name):
    import torch
    if name in cases.LOCAL_GROUPS:
        g, F, P, r = reference(pkg, name)
    else:
        g, n0 = local_frame_8193(pkg)
        F, P = pkg.Frame(**g.cur), pkg.LocalMapPoints(**g.points)
        p = g.params
        r = ref.search_local(F, P, p["th"], p["far"], p["th_far"], p["ratio"], p["taken"])
        base = reference(pkg, "local_claims")[3]   # the same scene, the keypoints n0 further on
        assert F.N == 8193 and r.n == base.n and np.array_equal(r.assign[n0:], base.assign)
    p = g.params
    cur = device_frame(pkg, F)
    n = P.n
    z3, z1 = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    local = pkg.DeviceLocalMap.from_host(torch.device("cuda"), pos=z3, normal=z3, min_dist=z1, max_dist=z1, desc=P.desc,
                                         observed=P.observed, is_bad=P.is_bad)
    for k, dt in (("track_in_view", np.uint8), ("track_proj", np.float32), ("track_depth", np.float32),
                  ("track_level", np.int32), ("track_view_cos", np.float32)):
        getattr(local, k)[:n].copy_(_up(getattr(P, k), dt))
    taken = _up(np.concatenate([p["taken"], np.ones(cur.cap - F.N, np.uint8)]), np.uint8)
    d_m, d_n = garbage_outputs(cur.cap)
    m = pkg.ORBmatcher(p["ratio"], True)
    st = torch.cuda.current_stream()
    pkg._lib.check(pkg._lib.load().orb_search_by_projection_local_device(
        m._handle(), ctypes.byref(cur.view()), taken.data_ptr(), ctypes.byref(local.view()), float(p["th"]), int(p["far"]),
        float(p["th_far"]), d_m.data_ptr(), d_n.data_ptr(), ctypes.c_void_p(st.cuda_stream)),
        "orb_search_by_projection_local_device")
    check_device_result(name, "device", g, r, F.N, d_m, d_n)


# the chain's matcher is ORBmatcher(0.9, true); th_motion and bMono belong to the chain, so the groups of
# one call share them
BATCHES = {}
for _n in cases.FRAME_GROUPS:
    if _n in ("frame_large_16385", "frame_large_65537", "frame_prep_8193", "frame_rotation_off"):
        continue   # more keypoints than the batch's cap / checkOri off
    _p = cases.group(_n).params
    BATCHES.setdefault((_p["th"], _p["mono"]), []).append(_n)


@pytest.mark.parametrize("cap", [None, 3000], ids=["lds-staged", "thread-per-point"])
@pytest.mark.parametrize("key", list(BATCHES), ids=lambda k: f"th{k[0]}-mono{int(k[1])}")
def test_frame_batch_forms(pkg, key, cap):
    """Through TrackingChainBatch with the motion gate off, an empty local map per slot and the identity
    pose.  m1 comes back after the outlier discard, so the search's own result is compared: n1, and the
    assignment rebuilt from the first graph (one edge per assigned keypoint, its xw the last-frame point's
    position, which is distinct per point).  cap None: the smallest that holds the groups (LDS-staged
    candidates); 3000 is above what one workgroup's LDS holds (thread per point)."""
    import torch
    th, mono = key
    names = BATCHES[key]
    refs = [reference(pkg, n) for n in names]
    small = max(C.N for _, C, _, _ in refs) + 5
    assert small <= 2706 < 3000
    cap = cap or small
    dev = torch.device("cuda")
    empty = dict(pos=np.zeros((0, 3), np.float32), normal=np.zeros((0, 3), np.float32), min_dist=np.zeros(0, np.float32),
                 max_dist=np.zeros(0, np.float32), desc=np.zeros((0, 32), np.uint8), observed=np.zeros(0, np.uint8),
                 is_bad=np.zeros(0, np.uint8))
    pose7 = np.array([0, 0, 0, 0, 0, 0, 1], np.float64)
    items = [(device_frame(pkg, C, cap=cap), device_last(pkg, L), pkg.DeviceLocalMap.from_host(dev, **empty), pose7)
             for _, C, L, _ in refs]
    batch = pkg.TrackingChainBatch(cap, len(items), th_motion=th, mono=mono, gate=False)
    res = batch.track(items).sync()
    form = f"batch cap {cap}"
    for name, (g, C, L, r), out in zip(names, refs, res):
        where = {tuple(np.asarray(x, np.float64)): i for i, x in enumerate(np.asarray(L.map_points["xyz"], np.float32))}
        got = np.full(C.N, -1, np.int64)
        kp = np.asarray(out["edge_kp1"])
        assert len(kp) == len(set(kp.tolist())) and (kp < C.N).all(), f"{name}/{form}: edge keypoints"
        for j, xw in zip(kp, out["edges1"]["xw"]):
            got[j] = where[tuple(xw)]
        assert_same(name, form, g, r, out["n1"], got)
    batch.release()
