"""Python restatement of the triangulation half of LocalMapping::CreateNewMapPoints (reference
src/LocalMapping.cc:626-910, with GeometricTools::Triangulate src/GeometricTools.cc:63-90,
KeyFrame::UnprojectStereo src/KeyFrame.cc:905-924, MapPoint::UpdateNormalAndDepth src/MapPoint.cc:567-642)
and of the rule of its neighbour loop (the first neighbour that succeeds keeps idx1): what the GPU tests of
orb_create_new_map_points compare against.

Two modes:
  truth()    float64 on the float32 inputs: the branch taken (triangulate / stereo 1 / stereo 2 / low
             parallax), x3D, the full status, and the smallest absolute margin of the cos-parallax
             comparisons on the job's path (a job is *decisive* when that margin is > 1e-5).  Triangulation
             solves the float32 A the kernel builds (rows exactly as GeometricTools.cc:73-76) with a float64 SVD.
  gates32()  the gates that follow x3D (:794-884) in exact float32 with the contractions csrc/orb_newpoints.hip
             lists, evaluated at a given float32 x3D: bit for bit what the kernel computes there.
"""
from __future__ import annotations

import math

import numpy as np

import conftest
from fuse_ref import dot3, f32, fma32

conftest.load_package()
from orbslam3_amd.keyframe import (NP_CHI2_1, NP_CHI2_2, NP_DIST_ZERO, NP_FAR, NP_LOW_PARALLAX, NP_NO_MATCH,  # noqa: E402
                                   NP_OK, NP_SCALE, NP_STEREO_DEPTH, NP_TAKEN, NP_TRI_W_ZERO, NP_Z1, NP_Z2)

BRANCH_NONE, BRANCH_TRI, BRANCH_STEREO1, BRANCH_STEREO2, BRANCH_LOW = range(5)
DECISIVE = 1e-5
ORB_ERR_CAPACITY = -3


class Params:
    def __init__(self, inertial=False, far_points=False, th_far_points=0.0, ratio_factor=1.5 * 1.2):
        self.inertial, self.far_points = bool(inertial), bool(far_points)
        self.th_far_points, self.ratio_factor = f32(th_far_points), f32(ratio_factor)


def center(kf):
    return kf.Ow if kf.Ow is not None else np.ascontiguousarray(-(kf.Tcw[:, :3].T @ kf.Tcw[:, 3]), dtype=f32)


def stereo_flag(kf, i):
    return kf.mvuRight is not None and kf.mvuRight[i] >= 0


def xn32(kf, i):
    """Pinhole::unprojectEig of mvKeysUn[i] in float32."""
    k = kf.mvKeysUn[i]
    return np.array([(f32(k["x"]) - f32(kf.cx)) / f32(kf.fx), (f32(k["y"]) - f32(kf.cy)) / f32(kf.fy), 1.0], f32)


def matrix_a32(kf1, kf2, i, j):
    """A of GeometricTools::Triangulate in float32: fma(xn[k], T[2][c], -T[k][c])."""
    A = np.zeros((4, 4), f32)
    for r0, (kf, idx) in enumerate(((kf1, i), (kf2, j))):
        xn = xn32(kf, idx)
        for k in range(2):
            A[2 * r0 + k] = fma32(xn[k], kf.Tcw[2], -kf.Tcw[k])
    return A


def null_vector(A, dtype):
    """The right singular vector of the smallest singular value (numpy / LAPACK, in `dtype`)."""
    return np.linalg.svd(A.astype(dtype))[2][3]


def unproject_stereo64(kf, i):
    z = float(kf.mvDepth[i])
    if not z > 0:
        return None
    k = (kf.mvKeys if kf.mvKeys is not None else kf.mvKeysUn)[i]
    x = (float(k["x"]) - kf.cx) * z * (1.0 / kf.fx)
    y = (float(k["y"]) - kf.cy) * z * (1.0 / kf.fy)
    T = kf.Tcw.astype(np.float64)
    return T[:, :3].T @ np.array([x, y, z]) + center(kf).astype(np.float64)


def gates64(kf1, kf2, i, j, X, prm):
    """:794-884 in float64 at X."""
    T1, T2 = kf1.Tcw.astype(np.float64), kf2.Tcw.astype(np.float64)
    z1 = T1[2, :3] @ X + T1[2, 3]
    if z1 <= 0:
        return NP_Z1
    z2 = T2[2, :3] @ X + T2[2, 3]
    if z2 <= 0:
        return NP_Z2
    for kf, T, z, idx, code in ((kf1, T1, z1, i, NP_CHI2_1), (kf2, T2, z2, j, NP_CHI2_2)):
        k = kf.mvKeysUn[idx]
        x, y = T[0, :3] @ X + T[0, 3], T[1, :3] @ X + T[1, 3]
        u, v = kf.fx * x / z + kf.cx, kf.fy * y / z + kf.cy
        e2 = (u - float(k["x"])) ** 2 + (v - float(k["y"])) ** 2
        sigma2 = float(kf.mvLevelSigma2[k["octave"]])
        if stereo_flag(kf, idx):
            e2 += (u - kf1.mbf / z - float(kf.mvuRight[idx])) ** 2  # keyframe 1's mbf for both (:826, :853)
            if e2 > 7.8 * sigma2:
                return code
        elif e2 > 5.991 * sigma2:
            return code
    d1 = np.linalg.norm(X - center(kf1).astype(np.float64))
    d2 = np.linalg.norm(X - center(kf2).astype(np.float64))
    if d1 == 0 or d2 == 0:
        return NP_DIST_ZERO
    if prm.far_points and (d1 >= prm.th_far_points or d2 >= prm.th_far_points):
        return NP_FAR
    ratio_dist = d2 / d1
    ratio_octave = float(kf1.mvScaleFactors[kf1.mvKeysUn[i]["octave"]]) / float(kf2.mvScaleFactors[kf2.mvKeysUn[j]["octave"]])
    rf = float(prm.ratio_factor)
    if ratio_dist * rf < ratio_octave or ratio_dist > ratio_octave * rf:
        return NP_SCALE
    return NP_OK


def truth(kf1, kf2, i, j, prm):
    """One job in float64.  Returns dict(branch, status, x3d (float64 or None), from_stereo, margin, A)."""
    out = dict(branch=BRANCH_NONE, status=NP_NO_MATCH, x3d=None, from_stereo=0, margin=math.inf, A=None)
    if j < 0:
        return out
    rays = []
    for kf, idx in ((kf1, i), (kf2, j)):
        xn = xn32(kf, idx).astype(np.float64)
        rays.append(kf.Tcw[:, :3].astype(np.float64).T @ xn)
    cos_rays = rays[0] @ rays[1] / (np.linalg.norm(rays[0]) * np.linalg.norm(rays[1]))
    s1, s2 = stereo_flag(kf1, i), stereo_flag(kf2, j)
    cos1 = cos2 = cos_rays + 1
    if s1:
        cos1 = math.cos(2 * math.atan2(kf1.mb / 2, float(kf1.mvDepth[i])))
    elif s2:
        cos2 = math.cos(2 * math.atan2(kf2.mb / 2, float(kf2.mvDepth[j])))
    cos_stereo = min(cos1, cos2)
    margins = []

    def less(a, b):  # a < b, recording the margin of a comparison that was evaluated
        margins.append(abs(a - b))
        return a < b

    lim = 0.9996 if prm.inertial else 0.9998
    if less(cos_rays, cos_stereo) and less(0.0, cos_rays) and (s1 or s2 or less(cos_rays, lim)):
        out["branch"] = BRANCH_TRI
        out["A"] = matrix_a32(kf1, kf2, i, j)
        xh = null_vector(out["A"], np.float64)
        if xh[3] == 0:
            out["status"] = NP_TRI_W_ZERO
        else:
            out["x3d"] = xh[:3] / xh[3]
    elif s1 and less(cos1, cos2):
        out["branch"], out["from_stereo"] = BRANCH_STEREO1, 1
        out["x3d"] = unproject_stereo64(kf1, i)
    elif s2 and less(cos2, cos1):
        out["branch"], out["from_stereo"] = BRANCH_STEREO2, 1
        out["x3d"] = unproject_stereo64(kf2, j)
    else:
        out["branch"], out["status"] = BRANCH_LOW, NP_LOW_PARALLAX
    out["margin"] = min(margins)
    if out["x3d"] is not None:
        out["status"] = gates64(kf1, kf2, i, j, out["x3d"], prm)
    elif out["from_stereo"]:
        out["status"] = NP_STEREO_DEPTH
    return out


def cam32(kf, r, X):
    return dot3(kf.Tcw[r, :3], X) + kf.Tcw[r, 3]


def chi2_rejects32(kf, X, z, idx, mbf1):
    k = kf.mvKeysUn[idx]
    x, y = cam32(kf, 0, X), cam32(kf, 1, X)
    invz = f32(1.0 / float(z))
    sigma2 = float(kf.mvLevelSigma2[k["octave"]])
    fx, fy, cx, cy = f32(kf.fx), f32(kf.fy), f32(kf.cx), f32(kf.cy)
    if not stereo_flag(kf, idx):
        ex, ey = (fx * x / z + cx) - k["x"], (fy * y / z + cy) - k["y"]
        return float(fma32(ex, ex, ey * ey)) > 5.991 * sigma2
    u = fma32(fx * x, invz, cx)
    u_r = fma32(-f32(mbf1), invz, u)
    v = fma32(fy * y, invz, cy)
    ex, ey, er = u - k["x"], v - k["y"], u_r - kf.mvuRight[idx]
    return float(fma32(er, er, fma32(ex, ex, ey * ey))) > 7.8 * sigma2


def gates32(kf1, kf2, i, j, X, prm):
    """:794-884 in the kernel's float32 arithmetic at the float32 X."""
    X = np.asarray(X, f32)
    with np.errstate(all="ignore"):
        z1 = cam32(kf1, 2, X)
        if z1 <= 0:
            return NP_Z1
        z2 = cam32(kf2, 2, X)
        if z2 <= 0:
            return NP_Z2
        if chi2_rejects32(kf1, X, z1, i, kf1.mbf):
            return NP_CHI2_1
        if chi2_rejects32(kf2, X, z2, j, kf1.mbf):
            return NP_CHI2_2
        n1, n2 = X - center(kf1), X - center(kf2)
        d1, d2 = np.sqrt(dot3(n1, n1)), np.sqrt(dot3(n2, n2))
        if d1 == 0 or d2 == 0:
            return NP_DIST_ZERO
        if prm.far_points and (d1 >= prm.th_far_points or d2 >= prm.th_far_points):
            return NP_FAR
        ratio_dist = d2 / d1
        ratio_octave = kf1.mvScaleFactors[kf1.mvKeysUn[i]["octave"]] / kf2.mvScaleFactors[kf2.mvKeysUn[j]["octave"]]
        if ratio_dist * prm.ratio_factor < ratio_octave or ratio_dist > ratio_octave * prm.ratio_factor:
            return NP_SCALE
    return NP_OK


def truth_all(kf1, kf2s, matches12, prm, n_matches=None):
    """truth() of every job: a [P][N1] list of dicts (a flagged pair has no matches)."""
    rows = []
    for p, kf2 in enumerate(kf2s):
        flagged = n_matches is not None and n_matches[p] < 0
        rows.append([truth(kf1, kf2, i, -1 if flagged else int(matches12[p][i]), prm) for i in range(kf1.N)])
    return rows


def resolve(status):
    """The neighbour loop's rule on a [P, N1] status array: (status with TAKEN, taken_by [N1], [(p, idx1)] in
    creation order)."""
    status = np.array(status, np.int32)
    P, n1 = status.shape
    taken = np.full(n1, -1, np.int32)
    for i in range(n1):
        for p in range(P):
            if status[p, i] == NP_OK:
                if taken[i] < 0:
                    taken[i] = p
                else:
                    status[p, i] = NP_TAKEN
    order = [(p, i) for p in range(P) for i in range(n1) if taken[i] == p]
    return status, taken, order


def record64(kf1, kf2, i, X):
    """MapPoint::UpdateNormalAndDepth for the two observations in float64: (normal, min_dist, max_dist)."""
    X = np.asarray(X, np.float64)
    n1, n2 = X - center(kf1).astype(np.float64), X - center(kf2).astype(np.float64)
    d1, d2 = np.linalg.norm(n1), np.linalg.norm(n2)
    mx = d1 * float(kf1.mvScaleFactors[kf1.mvKeysUn[i]["octave"]])
    return (n1 / d1 + n2 / d2) / 2, mx / float(kf1.mvScaleFactors[-1]), mx


def triangulation_errors(As, X, Ow1):
    """|x - x64| / |x64 - Ow1| per job: x64 from the float64 SVD of each float32 A [n, 4, 4], X [n, 3]."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    err = np.zeros(len(As))
    for k, A in enumerate(As):
        xh = null_vector(A, np.float64)
        x64 = xh[:3] / xh[3]
        err[k] = np.linalg.norm(X[k] - x64) / np.linalg.norm(x64 - np.asarray(Ow1, np.float64))
    return err


def yardstick_x3d(As):
    """The independent single-precision solver: LAPACK's sgesdd through scipy.linalg.svd, which keeps float32
    (np.linalg.svd does not: it computes a float32 input in double and casts the result), x3D = head / w in
    float32."""
    import scipy.linalg
    out = np.zeros((len(As), 3), f32)
    for k, A in enumerate(As):
        vt = scipy.linalg.svd(np.asarray(A, f32), lapack_driver="gesdd")[2]
        assert vt.dtype == f32
        out[k] = vt[3, :3] / vt[3, 3]
    return out


def host_svd4():
    """csrc/orb_svd4.h compiled for the host (tests/native/svd4_host.cpp) as a ctypes library."""
    import ctypes
    import pathlib
    import subprocess
    root = pathlib.Path(__file__).resolve().parents[1]
    build = root / "build" / "tests"
    build.mkdir(parents=True, exist_ok=True)
    so = build / "libsvd4_host.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Werror",
                    str(root / "tests" / "native" / "svd4_host.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.svd4_null_vectors.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.svd4_null_vectors.restype = None
    return lib
