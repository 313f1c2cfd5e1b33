"""Scenes for the triangulation half of LocalMapping::CreateNewMapPoints (tests/newpoints_ref.py, the GPU
tests): hand-built cases of one or two matches, keyframe 1 against 2-3 neighbours, that reach every status
code by a wide margin, and one seeded random scene.

Camera: fx = fy = 500, (cx, cy) = (320, 240), 8 levels of 1.2, mb = 0.1 m.  Unless a case says otherwise a
keyframe looks down +z from its centre and its keypoints are exact projections, so a triangulated point is
the world point it was projected from.

Two status codes compare for exact equality and no rigid, consistent input reaches them; their cases use
inputs the ABI accepts but a SLAM system does not produce, and say so:
  TRI_W_ZERO  x3Dh(3) == 0 needs parallel rays, which the parallax test has rejected before.  The case passes
              3x4 matrices that are not rigid poses and make A = diag(-1, -1.5, 2, 2): its null vector is e0.
  DIST_ZERO   x3D == Ow means z <= 0 first.  The case passes a camera centre that is not the pose's.
"""
from __future__ import annotations

import numpy as np

import conftest

conftest.load_package()
from orbslam3_amd._lib import KEYPOINT_DTYPE  # noqa: E402
from orbslam3_amd.keyframe import KeyFrame  # noqa: E402
import newpoints_ref as ref  # noqa: E402
from newpoints_ref import (NP_CHI2_1, NP_CHI2_2, NP_DIST_ZERO, NP_FAR, NP_LOW_PARALLAX, NP_NO_MATCH, NP_OK,  # noqa: E402
                           NP_SCALE, NP_STEREO_DEPTH, NP_TAKEN, NP_TRI_W_ZERO, NP_Z1, NP_Z2, Params)

FX = FY = 500.0
CX, CY = 320.0, 240.0
CAMERA = (FX, FY, CX, CY)
NLEVELS = 8
SCALE = (np.float32(1.2) ** np.arange(NLEVELS)).astype(np.float32)
SIGMA2 = (SCALE * SCALE).astype(np.float32)
MB = 0.1
MBF = MB * FX
RATIO_FACTOR = float(np.float32(1.5) * SCALE[1])


def pose(center, yaw=0.0, pitch=0.0):
    """Tcw (3x4 float64) of a camera at `center` turned by yaw (about y) then pitch (about x)."""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0, -sy], [0, 1, 0], [sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, sp], [0, -sp, cp]])
    R = Rx @ Ry
    return np.hstack([R, (-R @ np.asarray(center, float))[:, None]])


def project(Tcw, P):
    """(u, v, z) of world point P (float64); z may be negative (the line through the centre is projected)."""
    Pc = Tcw[:, :3] @ np.asarray(P, float) + Tcw[:, 3]
    return FX * Pc[0] / Pc[2] + CX, FY * Pc[1] / Pc[2] + CY, Pc[2]


def obs(Tcw, P, octave=0, stereo=False, dx=0.0, dy=0.0, depth=None, raw_shift=None, mbf=MBF):
    """A keypoint observing P: dict(x, y, octave, ur, depth, raw) -- ur / depth -1 for a monocular keypoint."""
    u, v, z = project(Tcw, P)
    d = (z if depth is None else depth) if stereo else -1.0
    ur = (u + dx) - mbf / z if stereo else -1.0
    raw = None if raw_shift is None else (u + dx + raw_shift[0], v + dy + raw_shift[1])
    return dict(x=u + dx, y=v + dy, octave=octave, ur=ur, depth=d, raw=raw)


def make_kf(Tcw, kps, Ow=None, stereo_arrays=None, mb=MB):
    """A KeyFrame of the keypoint dicts `kps`.  The stereo arrays are present when any keypoint is stereo
    (stereo_arrays overrides); mvKeys when any keypoint has a raw position."""
    n = len(kps)
    k = np.zeros(n, KEYPOINT_DTYPE)
    for i, o in enumerate(kps):
        k[i]["x"], k[i]["y"], k[i]["octave"], k[i]["size"] = o["x"], o["y"], o["octave"], 31.0
    has_st = any(o["ur"] >= 0 for o in kps) if stereo_arrays is None else stereo_arrays
    raw = None
    if any(o["raw"] is not None for o in kps):
        raw = k.copy()
        for i, o in enumerate(kps):
            if o["raw"] is not None:
                raw[i]["x"], raw[i]["y"] = o["raw"]
    return KeyFrame(k, np.zeros((n, 32), np.uint8), Tcw, CAMERA, SCALE, SIGMA2,
                    u_right=np.array([o["ur"] for o in kps], np.float32) if has_st else None, Ow=Ow, mb=mb, mbf=mb * FX,
                    depth=np.array([o["depth"] for o in kps], np.float32) if has_st else None, keys_raw=raw)


class Case:
    """name; kf1; kf2s; matches12 [P, N1]; n_matches [P] or None; prm; the expected status [P][N1] after the
    resolve, from_stereo [P][N1], branch [P][N1] (ref.BRANCH_*) and, where given, the expected x3D of a job."""

    def __init__(self, name, kf1, kf2s, m12, status, from_stereo, branch, prm=None, n_matches=None, x3d=None):
        self.name, self.kf1, self.kf2s = name, kf1, kf2s
        self.m12 = np.array(m12, np.int32).reshape(len(kf2s), kf1.N)
        self.status, self.from_stereo, self.branch = status, from_stereo, branch
        self.prm = prm or Params(ratio_factor=RATIO_FACTOR)
        self.n_matches = None if n_matches is None else np.array(n_matches, np.int32)
        self.x3d = x3d or {}


T0 = pose((0, 0, 0))
B_, T_, S1, S2, L_ = ref.BRANCH_NONE, ref.BRANCH_TRI, ref.BRANCH_STEREO1, ref.BRANCH_STEREO2, ref.BRANCH_LOW
EMPTY = lambda: make_kf(pose((0.3, 0.1, 0)), [])  # noqa: E731  (a neighbour without keypoints)


def cases():
    out = []
    P = (0.3, -0.2, 5.0)
    Ta, Tb, Tc = pose((0.5, 0, 0)), pose((-0.5, 0.05, 0), yaw=0.05, pitch=-0.03), pose((1.0, 0, 0.2), yaw=-0.1)

    # idx1 0 accepted by neighbours 0 and 2 (OK, TAKEN), unmatched in 1; idx1 1 rejected by 0 (its match sits 8 px
    # off the epipolar line at octave 0: about 4 px in each image, 16 > 5.991, while keyframe 1's octave 7 allows
    # 5.991 * 12.8), accepted by 1, accepted again by 2 (TAKEN)
    Q = (-0.4, 0.3, 6.0)
    kf1 = make_kf(T0, [obs(T0, P), obs(T0, Q, octave=7)])
    out.append(Case("mono_ok_taken_and_second_neighbour", kf1,
                    [make_kf(Ta, [obs(Ta, P), obs(Ta, Q, dy=8.0)]), make_kf(Tb, [obs(Tb, Q, octave=7)]),
                     make_kf(Tc, [obs(Tc, Q, octave=7), obs(Tc, P)])],
                    [[0, 1], [-1, 0], [1, 0]],
                    [[NP_OK, NP_CHI2_2], [NP_NO_MATCH, NP_OK], [NP_TAKEN, NP_TAKEN]], [[0, 0]] * 3,
                    [[T_, T_], [B_, T_], [T_, T_]], x3d={(0, 0): P, (1, 1): Q, (2, 0): P, (2, 1): Q}))

    # the same 8 px at octave 0 in keyframe 1: its own test rejects first
    kf1 = make_kf(T0, [obs(T0, P)])
    out.append(Case("chi2_1", kf1, [make_kf(Ta, [obs(Ta, P, dy=8.0)]), EMPTY()], [[0], [-1]],
                    [[NP_CHI2_1], [NP_NO_MATCH]], [[0]] * 2, [[T_], [B_]]))

    # 200 m away with a 0.5 m baseline: cos = 0.999997 (> 0.9998), no stereo
    F = (0.0, 0.0, 200.0)
    out.append(Case("low_parallax", make_kf(T0, [obs(T0, F)]), [make_kf(Ta, [obs(Ta, F)]), EMPTY()], [[0], [-1]],
                    [[NP_LOW_PARALLAX], [NP_NO_MATCH]], [[0]] * 2, [[L_], [B_]]))

    # cos = 0.9997 (0.5 m baseline, 20.4 m away): triangulated without IMU, low parallax with it
    G = (0.25, 0.0, 20.4)
    for inertial, st, br in ((False, NP_OK, T_), (True, NP_LOW_PARALLAX, L_)):
        out.append(Case(f"between_limits_inertial_{int(inertial)}", make_kf(T0, [obs(T0, G)]),
                        [make_kf(Ta, [obs(Ta, G)]), EMPTY()], [[0], [-1]], [[st], [NP_NO_MATCH]], [[0]] * 2, [[br], [B_]],
                        prm=Params(inertial=inertial, ratio_factor=RATIO_FACTOR), x3d={} if inertial else {(0, 0): G}))

    # not rigid poses (see the module docstring): A = diag(-1, -1.5, 2, 2) and rays at cos = 0.9
    Tw1 = np.array([[1, 0, 0, 0], [0, 1.5, 0, 0], [0, 0, 1, 0]], float)
    Tw2 = np.array([[0, 0, -2, 0], [0, 0, 0, -2], [np.sqrt(1 - 0.81), 0, 0.9, 0]], float)
    centre = dict(x=CX, y=CY, octave=0, ur=-1.0, depth=-1.0, raw=None)
    out.append(Case("tri_w_zero", make_kf(Tw1, [centre], Ow=(0, 0, 0)), [make_kf(Tw2, [centre], Ow=(1, 0, 0)), EMPTY()],
                    [[0], [-1]], [[NP_TRI_W_ZERO], [NP_NO_MATCH]], [[0]] * 2, [[T_], [B_]]))

    # a stereo keypoint whose mvDepth is -1: cos(2 atan2(0.05, -1)) = 0.995 against rays at 0.999997
    out.append(Case("stereo_depth", make_kf(T0, [obs(T0, F, stereo=True, depth=-1.0)]),
                    [make_kf(Ta, [obs(Ta, F)]), EMPTY()], [[0], [-1]], [[NP_STEREO_DEPTH], [NP_NO_MATCH]],
                    [[1], [0]], [[S1], [B_]]))

    # 2 m away: the stereo parallax (0.1 m, cos 0.99875) beats a 0.05 m baseline (cos 0.99969): unprojection
    # from keyframe 1, and from the neighbour when only its keypoint is stereo; with a 0.5 m baseline the same
    # stereo keypoint is triangulated (and tested with the 3-dof chi-square)
    N = (0.1, 0.05, 2.0)
    Ts = pose((0.05, 0, 0))
    out.append(Case("stereo_1", make_kf(T0, [obs(T0, N, stereo=True)]), [make_kf(Ts, [obs(Ts, N)]), EMPTY()],
                    [[0], [-1]], [[NP_OK], [NP_NO_MATCH]], [[1], [0]], [[S1], [B_]], x3d={(0, 0): N}))
    out.append(Case("stereo_2", make_kf(T0, [obs(T0, N)]), [EMPTY(), make_kf(Ts, [obs(Ts, N, stereo=True)])],
                    [[-1], [0]], [[NP_NO_MATCH], [NP_OK]], [[0], [1]], [[B_], [S2]], x3d={(1, 0): N}))
    out.append(Case("stereo_triangulated", make_kf(T0, [obs(T0, N, stereo=True)]),
                    [make_kf(Ta, [obs(Ta, N, stereo=True)]), EMPTY()], [[0], [-1]], [[NP_OK], [NP_NO_MATCH]], [[0]] * 2,
                    [[T_], [B_]], x3d={(0, 0): N}))

    # mvKeys 3 px right and 2 px up of mvKeysUn: UnprojectStereo reads mvKeys, so x3D moves by (3, -2) * 2 / 500;
    # octave 5 (7.8 * 6.19) lets the 22 px^2 this costs in keyframe 1 pass
    out.append(Case("raw_keys", make_kf(T0, [obs(T0, N, octave=5, stereo=True, raw_shift=(3.0, -2.0))]),
                    [make_kf(Ts, [obs(Ts, N, octave=5)]), EMPTY()], [[0], [-1]], [[NP_OK], [NP_NO_MATCH]], [[1], [0]],
                    [[S1], [B_]], x3d={(0, 0): (N[0] + 3 * 2 / 500, N[1] - 2 * 2 / 500, N[2])}))

    # the two observations swapped in u: the lines meet behind both cameras
    out.append(Case("z1", make_kf(T0, [obs(T0, P, dx=-60.0)]), [make_kf(Ta, [obs(Ta, P, dx=60.0)]), EMPTY()],
                    [[0], [-1]], [[NP_Z1], [NP_NO_MATCH]], [[0]] * 2, [[T_], [B_]]))

    # the point lies 5 m behind the neighbour (its line, not its ray, passes through it)
    Tz = pose((0.5, 0, 10.0))
    out.append(Case("z2", make_kf(T0, [obs(T0, (0, 0, 5.0))]), [EMPTY(), make_kf(Tz, [obs(Tz, (0, 0, 5.0))])],
                    [[-1], [0]], [[NP_NO_MATCH], [NP_Z2]], [[0]] * 2, [[B_], [T_]]))

    # a camera centre that is not the pose's (see the module docstring): keyframe 1 unprojects its stereo keypoint
    # at the principal point to exactly (0, 0, 4), which the neighbour reports as its centre
    centre4 = dict(x=CX, y=CY, octave=0, ur=CX - MBF / 4.0, depth=4.0, raw=None)
    Tn = pose((0.05, 0, 0))
    out.append(Case("dist_zero", make_kf(T0, [centre4], Ow=(0, 0, 0)),
                    [make_kf(Tn, [obs(Tn, (0, 0, 4.0))], Ow=(0, 0, 4.0)), EMPTY()], [[0], [-1]],
                    [[NP_DIST_ZERO], [NP_NO_MATCH]], [[1], [0]], [[S1], [B_]]))

    # mbFarPoints with a 3 m limit against a point 5 m away; the same scene without the flag
    for far, st in ((True, NP_FAR), (False, NP_OK)):
        out.append(Case(f"far_points_{int(far)}", make_kf(T0, [obs(T0, P)]), [make_kf(Ta, [obs(Ta, P)]), EMPTY()],
                        [[0], [-1]], [[st], [NP_NO_MATCH]], [[0]] * 2, [[T_], [B_]],
                        prm=Params(far_points=far, th_far_points=3.0, ratio_factor=RATIO_FACTOR)))

    # equal distances, octaves 0 and 7: ratioDist 1 > ratioOctave 0.279 * 1.8
    out.append(Case("scale", make_kf(T0, [obs(T0, P)]), [make_kf(Ta, [obs(Ta, P, octave=7)]), EMPTY()], [[0], [-1]],
                    [[NP_SCALE], [NP_NO_MATCH]], [[0]] * 2, [[T_], [B_]]))

    # two idx1 half a pixel apart share idx2 0 of neighbour 0: both are created (the caller's second AddMapPoint
    # to idx2 overwrites the first)
    out.append(Case("shared_idx2", make_kf(T0, [obs(T0, P), obs(T0, P, dx=0.5)]), [make_kf(Ta, [obs(Ta, P)]), EMPTY()],
                    [[0, 0], [-1, -1]], [[NP_OK, NP_OK], [NP_NO_MATCH] * 2], [[0, 0]] * 2, [[T_, T_], [B_, B_]]))

    # neighbour 0 flagged ORB_ERR_CAPACITY by the search: its (stale) matches yield nothing, neighbour 1 creates
    out.append(Case("capacity_flag", make_kf(T0, [obs(T0, P)]), [make_kf(Ta, [obs(Ta, P)]), make_kf(Tb, [obs(Tb, P)])],
                    [[0], [0]], [[NP_NO_MATCH], [NP_OK]], [[0]] * 2, [[B_], [T_]], n_matches=[ref.ORB_ERR_CAPACITY, 1]))
    return out


RANDOM_SEED = 5
RANDOM_MB = 0.25  # a stereo baseline inside the range of the keyframe baselines: all three branches occur


def random_scene(seed=RANDOM_SEED, n_neighbours=3, n_points=300, p_stereo=0.5):
    """Keyframe 1 at the origin and neighbours 0.1-0.5 m away, ~n_points keypoints each: world points 2-10 m
    deep, 1 px observation noise, about half the keypoints stereo (mb = 0.25 m), octaves following the depth, matches12
    synthesised (about 80 % of the keypoints matched per neighbour, 10 % of those to a wrong keypoint).
    Returns (kf1, kf2s, matches12 [P, N1] int32, prm)."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.0, 10.0, n_points)
    W = np.stack([rng.uniform(-0.5, 0.5, n_points) * z, rng.uniform(-0.4, 0.4, n_points) * z, z], 1)

    def keyframe(Tcw, order):
        kps = []
        for w in order:
            depth = project(Tcw, W[w])[2]
            octave = int(np.clip(np.round(np.log(depth / 2.0) / np.log(1.2)) + rng.integers(-1, 2), 0, NLEVELS - 1))
            stereo = bool(rng.random() < p_stereo)
            o = obs(Tcw, W[w], octave=octave, stereo=stereo, dx=rng.normal(0, 1.0), dy=rng.normal(0, 1.0),
                    depth=depth * (1 + rng.normal(0, 0.01)))
            if stereo:
                o["ur"] = o["x"] - RANDOM_MB * FX / o["depth"]
            kps.append(o)
        return make_kf(Tcw, kps, stereo_arrays=True, mb=RANDOM_MB)

    kf1 = keyframe(T0, range(n_points))
    kf2s, m12 = [], np.full((n_neighbours, n_points), -1, np.int32)
    for p in range(n_neighbours):
        b = rng.uniform(0.1, 0.5)
        a = rng.uniform(0, 2 * np.pi)
        c = (b * np.cos(a), 0.3 * b * np.sin(a), rng.uniform(-0.3, 0.3) * b)
        order = rng.permutation(n_points)[:n_points - 7 * p]  # neighbours of different sizes
        kf2s.append(keyframe(pose(c, yaw=rng.normal(0, 0.03), pitch=rng.normal(0, 0.03)), order))
        where = {int(w): j for j, w in enumerate(order)}
        for i in range(n_points):
            if i in where and rng.random() < 0.8:
                m12[p, i] = where[i] if rng.random() >= 0.1 else rng.integers(0, len(order))
    return kf1, kf2s, m12, Params(ratio_factor=RATIO_FACTOR)


_RANDOM: dict = {}


def random_truth():
    """The random scene with its float64 restatement, computed once and shared: dict(kf1, kf2s, m12, prm, truth
    [P][N1], decisive [P, N1] bool over the matched jobs, matched [P, N1] bool)."""
    if not _RANDOM:
        kf1, kf2s, m12, prm = random_scene()
        rows = ref.truth_all(kf1, kf2s, m12, prm)
        matched = m12 >= 0
        decisive = np.array([[t["margin"] > ref.DECISIVE for t in row] for row in rows]) & matched
        _RANDOM.update(kf1=kf1, kf2s=kf2s, m12=m12, prm=prm, truth=rows, decisive=decisive, matched=matched)
    return _RANDOM
