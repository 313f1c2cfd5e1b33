"""Scenes for ORBmatcher::Fuse: keyframes on an arc looking at one point cloud, as
LocalMapping::SearchInNeighbors meets them (a new keyframe's map points projected into its neighbours).
Kept out of orbslam3_amd.synth so that the random streams of the existing scenes do not move."""
from __future__ import annotations

import numpy as np

import conftest

pkg = conftest.load_package()
from orbslam3_amd._lib import KEYPOINT_DTYPE  # noqa: E402
from orbslam3_amd.keyframe import Frame, FusePoints, logf  # noqa: E402

WIDTH, HEIGHT = 640, 480
CAMERA = (500.0, 500.0, 320.0, 240.0)
BF = 40.0
NLEVELS, SCALE = 8, 1.2


def scale_factors(nlevels=NLEVELS, scale=SCALE):
    """mvScaleFactors as ORBextractor builds them (src/ORBextractor.cc:476-483): float products."""
    s = np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        s[i] = np.float32(s[i - 1] * np.float32(scale))
    return s


def inv_level_sigma2(s):
    return (np.float32(1.0) / (s * s).astype(np.float32)).astype(np.float32)  # src/ORBextractor.cc:480-489


def look_at(C, target):
    """Tcw (3 x 4) of a camera at C looking at target (x right, y down, z forward; world y is down)."""
    f = (target - C) / np.linalg.norm(target - C)
    r = np.cross(np.array([0.0, 1.0, 0.0]), f)
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack([r, d, f])
    return np.concatenate([R, (-R @ C)[:, None]], axis=1)


def flip_bits(rng, desc, k):
    bits = np.unpackbits(desc)
    bits[rng.choice(256, size=k, replace=False)] ^= 1
    return np.packbits(bits)


def make_scene(n_kfs=3, n_points=300, seed=0, stereo=True, n_clutter=150, p_obs=0.75, skip_fraction=0.1):
    """Returns dict(kfs=[Frame], points=FusePoints, skip=uint8 [K, n]).  Point classes (by index, shuffled):
    most points lie in front of every camera; a few lie behind the arc (depth), far to the side (image),
    carry a shrunk distance range (distance) or a normal turned away (normal)."""
    rng = np.random.default_rng(seed)
    s = scale_factors()
    inv_s2 = inv_level_sigma2(s)
    lsf = float(logf(SCALE))
    fx, fy, cx, cy = CAMERA
    centre = np.array([0.0, 0.0, 7.0])
    angles = np.linspace(-0.15, 0.15, n_kfs) if n_kfs > 1 else np.array([0.05])
    cams = [np.array([7.0 * np.sin(a), 0.0, 7.0 - 7.0 * np.cos(a)]) for a in angles]
    C_ref = np.zeros(3)

    n = n_points
    pos = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(4, 10, n)], axis=1)
    kind = rng.choice(5, size=n, p=[0.8, 0.05, 0.05, 0.05, 0.05])  # 0 plain, 1 behind, 2 aside, 3 range, 4 normal
    pos[kind == 1, 2] = rng.uniform(-5, -1, int((kind == 1).sum()))
    pos[kind == 2, 0] = rng.choice([-1.0, 1.0], int((kind == 2).sum())) * rng.uniform(8, 12, int((kind == 2).sum()))
    view = pos - C_ref
    d_ref = np.linalg.norm(view, axis=1)
    normal = view / d_ref[:, None]
    for i in np.flatnonzero(kind == 4):  # turned 75 .. 120 degrees away about the y axis
        a = rng.uniform(np.radians(75), np.radians(120)) * rng.choice([-1.0, 1.0])
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        normal[i] = R @ normal[i]
    level_ref = rng.integers(0, 5, n)
    max_dist = d_ref * s[level_ref].astype(np.float64)
    max_dist[kind == 3] *= rng.choice([0.3, 4.0], int((kind == 3).sum()))
    min_dist = max_dist / float(s[-1])
    base = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pts = FusePoints(pos, normal, min_dist, max_dist, base)

    kfs = []
    for C in cams:
        T = look_at(C, centre)
        kps, descs, urs = [], [], []

        def add(u, v, octave, desc, z):
            kp = np.zeros((), KEYPOINT_DTYPE)
            kp["x"], kp["y"], kp["octave"], kp["size"], kp["class_id"] = u, v, octave, 31.0 * s[octave], -1
            kps.append(kp)
            descs.append(desc)
            has_ur = stereo and z is not None and rng.random() < 0.5
            urs.append(u - BF / z + rng.normal(0, 0.3) if has_ur else -1.0)

        for i in range(n):
            Pc = T[:, :3] @ pts.pos[i].astype(np.float64) + T[:, 3]
            if Pc[2] <= 0.1 or rng.random() > p_obs:
                continue
            u, v = fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy
            if not (5 <= u < WIDTH - 5 and 5 <= v < HEIGHT - 5):
                continue
            dist = np.linalg.norm(pts.pos[i] - C)
            level = int(np.clip(np.ceil(np.log(float(pts.max_dist[i]) / dist) / np.log(SCALE)), 0, NLEVELS - 1))
            roll = rng.random()
            octave = level if roll < 0.5 else level - 1 if roll < 0.9 else level + rng.choice([-2, 2])
            octave = int(np.clip(octave, 0, NLEVELS - 1))
            sigma = (3.0 if rng.random() < 0.1 else 0.6) * float(s[octave])  # a tenth fails the chi-square gate
            flips = int(rng.integers(80, 120)) if rng.random() < 0.1 else int(rng.integers(0, 30))
            d = flip_bits(rng, pts.desc[i], flips)
            uu, vv = u + rng.normal(0, sigma), v + rng.normal(0, sigma)
            add(uu, vv, octave, d, Pc[2])
            if rng.random() < 0.05:  # a second keypoint with the same descriptor next to it: a distance tie
                add(uu + rng.uniform(-1, 1), vv + rng.uniform(-1, 1), octave, d, Pc[2])
        for _ in range(n_clutter):
            add(rng.uniform(0, WIDTH), rng.uniform(0, HEIGHT), int(rng.integers(0, NLEVELS)),
                rng.integers(0, 256, 32, dtype=np.uint8), None)
        order = rng.permutation(len(kps))  # keypoint order is unrelated to point order
        kps = np.array(kps, KEYPOINT_DTYPE)[order] if kps else np.zeros(0, KEYPOINT_DTYPE)
        descs = np.array(descs, np.uint8).reshape(-1, 32)[order]
        urs = np.array(urs, np.float32)[order]
        kfs.append(Frame(kps, descs, T.astype(np.float32), CAMERA, s, WIDTH, HEIGHT, bf=BF,
                         u_right=urs if stereo else None, Ow=C.astype(np.float32), inv_level_sigma2=inv_s2,
                         log_scale_factor=lsf))
    skip = (rng.random((n_kfs, n)) < skip_fraction).astype(np.uint8)
    return dict(kfs=kfs, points=pts, skip=skip)
