"""Scenes for loop closing's Sim3 searches (tests/sim3_projection_ref.py): one keyframe, a window of map points
built in image space so that every outcome of the per-point body occurs, and clusters of near-identical points
that compete for the same few keypoints, as the points of a loop candidate's covisible keyframes do (the same
landmark mapped several times).  Kept out of orbslam3_amd.synth so that the random streams of the existing
scenes do not move."""
from __future__ import annotations

import numpy as np

import conftest
import sim3_projection_ref as ref
from fuse_scenes import CAMERA, HEIGHT, NLEVELS, SCALE, WIDTH, flip_bits, look_at, scale_factors

pkg = conftest.load_package()
from orbslam3_amd._lib import KEYPOINT_DTYPE  # noqa: E402
from orbslam3_amd.keyframe import Frame, FusePoints, logf  # noqa: E402
from orbslam3_amd.matcher import sim3_pose  # noqa: E402

EMPTY = 70.0  # no keypoint has x < EMPTY and y < EMPTY: points projected there meet an empty window


def candidate_pose(T, s):
    """(Tcw, Ow) of the Sim3 (R, s t, s) around the SE3 T (3 x 4): the same camera at another map scale."""
    return sim3_pose(T[:, :3], np.float32(s) * T[:, 3].astype(np.float32), s)


def job(kf, first, count, mode, th, ratio, pose):
    return dict(kf=kf, first=first, count=count, mode=mode, th=th, ratio=ratio, Tcw=pose[0], Ow=pose[1])


def make_scene(seed=0, n_points=300, n_clutter=60, cluster_share=0.55, th=8.0, kf_cap=None):
    """Returns dict(kf=Frame, points=FusePoints, T=the true pose 3 x 4 float64, skip=uint8 [n], taken0=uint8 [N]).
    Point classes: clusters of 2-5 points on one landmark (positions within a pixel, descriptors a few bits
    apart) over 1 .. size + 1 keypoints; lone points with one keypoint; and one class per early exit (behind
    the camera, beside the image, distance range, normal, empty window, wrong octave, far descriptor)."""
    rng = np.random.default_rng(seed)
    s = scale_factors()
    fx, fy, cx, cy = CAMERA
    C = np.array([0.4, -0.2, 0.3])
    T = look_at(C, np.array([0.0, 0.0, 7.0]))
    R, t = T[:, :3], T[:, 3]

    pts, kps = [], []   # dicts; (x, y, octave, desc)

    def add_point(u, v, z, level, desc, kind="plain"):
        Pc = np.array([(u - cx) * z / fx, (v - cy) * z / fy, z])
        Pw = R.T @ (Pc - t)
        d = np.linalg.norm(Pw - C)
        mx = d * SCALE ** (level - 0.5)      # half a level away from either PredictScale step
        nrm = (Pw - C) / d
        if kind == "range":
            mx *= rng.choice([0.3, 4.0])
        if kind == "normal":
            a = rng.uniform(np.radians(75), np.radians(120)) * rng.choice([-1.0, 1.0])
            nrm = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ nrm
        pts.append(dict(pos=Pw, normal=nrm, max_dist=mx, min_dist=mx / float(s[-1]), desc=desc))

    def pixel():
        while True:
            u, v = rng.uniform(20, WIDTH - 20), rng.uniform(20, HEIGHT - 20)
            if u > EMPTY + 30 or v > EMPTY + 30:
                return u, v

    n_cluster_pts = int(cluster_share * n_points)
    while len(pts) < n_cluster_pts:
        size = int(rng.integers(2, 6))
        (u, v), z, level = pixel(), rng.uniform(4, 10), int(rng.integers(0, 4))
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for _ in range(size):
            add_point(u + rng.uniform(-0.7, 0.7), v + rng.uniform(-0.7, 0.7), z * rng.uniform(0.99, 1.01), level,
                      flip_bits(rng, base, int(rng.integers(0, 8))))
        for _ in range(int(rng.integers(1, size + 2))):
            kps.append((u + rng.normal(0, 1.2), v + rng.normal(0, 1.2), max(level - int(rng.integers(0, 2)), 0),
                        flip_bits(rng, base, int(rng.integers(0, 14)))))
    special = ["behind", "aside", "range", "normal", "empty", "octave", "far"]
    n_special = max(2 * len(special), int(0.2 * n_points))
    for q in range(n_special):
        kind = special[q % len(special)]
        (u, v), z, level = pixel(), rng.uniform(4, 10), int(rng.integers(2, 5))
        desc = rng.integers(0, 256, 32, dtype=np.uint8)
        if kind == "behind":
            z = -z
        elif kind == "aside":
            u = WIDTH + rng.uniform(40, 300) if rng.random() < 0.5 else -rng.uniform(40, 300)
        elif kind == "empty":
            u, v = rng.uniform(15, EMPTY - 35), rng.uniform(15, EMPTY - 35)
            level = 0
        elif kind == "octave":
            kps.append((u + 0.5, v - 0.5, level + 2 if rng.random() < 0.5 else level - 2, desc))
        elif kind == "far":
            kps.append((u + 0.5, v - 0.5, level, flip_bits(rng, desc, int(rng.integers(90, 120)))))
        add_point(u, v, z, level, desc, kind)
    while len(pts) < n_points:
        (u, v), z, level = pixel(), rng.uniform(4, 10), int(rng.integers(0, 5))
        desc = rng.integers(0, 256, 32, dtype=np.uint8)
        add_point(u, v, z, level, desc)
        if rng.random() < 0.8:
            kps.append((u + rng.normal(0, 1.0), v + rng.normal(0, 1.0), max(level - int(rng.integers(0, 2)), 0),
                        flip_bits(rng, desc, int(rng.integers(0, 70)))))
    for _ in range(n_clutter):
        u, v = pixel()
        kps.append((u, v, int(rng.integers(0, NLEVELS)), rng.integers(0, 256, 32, dtype=np.uint8)))
    if kf_cap is not None:
        kps = kps[:kf_cap]

    order = rng.permutation(len(pts))[:n_points]
    pts = [pts[i] for i in order]
    points = FusePoints(np.array([p["pos"] for p in pts]), np.array([p["normal"] for p in pts]),
                        [p["min_dist"] for p in pts], [p["max_dist"] for p in pts], np.array([p["desc"] for p in pts]))
    korder = rng.permutation(len(kps))
    k = np.zeros(len(kps), KEYPOINT_DTYPE)
    for dst, src in enumerate(korder):
        x, y, o, _ = kps[src]
        k[dst]["x"], k[dst]["y"], k[dst]["octave"] = x, y, int(np.clip(o, 0, NLEVELS - 1))
        k[dst]["size"], k[dst]["class_id"] = 31.0 * s[k[dst]["octave"]], -1
    d = np.array([kps[src][3] for src in korder], np.uint8).reshape(-1, 32)
    kf = Frame(k, d, T.astype(np.float32), CAMERA, s, WIDTH, HEIGHT, log_scale_factor=float(logf(SCALE)))
    assert not ((k["x"] < EMPTY) & (k["y"] < EMPTY)).any()
    skip = (rng.random(len(pts)) < 0.06).astype(np.uint8)
    taken0 = (rng.random(kf.N) < 0.05).astype(np.uint8)
    return dict(kf=kf, points=points, T=T, skip=skip, taken0=taken0, th=th)


def three_mode_jobs(sc, ratio=1.5, scale=1.25):
    """One job per mode over the whole window, at the true pose taken from a Sim3 of another scale."""
    pose = candidate_pose(sc["T"], scale)
    n = sc["points"].n
    return [job(0, 0, n, mode, sc["th"], ratio, pose) for mode in (ref.CLAIM_PROJECT, ref.CLAIM_INVZ, ref.FUSE)]


def identity_kf(kps, W=640, H=480, F=128.0):
    """A keyframe at the identity pose; kps: (x, y, octave, desc)."""
    s = scale_factors()
    k = np.zeros(len(kps), KEYPOINT_DTYPE)
    for i, (x, y, o, _) in enumerate(kps):
        k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, o
    d = np.array([p[3] for p in kps], np.uint8).reshape(-1, 32)
    T = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
    return Frame(k, d, T, (F, F, W / 2, H / 2), s, W, H, log_scale_factor=float(logf(SCALE)))


IDENTITY_POSE = (np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32), np.zeros(3, np.float32))


def project_vs_invz_scene(seed=1):
    """A scene on which the two projection forms give different results: a point of predicted level 0 whose u
    differs in the last bit between Pinhole::project and :660-665, and a keypoint with the point's descriptor
    at x = min(u) + th (exact: level 0's radius is th), which GetFeaturesInArea's `|dx| < r` accepts only for
    the larger u.  Returns (scene, jobs [PROJECT, INVZ], the point's index)."""
    sc = make_scene(seed, n_points=120, n_clutter=30, th=5.0)
    kf, P = sc["kf"], sc["points"]
    pose = candidate_pose(sc["T"], 1.0)
    Pc = ref.transform(pose[0], P.pos)
    ua, va = ref.project(kf, Pc, False)
    ub, vb = ref.project(kf, Pc, True)
    ra = ref.search_by_projection(kf, pose[0], pose[1], P, 0, P.n, 5.0, 1.0)["reason"]
    rb = ref.search_by_projection_kfs(kf, pose[0], pose[1], P, 0, P.n, 5.0, 1.0)["reason"]
    unmatched = (ra >= ref.EMPTY_WINDOW) & (ra != ref.MATCHED) & (rb >= ref.EMPTY_WINDOW) & (rb != ref.MATCHED)
    for i in np.flatnonzero((ua != ub) & (va == vb) & unmatched):
        lo = min(ua[i], ub[i])
        x = np.float32(lo + np.float32(5.0))
        if float(x) - float(lo) != 5.0 or x >= WIDTH - 20:
            continue
        d = float(np.linalg.norm(P.pos[i] - pose[1]))
        if ref.predict_scale(P.max_dist[i], np.float32(d), kf.mfLogScaleFactor, NLEVELS) != 0:
            continue
        k = np.zeros(1, KEYPOINT_DTYPE)
        k[0]["x"], k[0]["y"], k[0]["octave"] = x, va[i], 0
        kf2 = Frame(np.concatenate([kf.mvKeysUn, k]), np.concatenate([kf.mDescriptors, P.desc[i:i + 1]]), kf.Tcw, CAMERA,
                    kf.mvScaleFactors, WIDTH, HEIGHT, log_scale_factor=kf.mfLogScaleFactor)
        sc2 = dict(sc, kf=kf2)
        jobs = [job(0, 0, P.n, m, 5.0, 1.0, pose) for m in (ref.CLAIM_PROJECT, ref.CLAIM_INVZ)]
        return sc2, jobs, int(i)
    raise AssertionError("no unmatched point of level 0 with a differing u: try another seed")


def ones_desc(n):
    bits = np.zeros(256, np.uint8)
    bits[:n] = 1
    return np.packbits(bits)


def image_point(u, v, level=0, desc=None, z=4.0, W=640, H=480, F=128.0):
    """A map point projecting to (u, v) exactly at the identity pose (fuse_cases.point's construction)."""
    P = np.array([(u - W / 2) * z / F, (v - H / 2) * z / F, z])
    dist = np.linalg.norm(P)
    mx = dist * 1.2 ** (level - 0.5)
    return dict(pos=P, normal=P / dist, max_dist=mx, min_dist=mx / float(scale_factors()[-1]),
                desc=ones_desc(0) if desc is None else desc)


def points_of(pts):
    return FusePoints(np.array([p["pos"] for p in pts]), np.array([p["normal"] for p in pts]),
                      [p["min_dist"] for p in pts], [p["max_dist"] for p in pts], np.array([p["desc"] for p in pts]))


def chain_scene(n_points=12, n_kps=12):
    """n_points points with one descriptor and n_kps keypoints with that descriptor inside every point's
    window (level 0, th 8: one window of 16 x 16 px around (320, 240)); the keypoints sit in different grid
    cells and are indexed against the scan order.  Point i takes the i-th keypoint of the scan: a chain longer
    than any kept list."""
    xs = [314.0 + (q % 4) * 4.0 for q in range(n_kps)]   # columns 31 .. 33
    ys = [234.0 + (q // 4) * 4.0 for q in range(n_kps)]
    kps = [(xs[q], ys[q], 0, ones_desc(7)) for q in reversed(range(n_kps))]
    kf = identity_kf(kps)
    pts = points_of([image_point(320.0, 240.0, 0, ones_desc(7)) for _ in range(n_points)])
    return kf, pts, [job(0, 0, n_points, ref.CLAIM_PROJECT, 8.0, 1.0, IDENTITY_POSE)]


def hand_cases():
    """[(name, kf, FusePoints, jobs, expected best_idx per job, expected reasons per job)] at the identity pose
    with exact projections (fx = 128, depth 4, pixel coordinates multiples of 1/32)."""
    out = []
    Z, O60 = ones_desc(0), ones_desc(60)
    # A point whose best candidate is claimed and whose next one is above the threshold matches nothing and
    # claims nothing: point 2 (descriptor of keypoint 1) still finds keypoint 1 free.  With ratio 1.5 (75) point
    # 1 takes keypoint 1 at distance 60 and point 2 is left without.
    kf = identity_kf([(320.0, 240.0, 0, Z), (321.0, 240.0, 0, O60)])
    pts = points_of([image_point(320, 240, 0, Z), image_point(320, 240, 0, Z), image_point(320, 240, 0, O60)])
    jobs = [job(0, 0, 3, m, 5.0, r, IDENTITY_POSE) for m in (ref.CLAIM_PROJECT, ref.CLAIM_INVZ) for r in (1.0, 1.5)]
    out.append(("claimed_next_above", kf, pts, jobs, [[0, -1, 1], [0, 1, -1]] * 2,
                [[ref.MATCHED, ref.ABOVE_TH, ref.MATCHED], [ref.MATCHED, ref.MATCHED, ref.NO_CANDIDATE]] * 2))
    # IsInImage is half open: u == mnMaxX / v == mnMaxY rejected, u == mnMinX / v == mnMinY accepted
    kf = identity_kf([(1.0, 240.0, 0, Z), (320.0, 1.0, 0, Z)])
    pts = points_of([image_point(640, 240), image_point(0, 240), image_point(320, 480), image_point(320, 0)])
    jobs = [job(0, 0, 4, m, 3.0, 1.0, IDENTITY_POSE) for m in (ref.CLAIM_PROJECT, ref.CLAIM_INVZ, ref.FUSE)]
    out.append(("image_edges", kf, pts, jobs, [[-1, 0, -1, 1]] * 3, [[ref.IMAGE, ref.MATCHED, ref.IMAGE, ref.MATCHED]] * 3))
    # depth exactly 0 (and -0.0) is not `< 0.0`: the division gives NaN or infinity and IsInImage rejects it
    p0 = image_point(320, 240)
    zs = []
    for pos in ([0, 0, 0], [1, 0, 0], [0, 0, -0.0], [0, 0, -1e-30], [0, 0, -4]):
        q = dict(p0)
        q["pos"] = np.array(pos, np.float64)
        zs.append(q)
    kf = identity_kf([(320.0, 240.0, 0, Z)])
    jobs = [job(0, 0, 5, m, 3.0, 1.0, IDENTITY_POSE) for m in (ref.CLAIM_PROJECT, ref.CLAIM_INVZ, ref.FUSE)]
    out.append(("depth_zero", kf, points_of(zs), jobs, [[-1] * 5] * 3,
                [[ref.IMAGE, ref.IMAGE, ref.IMAGE, ref.DEPTH, ref.DEPTH]] * 3))
    return out
