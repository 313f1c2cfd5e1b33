"""Hand-built ORBmatcher::Fuse cases that pin the semantics of src/ORBmatcher.cc:1356-1506: identity pose,
camera centre at the origin, fx = fy = 128, depth 4 and pixel coordinates that are multiples of 1/32, so
every projection is exact in float and fma and plain arithmetic agree.  Used by test_fuse_ref_cpu.py (the
expected values below against the Python reference) and test_fuse_gpu.py (the library against both)."""
from __future__ import annotations

import numpy as np

import conftest
import fuse_ref as ref
from fuse_scenes import inv_level_sigma2, scale_factors

conftest.load_package()
from orbslam3_amd._lib import KEYPOINT_DTYPE  # noqa: E402
from orbslam3_amd.keyframe import Frame, FusePoints, logf  # noqa: E402

W, H, F, Z, BF = 640, 480, 128.0, 4.0, 40.0
S = scale_factors()


def desc_ones(n):
    """A descriptor with n leading one bits: two of them differ by the difference of their counts."""
    bits = np.zeros(256, np.uint8)
    bits[:n] = 1
    return np.packbits(bits)


def make_kf(kps, grid_inv=None):
    """kps: (x, y, octave, leading ones of the descriptor, u_right)."""
    k = np.zeros(len(kps), KEYPOINT_DTYPE)
    for i, (x, y, o, _, _) in enumerate(kps):
        k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, o
    d = np.array([desc_ones(p[3]) for p in kps], np.uint8).reshape(-1, 32)
    ur = np.array([p[4] for p in kps], np.float32)
    T = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(np.float32)
    kf = Frame(k, d, T, (F, F, W / 2, H / 2), S, W, H, bf=BF, u_right=ur, Ow=np.zeros(3, np.float32),
               inv_level_sigma2=inv_level_sigma2(S), log_scale_factor=float(logf(1.2)))
    if grid_inv is not None:
        kf.mfGridElementWidthInv, kf.mfGridElementHeightInv = grid_inv
    return kf


def point(u, v, level=0, ones=0, z=Z):
    """A map point projecting to (u, v) exactly, seen along its normal, whose predicted level is `level`
    (mfMaxDistance = dist * 1.2^(level - 0.5): half a level away from either step)."""
    P = np.array([(u - W / 2) * z / F, (v - H / 2) * z / F, z])
    dist = np.linalg.norm(P)
    mx = dist * 1.2 ** (level - 0.5)
    return dict(pos=P, normal=P / dist, max_dist=mx, min_dist=mx / float(S[-1]), desc=desc_ones(ones))


def points_of(*pts):
    return FusePoints(np.array([p["pos"] for p in pts]), np.array([p["normal"] for p in pts]),
                      [p["min_dist"] for p in pts], [p["max_dist"] for p in pts], np.array([p["desc"] for p in pts]))


def cases():
    """[(name, kf, FusePoints, th, expected best_idx, expected best_dist, expected reasons)]"""
    out = []
    centre = [(320.0, 240.0, 0, 0, -1.0)]

    # depth: exactly 0 is not `< 0.0f`: 1 / 0 and 0 / 0 fall out at IsInImage; so does -0.0; just below 0
    # is the depth test's
    p0 = point(320, 240)
    zs = []
    for pos in ([0, 0, 0], [1, 0, 0], [0, 0, -0.0], [0, 0, -1e-30], [0, 0, -4]):
        q = dict(p0)
        q["pos"] = np.array(pos, np.float64)
        zs.append(q)
    out.append(("depth", make_kf(centre), points_of(*zs), 3.0, [-1] * 5, [256] * 5,
                [ref.IMAGE, ref.IMAGE, ref.IMAGE, ref.DEPTH, ref.DEPTH]))

    # IsInImage is half open: u == mnMaxX / v == mnMaxY rejected, u == mnMinX / v == mnMinY accepted
    kf = make_kf([(1.0, 240.0, 0, 0, -1.0), (320.0, 1.0, 0, 0, -1.0)])
    out.append(("image", kf, points_of(point(640, 240), point(0, 240), point(320, 480), point(320, 0)), 3.0,
                [-1, 0, -1, 1], [256, 0, 256, 0], [ref.IMAGE, ref.FUSED, ref.IMAGE, ref.FUSED]))

    # the distance equal to either bound is accepted: 0.8f * 5 == 4 == dist and 1.2f * f32(10 / 3) == 4
    lo, hi, below, above = (dict(p0) for _ in range(4))
    lo.update(min_dist=5.0, max_dist=4.0)
    hi.update(min_dist=1.0, max_dist=np.float32(10.0 / 3.0))
    below.update(min_dist=np.nextafter(np.float32(5.0), np.float32(6.0)) + np.float32(1e-6), max_dist=4.0)
    above.update(min_dist=1.0, max_dist=np.float32(3.3))
    out.append(("distance", make_kf(centre), points_of(lo, hi, below, above), 3.0, [0, 0, -1, -1], [0, 0, 256, 256],
                [ref.FUSED, ref.FUSED, ref.DISTANCE, ref.DISTANCE]))

    # PO . Pn == 0.5 * dist accepted (the normal need not be a unit vector), the next float below rejected
    eq, lt = dict(p0), dict(p0)
    eq["normal"] = np.array([0, 0, 0.5])
    lt["normal"] = np.array([0, 0, np.nextafter(np.float32(0.5), np.float32(0))])
    out.append(("normal", make_kf(centre), points_of(eq, lt), 3.0, [0, -1], [0, 256], [ref.FUSED, ref.NORMAL]))

    # the level clamps: a ratio below 1 gives a negative level -> 0; 1.2^10 -> nlevels - 1
    near, far = dict(p0), dict(p0)
    near.update(max_dist=3.4, min_dist=1.0)
    far.update(max_dist=4.0 * 1.2 ** 10, min_dist=1.0)
    kf = make_kf([(320.0, 240.0, 0, 0, -1.0), (320.0, 240.0, 7, 0, -1.0)])
    out.append(("level_clamp0", kf, points_of(near), 3.0, [0], [0], [ref.FUSED]))
    out.append(("level_clamp7", kf, points_of(far), 3.0, [1], [0], [ref.FUSED]))

    # octave level - 2 and level + 1 rejected (their descriptors match exactly); level - 1 and level kept
    kf = make_kf([(320.0, 240.0, 1, 0, -1.0), (320.0, 240.0, 4, 0, -1.0), (320.0, 240.0, 2, 12, -1.0),
                  (320.0, 240.0, 3, 10, -1.0)])
    out.append(("octave", kf, points_of(point(320, 240, level=3)), 3.0, [3], [10], [ref.FUSED]))
    kf = make_kf([(320.0, 240.0, 1, 0, -1.0), (320.0, 240.0, 4, 0, -1.0)])
    out.append(("octave_none", kf, points_of(point(320, 240, level=3)), 3.0, [-1], [256], [ref.NO_CANDIDATE]))

    # chi-square gates (octave 0: mvInvLevelSigma2 = 1; ur = 320 - 40 / 4 = 310).  A stereo keypoint at the
    # projection whose u_R is 3 px off fails on er alone (9 > 7.8); the mono one behind it is taken.
    kf = make_kf([(320.0, 240.0, 0, 0, 313.0), (320.0, 240.0, 0, 20, -1.0)])
    out.append(("stereo_er", kf, points_of(point(320, 240)), 3.0, [1], [20], [ref.FUSED]))
    # ex = 2.5: 6.25 > 5.99 fails the mono gate and passes the stereo one (er = 0; 6.25 <= 7.8)
    kf = make_kf([(322.5, 240.0, 0, 0, -1.0), (322.5, 240.0, 0, 30, 310.0)])
    out.append(("chi2_thresholds", kf, points_of(point(320, 240)), 3.0, [1], [30], [ref.FUSED]))

    # bestDist == TH_LOW fused, 51 not (best_dist still reports it)
    out.append(("th_low", make_kf(centre), points_of(point(320, 240, ones=50), point(320, 240, ones=51)), 3.0,
                [0, -1], [50, 51], [ref.FUSED, ref.ABOVE_TH_LOW]))

    # a distance tie: keypoint 1 lies in grid column 31 (x in [305, 315)), keypoint 0 in column 32; the scan
    # is column-major, so the higher index is met first and the strict `<` keeps it
    kf = make_kf([(317.0, 240.0, 4, 7, -1.0), (313.0, 240.0, 4, 7, -1.0)])
    out.append(("tie_column", kf, points_of(point(316, 240, level=4)), 3.0, [1], [7], [ref.FUSED]))
    # inside one cell the lower index wins
    kf = make_kf([(317.0, 240.0, 4, 7, -1.0), (318.0, 240.0, 4, 7, -1.0)])
    out.append(("tie_cell", kf, points_of(point(316, 240, level=4)), 3.0, [0], [7], [ref.FUSED]))

    # windows clipped at each grid border (the last column holds x in [625, 635), the last row y in [465, 475));
    # keypoints 4 .. 7 round to cells outside the grid and are never candidates although they match exactly
    kf = make_kf([(1.0, 240.0, 0, 9, -1.0), (634.0, 240.0, 0, 9, -1.0), (320.0, 1.0, 0, 9, -1.0),
                  (320.0, 474.0, 0, 9, -1.0), (636.0, 240.0, 0, 0, -1.0), (320.0, 476.0, 0, 0, -1.0),
                  (-6.0, 240.0, 0, 0, -1.0), (320.0, -6.0, 0, 0, -1.0)])
    out.append(("borders", kf, points_of(point(0, 240), point(636, 240), point(320, 0), point(320, 476)), 3.0,
                [0, 1, 2, 3], [9, 9, 9, 9], [ref.FUSED] * 4))

    # GetFeaturesInArea's early returns that a point inside the image can reach: a grid finer than the image
    # (inverse cell sizes 0.2) puts the window's first column / row past the grid
    kf = make_kf([(100.0, 100.0, 0, 0, -1.0)], grid_inv=(0.2, 0.1))
    out.append(("early_return_x", kf, points_of(point(400, 100), point(100, 100)), 3.0, [-1, 0], [256, 0],
                [ref.EMPTY_WINDOW, ref.FUSED]))
    kf = make_kf([(100.0, 100.0, 0, 0, -1.0)], grid_inv=(0.1, 0.2))
    out.append(("early_return_y", kf, points_of(point(100, 400), point(100, 100)), 3.0, [-1, 0], [256, 0],
                [ref.EMPTY_WINDOW, ref.FUSED]))
    return out
