"""Python restatement of the search half of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th)
(reference src/ORBmatcher.cc:1356-1506) with KeyFrame::GetFeaturesInArea / IsInImage (src/KeyFrame.cc:
843-897), Frame::AssignFeaturesToGrid for KeyFrame::mGrid (src/Frame.cc:1418-1440, NLeft == -1) and
MapPoint::PredictScale (src/MapPoint.cc:688-706): what the GPU tests compare against.

Float32 arithmetic is exact: +, -, *, / and sqrt are numpy float32 operations (IEEE, correctly rounded) and
the fused multiply-adds the reference build contracts (oracle/orb_projection_oracle.cpp: `a*b + c*d` ->
fma(a, b, c*d), `a - b*c` -> fma(-b, c, a)) round once -- fma32 below: the product is exact in double;
the double sum is used only where its rounding cannot have moved the float32 result (it is not a float32
rounding midpoint), and everything else goes through exact rational arithmetic.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import conftest

conftest.load_package()
from orbslam3_amd.keyframe import FRAME_GRID_COLS, FRAME_GRID_ROWS, logf  # noqa: E402

TH_LOW = 50
SKIPPED, DEPTH, IMAGE, DISTANCE, NORMAL, EMPTY_WINDOW, NO_CANDIDATE, ABOVE_TH_LOW, FUSED = range(9)
REASONS = ("skipped", "depth", "image", "distance", "normal", "empty window", "no candidate after the gates",
           "above TH_LOW", "fused")

f32 = np.float32


def round_fraction_f32(x: Fraction) -> np.float32:
    """x rounded to the nearest float32, ties to even (integer arithmetic only)."""
    if x == 0:
        return f32(0.0)
    sign = -1 if x < 0 else 1
    a = -x if x < 0 else x
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^(e-1) < a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, -126)             # subnormals share the smallest normal exponent's quantum
    q = Fraction(2) ** (e - 23)  # one unit in the last place
    m = a / q
    fl = m.numerator // m.denominator
    rem = m - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (fl & 1)):
        fl += 1
    if fl >= 1 << 24 and e >= 127 or e > 127:
        return f32(sign * math.inf)
    return f32(sign * math.ldexp(float(fl), e - 23))  # fl <= 2^24: exact


def fma32(a, b, c):
    """float32 fma(a, b, c) with a single rounding, elementwise."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    shape = a.shape
    a, b, c = (np.ascontiguousarray(v).reshape(-1) for v in (a, b, c))
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)  # the product is exact
        out = s.astype(f32)
    bits = s.view(np.uint64)
    # exact path wherever the double sum sits on a float32 rounding midpoint (its own rounding may have put
    # it there) or in / near the float32 subnormal range (another quantum)
    risky = np.isfinite(s) & (((bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) |
                              ((np.abs(s) < 2.0 ** -125) & (s != 0)))
    for i in np.flatnonzero(risky):
        out[i] = round_fraction_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out.reshape(shape) if shape else f32(out[0])


def dot3(a, b):
    """Eigen's 3-term sum as contracted: fma(a2, b2, fma(a0, b0, a1 * b1)); a, b [..., 3] float32."""
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 0], b[..., 0], a[..., 1] * b[..., 1]))


def descriptor_distance(a, b) -> int:
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def roundf(x):
    """C roundf (half away from zero) of float32 values, as ints."""
    x = np.asarray(x, np.float64)
    return np.trunc(x + np.copysign(0.5, x)).astype(np.int64)


def assign_features_to_grid(kf):
    """mGrid[ix][iy]: keypoint indices in index order (Frame::PosInGrid: round((x - mnMinX) * inv))."""
    grid = [[[] for _ in range(FRAME_GRID_ROWS)] for _ in range(FRAME_GRID_COLS)]
    if kf.N == 0:
        return grid
    x, y = kf.mvKeysUn["x"], kf.mvKeysUn["y"]
    px = roundf((x - f32(kf.mnMinX)) * f32(kf.mfGridElementWidthInv))
    py = roundf((y - f32(kf.mnMinY)) * f32(kf.mfGridElementHeightInv))
    for i in range(kf.N):
        if 0 <= px[i] < FRAME_GRID_COLS and 0 <= py[i] < FRAME_GRID_ROWS:
            grid[px[i]][py[i]].append(i)
    return grid


def get_features_in_area(kf, grid, x, y, r):
    """KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:843-891), all float32; the indices in scan order."""
    x, y, r = f32(x), f32(y), f32(r)
    minx, miny = f32(kf.mnMinX), f32(kf.mnMinY)
    iw, ih = f32(kf.mfGridElementWidthInv), f32(kf.mfGridElementHeightInv)
    x0 = max(0, int(math.floor(float((x - minx - r) * iw))))
    if x0 >= FRAME_GRID_COLS:
        return []
    x1 = min(FRAME_GRID_COLS - 1, int(math.ceil(float((x - minx + r) * iw))))
    if x1 < 0:
        return []
    y0 = max(0, int(math.floor(float((y - miny - r) * ih))))
    if y0 >= FRAME_GRID_ROWS:
        return []
    y1 = min(FRAME_GRID_ROWS - 1, int(math.ceil(float((y - miny + r) * ih))))
    if y1 < 0:
        return []
    kx, ky = kf.mvKeysUn["x"], kf.mvKeysUn["y"]
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for j in grid[ix][iy]:
                if abs(kx[j] - x) < r and abs(ky[j] - y) < r:
                    out.append(j)
    return out


def predict_scale(max_dist, dist, log_scale_factor, nlevels) -> int:
    """MapPoint::PredictScale: ceil(logf(mfMaxDistance / dist) / mfLogScaleFactor), float, clamped; the
    (int) of a non-finite float is INT_MIN on x86, clamped to 0."""
    with np.errstate(all="ignore"):
        ratio = f32(max_dist) / f32(dist)
        val = np.ceil(logf(ratio) / f32(log_scale_factor))
    n = int(val) if np.isfinite(val) else -(1 << 31)
    return 0 if n < 0 else min(n, nlevels - 1)


def fuse_search(kfs, points, th=3.0, skip=None):
    """For every job (keyframe k, point i): best_idx, best_dist [K, n] int32 as orb_fuse writes them, the
    reason code [K, n], and detail arrays u, v, ur [K, n] float32 (NaN before the image test passed) and
    level [K, n] (-1 before PredictScale ran).  kfs: orbslam3_amd Frame objects with the Fuse fields;
    points: orbslam3_amd FusePoints."""
    K, n = len(kfs), points.n
    best_idx = np.full((K, n), -1, np.int32)
    best_dist = np.full((K, n), 256, np.int32)
    reason = np.full((K, n), SKIPPED, np.int32)
    det = dict(u=np.full((K, n), np.nan, f32), v=np.full((K, n), np.nan, f32), ur=np.full((K, n), np.nan, f32),
               level=np.full((K, n), -1, np.int32))
    th = f32(th)
    skip = None if skip is None else np.asarray(skip, np.uint8).reshape(K, n)
    P, Pn = points.pos, points.normal
    for k, kf in enumerate(kfs):
        kf.fuse_view()  # fills the defaults of Ow / mvInvLevelSigma2 / mfLogScaleFactor
        if n == 0:
            continue
        T = kf.Tcw.astype(f32)
        grid = assign_features_to_grid(kf)
        with np.errstate(all="ignore"):
            Pc = np.stack([fma32(T[r, 2], P[:, 2], fma32(T[r, 0], P[:, 0], T[r, 1] * P[:, 1])) + T[r, 3]
                           for r in range(3)], axis=1).astype(f32)
            invz = f32(1.0) / Pc[:, 2]
            u = f32(kf.fx) * Pc[:, 0] / Pc[:, 2] + f32(kf.cx)
            v = f32(kf.fy) * Pc[:, 1] / Pc[:, 2] + f32(kf.cy)
            ur = fma32(-f32(kf.mbf), invz, u)
            PO = (P - kf.Ow.astype(f32)[None, :]).astype(f32)
            dist = np.sqrt(dot3(PO, PO)).astype(f32)
            cosd = dot3(PO, Pn)
            lo = f32(0.8) * points.min_dist
            hi = f32(1.2) * points.max_dist
        nlevels = len(kf.mvScaleFactors)
        for i in range(n):
            if skip is not None and skip[k, i]:
                continue
            if Pc[i, 2] < 0:
                reason[k, i] = DEPTH
                continue
            if not (u[i] >= f32(kf.mnMinX) and u[i] < f32(kf.mnMaxX) and v[i] >= f32(kf.mnMinY) and v[i] < f32(kf.mnMaxY)):
                reason[k, i] = IMAGE
                continue
            det["u"][k, i], det["v"][k, i], det["ur"][k, i] = u[i], v[i], ur[i]
            if dist[i] < lo[i] or dist[i] > hi[i]:
                reason[k, i] = DISTANCE
                continue
            if cosd[i] < f32(0.5) * dist[i]:
                reason[k, i] = NORMAL
                continue
            level = predict_scale(points.max_dist[i], dist[i], kf.mfLogScaleFactor, nlevels)
            det["level"][k, i] = level
            radius = th * kf.mvScaleFactors[level]
            cand = get_features_in_area(kf, grid, u[i], v[i], radius)
            if not cand:
                reason[k, i] = EMPTY_WINDOW
                continue
            bd, bi = 256, -1
            passed = 0
            for j in cand:
                kp = kf.mvKeysUn[j]
                oct_ = int(kp["octave"])
                if oct_ < level - 1 or oct_ > level:
                    continue
                ex, ey = u[i] - kp["x"], v[i] - kp["y"]
                inv = kf.mvInvLevelSigma2[oct_]
                if kf.mvuRight is not None and kf.mvuRight[j] >= 0:
                    er = ur[i] - kf.mvuRight[j]
                    e2 = fma32(er, er, fma32(ex, ex, ey * ey))
                    if float(f32(e2 * inv)) > 7.8:   # the float product against the double literal
                        continue
                else:
                    e2 = fma32(ex, ex, ey * ey)
                    if float(f32(e2 * inv)) > 5.99:
                        continue
                passed += 1
                d = descriptor_distance(points.desc[i], kf.mDescriptors[j])
                if d < bd:
                    bd, bi = d, j
            best_dist[k, i] = bd
            if bd <= TH_LOW:
                best_idx[k, i] = bi
                reason[k, i] = FUSED
            else:
                reason[k, i] = ABOVE_TH_LOW if passed else NO_CANDIDATE
    return best_idx, best_dist, reason, det
