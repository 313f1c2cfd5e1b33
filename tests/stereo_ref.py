"""Second reference of Frame::ComputeStereoMatches: a loop-by-loop Python reading of reference
src/Frame.cc:1102-1358 with np.float32 scalars where the reference uses float.

It is independent of the C oracle (oracle/orb_stereo_oracle.cpp) and of the package: it calls
neither.  Besides (mvuRight, mvDepth, kept) it says, per left keypoint, why the keypoint ended as it
did (REASONS), and for every accepted match the winning SAD and window offset, so that built cases
(tests/stereo_cases.py) can pin each gate.

It is defined on caller-supplied keypoints: a left keypoint whose row is outside the image is
skipped, and so are the SAD windows that leave the level view on the left, top or bottom, where the
reference's cv::Mat::rowRange / colRange would throw (:1244, :1255).
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

REASONS = ("no_row_candidates", "hamming_ge_75", "window_right_edge", "window_view_bound", "best_at_minus_L",
           "best_at_plus_L", "disparity_negative", "disparity_ge_max", "clamped_zero", "matched", "culled")
# |deltaR| > 1 (:1308) cannot happen after a first strict minimum inside (-L, L): dist1 > dist2 <= dist3
# bounds the parabola's vertex by 1/2.  The code exists so that the restatement is complete.
UNREACHABLE = "delta_out_of_range"

TH_HIGH, TH_LOW = 100, 50  # ORBmatcher::TH_HIGH / TH_LOW
W, L = 5, 5                # SAD window half size / search half range, :1237-1238


class StereoResult(NamedTuple):
    u_right: np.ndarray   # float32 [n_l], -1 = no match
    depth: np.ndarray     # float32 [n_l]
    kept: int
    reasons: list         # one of REASONS per left keypoint
    best_idx: np.ndarray  # int [n_l]: right index the Hamming search chose (-1: the search found none < TH_HIGH)
    best_dist: np.ndarray  # int [n_l]: its distance (TH_HIGH if none)
    sad: np.ndarray       # int [n_l]: winning SAD of accepted matches (before the cull), -1 otherwise
    offset: np.ndarray    # int [n_l]: winning incR of accepted matches, 0 otherwise
    sads: dict            # iL -> the 11 SADs of the window search (every keypoint that reached it)
    candidates: dict      # iL -> [(iR, distance)] that passed every gate, in ascending iR


def popcount_dist(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def _round(v):  # std::round: half away from zero
    v = float(v)
    return np.float32(math.copysign(math.floor(abs(v) + 0.5), v))


def stereo_ref(kl, dl, kr, dr, planes_l, planes_r, scale, inv_scale, bf, b) -> StereoResult:
    f32 = np.float32
    n = len(kl)
    ur = np.full(n, -1.0, np.float32)
    dp = np.full(n, -1.0, np.float32)
    reasons = [None] * n
    best_idx = np.full(n, -1, np.int64)
    best_dist = np.full(n, TH_HIGH, np.int64)
    sad = np.full(n, -1, np.int64)
    offset = np.zeros(n, np.int64)
    all_sads, all_cands = {}, {}
    th_orb = (TH_HIGH + TH_LOW) // 2
    n_rows = planes_l[0].shape[0] - 38                               # mvImagePyramid[0].rows, :1126
    rows = [[] for _ in range(n_rows)]
    for ir in range(len(kr)):                                        # :1134-1152
        y = f32(kr[ir]["y"])
        r = f32(f32(2.0) * f32(scale[kr[ir]["octave"]]))
        for yi in range(math.floor(f32(y - r)), math.ceil(f32(y + r)) + 1):
            if 0 <= yi < n_rows:
                rows[yi].append(ir)
    min_d = f32(0)
    max_d = f32(f32(bf) / f32(b))                                    # :1160-1163
    pairs = []
    for il in range(n):
        kp = kl[il]
        lvl = int(kp["octave"])
        vl, ul = f32(kp["y"]), f32(kp["x"])
        row = int(vl)                                                # (size_t)vL
        if row < 0 or row >= n_rows:
            reasons[il] = "no_row_candidates"
            continue
        cand = rows[row]
        if not cand:
            reasons[il] = "no_row_candidates"
            continue
        min_u, max_u = f32(ul - max_d), f32(ul - min_d)
        if max_u < 0:
            reasons[il] = "no_row_candidates"
            continue
        best, best_i = TH_HIGH, 0
        passed = []
        for ir in cand:                                              # :1195-1220
            o = int(kr[ir]["octave"])
            if o < lvl - 1 or o > lvl + 1:
                continue
            u = f32(kr[ir]["x"])
            if min_u <= u <= max_u:
                d = popcount_dist(dl[il], dr[ir])
                passed.append((ir, d))
                if d < best:
                    best, best_i = d, ir
        all_cands[il] = passed
        best_dist[il] = best
        if best < TH_HIGH:
            best_idx[il] = best_i
        if best >= th_orb:                                           # :1223
            reasons[il] = "hamming_ge_75"
            continue
        sf = f32(inv_scale[lvl])
        su_l, sv_l = _round(f32(ul * sf)), _round(f32(vl * sf))       # :1231-1234
        su_r = _round(f32(f32(kr[best_i]["x"]) * sf))
        lw, lh = planes_r[lvl].shape[1] - 38, planes_r[lvl].shape[0] - 38
        iniu = f32(f32(su_r + f32(L)) - f32(W))
        endu = f32(f32(f32(su_r + f32(L)) + f32(W)) + f32(1))
        if iniu < 0 or endu >= lw:                                   # :1262-1265
            reasons[il] = "window_right_edge"
            continue
        cu_l, cv_l, cu_r = int(su_l), int(sv_l), int(su_r)
        if cu_r - L - W < 0 or cv_l - W < 0 or cv_l + W >= lh or cu_l - W < 0 or cu_l + W >= lw:
            reasons[il] = "window_view_bound"                        # cv::Mat ranges would throw
            continue
        il_img = planes_l[lvl][19:-19, 19:-19].astype(np.int64)
        ir_img = planes_r[lvl][19:-19, 19:-19].astype(np.int64)
        patch = il_img[cv_l - W:cv_l + W + 1, cu_l - W:cu_l + W + 1]
        dists = []
        best_s, best_inc = None, 0
        for inc in range(-L, L + 1):                                 # :1267-1280
            s = f32(np.abs(patch - ir_img[cv_l - W:cv_l + W + 1, cu_r + inc - W:cu_r + inc + W + 1]).sum())
            if best_s is None or s < best_s:
                best_s, best_inc = s, inc
            dists.append(s)
        all_sads[il] = [int(s) for s in dists]
        if best_inc == -L:                                           # :1282
            reasons[il] = "best_at_minus_L"
            continue
        if best_inc == L:
            reasons[il] = "best_at_plus_L"
            continue
        d1, d2, d3 = dists[L + best_inc - 1], dists[L + best_inc], dists[L + best_inc + 1]
        with np.errstate(all="ignore"):
            delta = f32(f32(d1 - d3) / f32(f32(2.0) * f32(f32(d1 + d3) - f32(f32(2.0) * d2))))
        if delta < -1 or delta > 1:                                  # :1308
            reasons[il] = UNREACHABLE
            continue
        best_u = f32(f32(scale[lvl]) * f32(f32(f32(su_r) + f32(best_inc)) + delta))
        disp = f32(ul - best_u)
        if not disp >= min_d:                                        # :1315
            reasons[il] = "disparity_negative"
            continue
        if not disp < max_d:
            reasons[il] = "disparity_ge_max"
            continue
        reasons[il] = "matched"
        if disp <= 0:                                                # :1317-1321, double literals
            disp = f32(0.01)
            best_u = f32(float(ul) - 0.01)
            reasons[il] = "clamped_zero"
        dp[il] = f32(f32(bf) / disp)
        ur[il] = best_u
        sad[il] = int(best_s)
        offset[il] = best_inc
        pairs.append((int(best_s), il))
    kept = len(pairs)
    if pairs:                                                        # :1334-1352
        pairs.sort()
        median = f32(pairs[len(pairs) // 2][0])
        th = f32(f32(f32(1.5) * f32(1.4)) * median)
        for d, il in reversed(pairs):
            if f32(d) < th:
                break
            ur[il] = dp[il] = -1.0
            reasons[il] = "culled"
            kept -= 1
    return StereoResult(ur, dp, kept, reasons, best_idx, best_dist, sad, offset, all_sads, all_cands)


def python_stereo(kl, dl, kr, dr, planes_l, planes_r, scale, inv_scale, bf, b):
    """(mvuRight, mvDepth, kept) alone."""
    r = stereo_ref(kl, dl, kr, dr, planes_l, planes_r, scale, inv_scale, bf, b)
    return r.u_right, r.depth, r.kept
