"""Python restatement of loop closing's three Sim3 searches, what the GPU tests compare against:
  search_by_projection      ORBmatcher::SearchByProjection(KF, Scw, vpPoints, vpMatched, th, ratioHamming)
                            (reference src/ORBmatcher.cc:496-619)
  search_by_projection_kfs  the overload that also fills vpMatchedKF (:621-733)
  fuse                      the search half of ORBmatcher::Fuse(KF, Scw, vpPoints, th, vpReplacePoint) (:1547-1651)
with KeyFrame::GetFeaturesInArea / IsInImage, KeyFrame::mGrid and MapPoint::PredictScale from tests/fuse_ref.py.
The loops are sequential and written line by line; the pose (Tcw, Ow) is the caller's (sim3_pose).

Float32 arithmetic is exact as in fuse_ref.py: the reference build contracts `a*b + c*d` to fma(a, b, c*d) and
`a*b + c` to fma(a, b, c) (oracle/orb_projection_oracle.cpp), so Tcw * p3Dw and the dot products round as there,
Pinhole::project is fx * x / z + cx in plain float operations, and :664's `fx*x+cx` is one fma.
"""
from __future__ import annotations

import numpy as np

from fuse_ref import (assign_features_to_grid, descriptor_distance, dot3, f32, fma32, get_features_in_area,
                      predict_scale)

TH_LOW = 50
CLAIM_PROJECT, CLAIM_INVZ, FUSE = 0, 1, 2
SKIPPED, DEPTH, IMAGE, DISTANCE, NORMAL, EMPTY_WINDOW, NO_CANDIDATE, ABOVE_TH, MATCHED = range(9)
REASONS = ("skipped", "depth", "image", "distance", "normal", "empty window",
           "no candidate (octave, or claimed by an earlier point)", "above the threshold", "matched")


def transform(Tcw, P):
    """Tcw * p3Dw for P [n, 3]: fma(R[r][2], P[2], fma(R[r][0], P[0], R[r][1] * P[1])) + t[r]."""
    T = np.asarray(Tcw, f32).reshape(3, 4)
    with np.errstate(all="ignore"):
        return np.stack([fma32(T[r, 2], P[:, 2], fma32(T[r, 0], P[:, 0], T[r, 1] * P[:, 1])) + T[r, 3]
                         for r in range(3)], axis=1).astype(f32)


def project(kf, Pc, invz_form: bool):
    """(u, v) of camera points Pc [n, 3]: Pinhole::project, or :660-665 when invz_form."""
    fx, fy, cx, cy = f32(kf.fx), f32(kf.fy), f32(kf.cx), f32(kf.cy)
    with np.errstate(all="ignore"):
        if invz_form:
            invz = f32(1.0) / Pc[:, 2]
            return fma32(fx, Pc[:, 0] * invz, cx), fma32(fy, Pc[:, 1] * invz, cy)
        return fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy


def _search(kf, Tcw, Ow, points, first, count, mode, th, ratio, skip, taken0):
    """One call of a reference function on points[first : first + count].  Returns a dict: matched [N]
    (the point that took each keypoint, -1), nmatches, best_idx / best_dist / reason [count], and first_choice
    [count]: the keypoint the point would take if no earlier point of this call had claimed anything (-1 none)."""
    kf.fuse_view()  # fills the default of mfLogScaleFactor
    n = count
    sl = slice(first, first + count)
    P, Pn = points.pos[sl], points.normal[sl]
    mind, maxd, desc = points.min_dist[sl], points.max_dist[sl], points.desc[sl]
    matched = np.full(kf.N, -1, np.int32)
    claimed = np.zeros(kf.N, bool) if taken0 is None else np.asarray(taken0[:kf.N], bool).copy()  # vpMatched[idx] != NULL
    best_idx = np.full(n, -1, np.int32)
    best_dist = np.full(n, 256, np.int32)
    reason = np.full(n, SKIPPED, np.int32)
    first_choice = np.full(n, -1, np.int32)
    out = dict(matched=matched, nmatches=0, best_idx=best_idx, best_dist=best_dist, reason=reason,
               first_choice=first_choice, u=np.full(n, np.nan, f32), v=np.full(n, np.nan, f32))
    if n == 0 or kf.N == 0:
        return out
    th = f32(th)
    thr = f32(TH_LOW) if mode == FUSE else f32(TH_LOW) * f32(ratio)   # int * float: a float product
    grid = assign_features_to_grid(kf)
    Pc = transform(Tcw, P)
    u, v = project(kf, Pc, mode == CLAIM_INVZ)
    with np.errstate(all="ignore"):
        PO = (P - np.asarray(Ow, f32)[None, :]).astype(f32)
        dist = np.sqrt(dot3(PO, PO)).astype(f32)
        cosd = dot3(PO, Pn)
        lo, hi = f32(0.8) * mind, f32(1.2) * maxd          # Get{Min,Max}DistanceInvariance
    nlevels = len(kf.mvScaleFactors)
    taken_before = claimed.copy()
    nmatches = 0
    for i in range(n):                                      # :520
        if skip is not None and skip[i]:                    # :526
            continue
        if Pc[i, 2] < 0.0:                                  # :538
            reason[i] = DEPTH
            continue
        if not (u[i] >= f32(kf.mnMinX) and u[i] < f32(kf.mnMaxX) and v[i] >= f32(kf.mnMinY) and v[i] < f32(kf.mnMaxY)):
            reason[i] = IMAGE                               # :546
            continue
        out["u"][i], out["v"][i] = u[i], v[i]
        if dist[i] < lo[i] or dist[i] > hi[i]:              # :557
            reason[i] = DISTANCE
            continue
        if cosd[i] < f32(0.5) * dist[i]:                    # :564
            reason[i] = NORMAL
            continue
        level = predict_scale(maxd[i], dist[i], kf.mfLogScaleFactor, nlevels)   # :568
        radius = th * kf.mvScaleFactors[level]              # :572
        cand = get_features_in_area(kf, grid, u[i], v[i], radius)               # :575
        if not cand:
            reason[i] = EMPTY_WINDOW
            continue
        bd, bi = 256, -1
        bd0, bi0 = 256, -1                                  # the same minimum with only the pre-filled entries claimed
        for j in cand:                                      # :586
            octave = int(kf.mvKeysUn[j]["octave"])
            if mode != FUSE and claimed[j]:                 # :589
                if not taken_before[j] and level - 1 <= octave <= level:
                    d = descriptor_distance(desc[i], kf.mDescriptors[j])
                    if d < bd0:
                        bd0, bi0 = d, j
                continue
            if octave < level - 1 or octave > level:        # :595
                continue
            d = descriptor_distance(desc[i], kf.mDescriptors[j])                # :600
            if d < bd:                                      # :602
                bd, bi = d, j
            if d < bd0:
                bd0, bi0 = d, j
        if f32(bd0) <= thr:
            first_choice[i] = bi0
        if mode == FUSE:
            best_dist[i] = bd
        if f32(bd) <= thr:                                  # :610 / :1655
            if mode != FUSE:
                claimed[bi] = True                          # vpMatched[bestIdx] = pMP
                matched[bi] = i
                best_dist[i] = bd
            best_idx[i] = bi
            nmatches += 1
            reason[i] = MATCHED
        else:
            reason[i] = ABOVE_TH if bi >= 0 else NO_CANDIDATE
    out["nmatches"] = nmatches
    return out


def search_by_projection(kf, Tcw, Ow, points, first, count, th, ratio, skip=None, taken0=None):
    return _search(kf, Tcw, Ow, points, first, count, CLAIM_PROJECT, th, ratio, skip, taken0)


def search_by_projection_kfs(kf, Tcw, Ow, points, first, count, th, ratio, skip=None, taken0=None):
    return _search(kf, Tcw, Ow, points, first, count, CLAIM_INVZ, th, ratio, skip, taken0)


def fuse(kf, Tcw, Ow, points, first, count, th, skip=None):
    return _search(kf, Tcw, Ow, points, first, count, FUSE, th, 1.0, skip, None)


def run_jobs(kfs, jobs, points, skip=None, taken0=None, stride=None):
    """The jobs of one ORBmatcher.SearchByProjectionSim3 call, each through its reference loop; the outputs in
    that call's layout plus `reason` and `first_choice` per point and `per_job` (the loops' own dicts)."""
    B = len(jobs)
    offs = np.zeros(B + 1, np.int64)
    for b, j in enumerate(jobs):
        offs[b + 1] = offs[b] + j["count"]
    T = int(offs[-1])
    if stride is None:
        stride = max([k.N for k in kfs] + [1])
    skip = None if skip is None else np.asarray(skip, np.uint8).reshape(-1)
    out = dict(matched=np.full((B, stride), -1, np.int32), nmatches=np.zeros(B, np.int32),
               best_idx=np.full(T, -1, np.int32), best_dist=np.full(T, 256, np.int32), offsets=offs,
               reason=np.full(T, SKIPPED, np.int32), first_choice=np.full(T, -1, np.int32), per_job=[])
    for b, j in enumerate(jobs):
        kf, s = kfs[j["kf"]], slice(int(offs[b]), int(offs[b + 1]))
        r = _search(kf, j["Tcw"], j["Ow"], points, j["first"], j["count"], j["mode"], j["th"], j.get("ratio", 1.0),
                    None if skip is None else skip[s], None if taken0 is None or j["mode"] == FUSE else taken0[b])
        if j["mode"] != FUSE:
            out["matched"][b, :kf.N] = r["matched"]
        out["nmatches"][b] = r["nmatches"]
        for k in ("best_idx", "best_dist", "reason", "first_choice"):
            out[k][s] = r[k]
        out["per_job"].append(r)
    return out


def displacement(r):
    """For one claim job's result: (displaced [count] bool: matched to another keypoint than first_choice;
    depth [count]: the length of the chain of points that ends at this one -- 1 for a point that got its first
    choice, 1 + the depth of the earlier point that holds its first choice otherwise)."""
    bi, fc, matched = r["best_idx"], r["first_choice"], r["matched"]
    n = len(bi)
    displaced = (bi >= 0) & (bi != fc)
    depth = np.zeros(n, np.int32)
    for i in range(n):
        if fc[i] < 0:
            continue
        holder = matched[fc[i]]
        depth[i] = 1 if bi[i] == fc[i] else 1 + depth[holder]
    return displaced, depth
