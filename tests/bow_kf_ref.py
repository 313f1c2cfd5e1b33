"""A plain sequential numpy / Python restatement of loop closing's BoW head, written from the reference source
statement by statement, not from the kernels.  Test infrastructure: the expected values of the GPU tests.

  search_by_bow_kf   ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (src/ORBmatcher.cc:893-1044),
                     single camera (NLeft == -1)
  merge              the window merge of LoopClosing::DetectCommonRegionsFromBoW (src/LoopClosing.cc:855-881)
  gather             the Sim3Solver constructor's loop (src/Sim3Solver.cc:71-118), float32 without contraction

Inputs are flat: descriptors uint8 [n, 32], keypoint angles float32 [n], FeatureVectors as dicts node id -> list of
feature indices (std::map order = ascending node id), ok[i] = the keyframe's map point i is non-NULL and not
isBad(), map points as indices into a pool (-1: NULL).
"""
from __future__ import annotations

import numpy as np

from bow_search_ref import HISTO_LENGTH, TH_LOW, compute_three_maxima, descriptor_distance

f32 = np.float32


def rot_bin(a1, a2) -> int:
    """:995-1000 with factor = 1.0f / HISTO_LENGTH (:917); C round(): half away from zero."""
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    x = float(f32(rot * (f32(1.0) / f32(HISTO_LENGTH))))
    b = int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))
    return 0 if b == HISTO_LENGTH else b


def search_by_bow_kf(desc1, angle1, fv1: dict, ok1, desc2, angle2, fv2: dict, ok2, nnratio: float,
                     check_orientation: bool, stats: dict | None = None):
    """Returns (nmatches, matches12 int32[N1]) with matches12[idx1] = the feature of KF2 whose map point
    vpMatches12[idx1] holds at the end, or -1.  ok1 / ok2 None: no usable map point on that side.
    stats (optional) receives what the walk met; tests assert on it that a scene contains what it is for."""
    desc1 = np.asarray(desc1, np.uint8).reshape(-1, 32)
    desc2 = np.asarray(desc2, np.uint8).reshape(-1, 32)
    n1, n2 = len(desc1), len(desc2)
    nnratio = f32(nnratio)
    matches12 = np.full(n1, -1, np.int32)        # vpMatches12 as KF2 feature indices (:907)
    matched2 = np.zeros(n2, bool)                # vbMatched2 (:908)
    claimer = {}                                 # idx2 -> idx1 (for stats only)
    blocked = []                                 # (idx1, idx2, dist): idx1's smallest-distance usable candidate was claimed
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    st = dict(exact_th=0, tie_first=0, tie_accepted=0, equal_second_fail=0, claimed_best=0, claimed_best_mem=0,
              ok2_masked_best=0, ok1_skipped=0, max_node1=0, max_node2=0, best_pos_ge64=0, rot_removed=0,
              rot_removed_blocks=0, only1=len(set(fv1) - set(fv2)), only2=len(set(fv2) - set(fv1)))
    for node in sorted(set(fv1) & set(fv2)):     # :926-1020: the node ids both maps hold, ascending
        idx_1, idx_2 = list(fv1[node]), list(fv2[node])
        st["max_node1"] = max(st["max_node1"], len(idx_1))
        st["max_node2"] = max(st["max_node2"], len(idx_2))
        for idx1 in idx_1:                       # :932
            if ok1 is None or not ok1[idx1]:     # :939-943
                st["ok1_skipped"] += 1
                continue
            best1, best_idx2, best2 = 256, -1, 256  # :947-949
            best_pos = -1
            all_d = []
            for pos, idx2 in enumerate(idx_2):   # :952
                dist = descriptor_distance(desc1[idx1], desc2[idx2])
                usable = ok2 is not None and bool(ok2[idx2])
                all_d.append((dist, pos, idx2, usable))
                if matched2[idx2] or not usable:  # :963-967
                    continue
                if dist < best1:                 # :973-982
                    best2 = best1
                    best1 = dist
                    best_idx2 = idx2
                    best_pos = pos
                elif dist < best2:
                    best2 = dist
            if all_d:
                d_min, pos_min, i_min, usable_min = min(all_d)[:4]
                if not usable_min:
                    st["ok2_masked_best"] += 1
                usable_d = [a for a in all_d if a[3]]
                if usable_d and matched2[min(usable_d)[2]]:
                    st["claimed_best"] += 1
                    st["claimed_best_mem"] += min(usable_d)[1] >= 64
                    blocked.append((idx1, min(usable_d)[2], min(usable_d)[0]))
            if best1 < 256 and best1 == best2:
                st["tie_first"] += 1
                if best1 < TH_LOW:
                    st["equal_second_fail" if not f32(best1) < nnratio * f32(best2) else "tie_accepted"] += 1
            st["exact_th"] += best1 == TH_LOW and bool(f32(best1) < nnratio * f32(best2))
            if best1 < TH_LOW:                   # :986
                if f32(best1) < nnratio * f32(best2):  # :988
                    matches12[idx1] = best_idx2  # :990
                    matched2[best_idx2] = True   # :991
                    claimer[best_idx2] = idx1
                    st["best_pos_ge64"] += best_pos >= 64
                    if check_orientation:        # :993-1003
                        b = rot_bin(angle1[idx1], angle2[best_idx2])
                        assert 0 <= b < HISTO_LENGTH
                        rot_hist[b].append(idx1)
                    nmatches += 1
    removed = set()
    if check_orientation:                        # :1023-1041
        ind = compute_three_maxima([len(h) for h in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for idx1 in rot_hist[i]:
                matches12[idx1] = -1
                nmatches -= 1
                removed.add(idx1)
    st["rot_removed"] = len(removed)
    # a claim the rotation check emptied, which a later KF1 feature would have taken (distance below TH_LOW)
    st["rot_removed_blocks"] = sum(1 for _, idx2, d in blocked if claimer.get(idx2) in removed and d < TH_LOW)
    if stats is not None:
        stats.update(st)
    return nmatches, matches12


def merge(matches12_rows, mp_id2_rows, bad, pair_ok, n1: int):
    """:855-881 for one candidate.  matches12_rows[j][k]: the feature of window keyframe j matched to KF1's feature
    k or -1 (vvpMatchedMPs[j][k] = mvpMapPoints2[that]); mp_id2_rows[j]: the window keyframe's map points.  A pair
    with pair_ok[j] == 0 was skipped at :842, its vvpMatchedMPs[j] is empty.  Returns (num_bow, matched_point
    int32[n1], matched_pair int32[n1])."""
    seen = set()                                 # spMatchedMPi
    num_bow = 0
    matched_point = np.full(n1, -1, np.int32)    # vpMatchedPoints
    matched_pair = np.full(n1, -1, np.int32)     # vpKeyFrameMatchedMP, as j
    for j in range(len(matches12_rows)):         # :855
        if pair_ok is not None and not pair_ok[j]:
            continue
        for k in range(n1):                      # :859
            idx2 = int(matches12_rows[j][k])
            mp = int(mp_id2_rows[j][idx2]) if idx2 >= 0 else -1
            if mp < 0 or (bad is not None and bad[mp]):  # :864
                continue
            if mp not in seen:                   # :868
                seen.add(mp)
                num_bow += 1
                matched_point[k] = mp
                matched_pair[k] = j
    return num_bow, matched_point, matched_pair


def transform(T, X):
    """R X + t in float32, products and sums rounded one by one (no contraction), left to right."""
    T = np.asarray(T, f32).reshape(3, 4)
    X = np.asarray(X, f32)
    out = np.empty(3, f32)
    for r in range(3):
        out[r] = f32(f32(f32(f32(T[r, 0] * X[0]) + f32(T[r, 1] * X[1])) + f32(T[r, 2] * X[2])) + T[r, 3])
    return out


def transform_bound(T, X):
    """4 * 2^-24 * (|r0 x| + |r1 y| + |r2 z| + |t|) per component: covers any contraction of the three
    products and three sums."""
    T = np.abs(np.asarray(T, np.float64).reshape(3, 4))
    X = np.abs(np.asarray(X, np.float64))
    return 4.0 * 2.0 ** -24 * (T[:, 0] * X[0] + T[:, 1] * X[1] + T[:, 2] * X[2] + T[:, 3])


def gather(matched_point, matched_pair, matches12_rows, mp_id1, ok1, bad, xyz, octave1, sigma2_1, octave2_rows,
           sigma2_2_rows, Tcw1, Tcw2, obs_ok1=None, obs_ok2_rows=None):
    """Sim3Solver.cc:71-118 for one candidate, with indexKF1 = i1 and indexKF2 = the matched feature of the window
    keyframe matched_pair[i1] (the map's invariant), obs_ok standing for GetIndexInKeyFrame >= 0.  Returns a dict:
    n, idx1 [n], x3dc1 / x3dc2 [n, 3], max_err1 / max_err2 [n], bound1 / bound2 [n, 3]."""
    idx1, x1, x2, e1, e2, b1, b2 = [], [], [], [], [], [], []
    for i1 in range(len(matched_point)):         # :71
        mp2 = int(matched_point[i1])
        if mp2 < 0:                              # :73
            continue
        if not ok1[i1]:                          # :78-82, pMP1
            continue
        if bad is not None and bad[mp2]:         # :81, pMP2
            continue
        j = int(matched_pair[i1])                # :85
        idx2 = int(matches12_rows[j][i1])        # :88
        if obs_ok1 is not None and not obs_ok1[i1]:  # :90
            continue
        if obs_ok2_rows is not None and obs_ok2_rows[j] is not None and not obs_ok2_rows[j][idx2]:
            continue
        s1 = f32(sigma2_1[int(octave1[i1])])     # :93-97
        s2 = f32(sigma2_2_rows[j][int(octave2_rows[j][idx2])])
        e1.append(f32(9.210 * float(s1)))        # :99-100
        e2.append(f32(9.210 * float(s2)))
        idx1.append(i1)                          # :104
        X1, X2 = xyz[int(mp_id1[i1])], xyz[mp2]
        x1.append(transform(Tcw1, X1))           # :106-110
        x2.append(transform(Tcw2, X2))
        b1.append(transform_bound(Tcw1, X1))
        b2.append(transform_bound(Tcw2, X2))
    n = len(idx1)
    arr = lambda a, w: np.asarray(a, f32).reshape(n, w) if w else np.asarray(a, f32).reshape(n)  # noqa: E731
    return dict(n=n, idx1=np.asarray(idx1, np.int32), x3dc1=arr(x1, 3), x3dc2=arr(x2, 3), max_err1=arr(e1, 0),
                max_err2=arr(e2, 0), bound1=np.asarray(b1, np.float64).reshape(n, 3),
                bound2=np.asarray(b2, np.float64).reshape(n, 3))
