"""A plain numpy / Python restatement of ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
(reference src/ORBmatcher.cc:260-494) with ORBmatcher::ComputeThreeMaxima (:2336-2378), single-camera
branch (F.Nleft == -1, mpCamera2 == NULL).  Test infrastructure: the expected values of the GPU tests;
written from the reference source, statement by statement, not from the kernel.

Inputs are flat: descriptors uint8 [n, 32], keypoint angles float32 [n], FeatureVectors as dicts
node id -> list of feature indices (std::map order = ascending node id), point_ok[i] = the keyframe's
map point i is non-NULL and not isBad().
"""
from __future__ import annotations

import numpy as np

TH_LOW = 50        # src/ORBmatcher.cc:37
HISTO_LENGTH = 30  # src/ORBmatcher.cc:38

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def descriptor_distance(a, b) -> int:
    """ORBmatcher::DescriptorDistance (:2384-2404): the number of differing bits of two 32-byte rows."""
    return int(_POP[np.bitwise_xor(a, b)].sum())


def compute_three_maxima(sizes):
    """ComputeThreeMaxima (:2336-2378) on the bins' sizes.  Returns (ind1, ind2, ind3)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3 = s
            ind3 = i
    if max2 < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif max3 < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def search_by_bow(kf_desc, kf_angle, kf_fv: dict, point_ok, f_desc, f_angle, f_fv: dict, nnratio: float,
                  check_orientation: bool, stats: dict | None = None):
    """Returns (nmatches, match int32[F.N]) with match[iF] = the keyframe feature whose map point
    vpMapPointMatches[iF] holds at the end, or -1.  stats (optional) receives `taken`: how many visited
    keyframe features had their smallest-distance frame feature (the first one in node order) already
    assigned, `rot_rejected`: the matches the rotation check removed, and `max_node`: the largest number
    of frame features in a shared node."""
    kf_desc = np.asarray(kf_desc, np.uint8).reshape(-1, 32)
    f_desc = np.asarray(f_desc, np.uint8).reshape(-1, 32)
    kf_angle = np.asarray(kf_angle, np.float32)
    f_angle = np.asarray(f_angle, np.float32)
    n_f = len(f_desc)
    nnratio = np.float32(nnratio)
    match = np.full(n_f, -1, np.int32)           # vpMapPointMatches, as keyframe feature indices (:266)
    assigned = np.zeros(n_f, bool)               # vpMapPointMatches[realIdxF] != NULL during the walk
    nmatches = 0
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    factor = np.float32(1.0) / np.float32(HISTO_LENGTH)  # :281, the upstream factor
    n_taken = max_node = 0
    # :290-465: the walk with lower_bound visits exactly the node ids both maps hold, in ascending order
    for node in sorted(set(kf_fv) & set(f_fv)):
        idx_kf, idx_f = kf_fv[node], f_fv[node]
        max_node = max(max_node, len(idx_f))
        if len(idx_f) == 0:
            continue
        fd = f_desc[np.asarray(idx_f, np.int64)]
        for real_kf in idx_kf:                   # :301
            if point_ok is None or not point_ok[real_kf]:  # :307-313
                continue
            dists = _POP[np.bitwise_xor(fd, kf_desc[real_kf][None, :])].sum(axis=1)
            best1, best_f, best2 = 256, -1, 256  # :317-319
            for i_f, real_f in enumerate(idx_f):  # :325
                if assigned[real_f]:             # :332
                    continue
                dist = int(dists[i_f])
                if dist < best1:                 # :341-351
                    best2 = best1
                    best1 = dist
                    best_f = real_f
                elif dist < best2:
                    best2 = dist
            if stats is not None and assigned[idx_f[int(np.argmin(dists))]]:
                n_taken += 1
            if best1 <= TH_LOW:                  # :385
                if np.float32(best1) < nnratio * np.float32(best2):  # :388
                    match[best_f] = real_kf      # :391
                    assigned[best_f] = True
                    if check_orientation:        # :399-414
                        rot = np.float32(kf_angle[real_kf] - f_angle[best_f])
                        if rot < 0.0:
                            rot = np.float32(rot + np.float32(360.0))
                        x = float(np.float32(rot * factor))  # float product, then C round(): half away from zero
                        b = int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))
                        if b == HISTO_LENGTH:
                            b = 0
                        assert 0 <= b < HISTO_LENGTH
                        rot_hist[b].append(best_f)
                    nmatches += 1
    n_rot = 0
    if check_orientation:                        # :468-491
        ind = compute_three_maxima([len(h) for h in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for j in rot_hist[i]:
                match[j] = -1
                nmatches -= 1
                n_rot += 1
    if stats is not None:
        stats.update(taken=n_taken, rot_rejected=n_rot, max_node=max_node)
    return nmatches, match


def search_by_bow_kf(pKF, F, point_ok, nnratio: float, check_orientation: bool, stats: dict | None = None):
    """The same on two objects with mDescriptors, mvKeysUn (an `angle` field) and mFeatVec (the
    package's KeyFrame)."""
    return search_by_bow(pKF.mDescriptors, pKF.mvKeysUn["angle"], pKF.mFeatVec, point_ok, F.mDescriptors,
                         F.mvKeysUn["angle"], F.mFeatVec, nnratio, check_orientation, stats)
