"""Pins tests/bow_search_ref.py, the Python restatement of ORBmatcher::SearchByBoW (reference
src/ORBmatcher.cc:260-494) the GPU tests compare against, on hand-built cases whose expected values are
worked out below from the reference's statements."""
from __future__ import annotations

import numpy as np

import bow_search_ref as ref


def _desc(*bit_counts):
    """Descriptors with the given numbers of leading one bits: the distance of two of them is the
    difference of their counts."""
    out = np.zeros((len(bit_counts), 32), np.uint8)
    for i, n in enumerate(bit_counts):
        bits = np.zeros(256, np.uint8)
        bits[:n] = 1
        out[i] = np.packbits(bits)
    return out


def test_descriptor_distance_and_three_maxima():
    d = _desc(0, 7, 256)
    assert ref.descriptor_distance(d[0], d[1]) == 7 and ref.descriptor_distance(d[1], d[2]) == 249
    # 10, 9 and 1 of 30 bins: the third is below 0.1 * max1 and is dropped; a lone bin keeps only itself
    sizes = [0] * 30
    sizes[3], sizes[7], sizes[20] = 9, 10, 0
    assert ref.compute_three_maxima(sizes) == (7, 3, -1)
    sizes[20] = 1
    assert ref.compute_three_maxima(sizes) == (7, 3, 20)
    sizes[3], sizes[20] = 0, 0
    assert ref.compute_three_maxima(sizes) == (7, -1, -1)


def test_duplicate_descriptor_tie():
    """Two frame features with the same descriptor in one node: the first in node order is the best, the
    later equal distance becomes bestDist2 (`else if(dist<bestDist2)`), and 10 < 0.7 * 10 fails, so the
    keyframe feature is not matched.  A second keyframe feature in another node whose candidates are at
    distances 5 and 40 is matched to the first: 5 < 0.7 * 40."""
    kf_desc = _desc(0, 100)
    f_desc = _desc(10, 10, 105, 140, 200)
    kf_fv = {11: [0], 12: [1], 13: []}
    f_fv = {11: [1, 0], 12: [3, 2], 14: [4]}  # node 13 / 14: not shared
    zero = np.zeros(5, np.float32)
    stats = {}
    n, m = ref.search_by_bow(kf_desc, zero[:2], kf_fv, np.ones(2, np.uint8), f_desc, zero, f_fv, 0.7, False, stats)
    assert n == 1 and m.tolist() == [-1, -1, 1, -1, -1]
    assert stats == dict(taken=0, rot_rejected=0, max_node=2)
    # with a permissive ratio the tie goes to the first index in node order: frame feature 1
    n, m = ref.search_by_bow(kf_desc, zero[:2], kf_fv, np.ones(2, np.uint8), f_desc, zero, f_fv, 1.01, False)
    assert n == 2 and m.tolist() == [-1, 0, 1, -1, -1]
    # an unusable map point is not visited
    n, m = ref.search_by_bow(kf_desc, zero[:2], kf_fv, np.array([1, 0], np.uint8), f_desc, zero, f_fv, 1.01, False)
    assert n == 1 and m.tolist() == [-1, 0, -1, -1, -1]


def test_best_already_taken_falls_to_second_choice():
    """One node; keyframe features A (20 bits) then B (22 bits); frame features at 21, 60 and 120 bits.
    A: distances 1, 40, 100 -> best 1, second 40, accepted (1 < 28), takes frame feature 0.
    B: its true best (distance 1, frame feature 0) is taken; of the rest: 38 and 98 -> best 38 <= 50 and
    38 < 0.7 * 98 = 68.6, so B falls to frame feature 1.
    Rotation: A's angle difference is 10 - 350 + 360 = 20 -> round(20 / 30) = 1; B's is 200 - 20 = 180 ->
    round(6.0) = 6.  Bins 1 and 6 hold one match each: both are kept (max2 = 1 >= 0.1 * 1).  With a third
    keyframe feature C (125 bits, angle 0 against 100 -> 260 / 30 = 8.67 -> bin 9) all three bins are maxima."""
    kf_desc = _desc(20, 22, 125)
    f_desc = _desc(21, 60, 120)
    kf_angle = np.array([10, 200, 0], np.float32)
    f_angle = np.array([350, 20, 100], np.float32)
    ok = np.ones(3, np.uint8)
    stats = {}
    n, m = ref.search_by_bow(kf_desc, kf_angle, {5: [0, 1]}, ok, f_desc, f_angle, {5: [0, 1, 2]}, 0.7, True, stats)
    assert n == 2 and m.tolist() == [0, 1, -1]
    assert stats == dict(taken=1, rot_rejected=0, max_node=3)
    n, m = ref.search_by_bow(kf_desc, kf_angle, {5: [0, 1, 2]}, ok, f_desc, f_angle, {5: [0, 1, 2]}, 0.7, True, stats)
    assert n == 3 and m.tolist() == [0, 1, 2] and stats["taken"] == 1
    # in the other stored order B comes first and takes frame feature 0 (distance 1); A then finds 40 and 100
    n, m = ref.search_by_bow(kf_desc, kf_angle, {5: [1, 0]}, ok, f_desc, f_angle, {5: [0, 1, 2]}, 0.7, False, stats)
    assert n == 2 and m.tolist() == [1, 0, -1] and stats["taken"] == 1


def test_rotation_check_rejects_minor_bins():
    """Twelve matches in bin 0, one in bin 6: 1 < 0.1 * 12 drops the second maximum, and the lone match is
    reset to -1 and uncounted."""
    n = 13
    kf_desc = _desc(*[16 * i for i in range(n)])
    f_desc = kf_desc.copy()
    kf_angle = np.zeros(n, np.float32)
    kf_angle[4] = 180
    fv = {100 + i: [i] for i in range(n)}
    stats = {}
    cnt, m = ref.search_by_bow(kf_desc, kf_angle, fv, np.ones(n, np.uint8), f_desc, np.zeros(n, np.float32), fv, 0.7,
                               True, stats)
    exp = list(range(n))
    exp[4] = -1
    assert cnt == 12 and m.tolist() == exp and stats["rot_rejected"] == 1
