"""GPU parity of ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (k_bow_match / k_bow_finish, reference
src/ORBmatcher.cc:260-494) against the Python restatement tests/bow_search_ref.py.

Bar: the match array and the match count are equal, exactly, with and without the orientation check --
on a scene whose nodes hold a handful of features (where the greedy walk's taken features and the rotation
check both occur), on FeatureVectors merged into nodes of ~470 and ~1400 features (past the 64 lanes of a
wave and past 256), on the reference's edge cases, batched over keyframes, and on device-resident sides.
"""
from __future__ import annotations

import numpy as np
import pytest

import bow_search_ref as ref
from bow_search_scenes import device_keyframe, merge_nodes, variant

pytestmark = pytest.mark.gpu

NNRATIO = 0.7


@pytest.fixture(scope="module")
def scene(pkg, synth):
    return [pkg.KeyFrame(**k) for k in synth.keyframe_scene(n_kf=3, n_points=300, seed=201, mappoint_frac=0.8,
                                                            clutter=60)]


@pytest.fixture(scope="module")
def expected(scene):
    """The restatement on the base scene: {(frame, check_ori): (n, match, stats)}, computed once."""
    out = {}
    for f in (1, 2):
        for ori in (False, True):
            st = {}
            n, m = ref.search_by_bow_kf(scene[0], scene[f], scene[0].has_mappoint, NNRATIO, ori, st)
            out[f, ori] = (n, m, st)
    return out


@pytest.fixture(scope="module")
def big_scene(pkg, synth):
    return [pkg.KeyFrame(**k) for k in synth.keyframe_scene(n_kf=2, n_points=1500, seed=201, mappoint_frac=0.8,
                                                            clutter=250)]


@pytest.mark.parametrize("check_ori", [False, True])
def test_base_scene_parity(pkg, scene, expected, check_ori):
    matcher = pkg.ORBmatcher(NNRATIO, check_ori)
    for f in (1, 2):
        rn, rm, st = expected[f, check_ori]
        # the case exercises what it is for: a taken best candidate, and (with the check) a rotation reject
        assert st["taken"] >= 1 and rn >= 20
        if check_ori:
            assert st["rot_rejected"] >= 1
        n, m = matcher.SearchByBoW(scene[0], scene[f], scene[0].has_mappoint)
        print(f"frame {f} ori {check_ori}: {n} matches (restatement {rn}), stats {st}")
        assert n == rn, f"count {n} vs restatement {rn}"
        assert m.dtype == np.int32 and m.shape == (scene[f].N,)
        assert np.array_equal(m, rm), f"{int((m != rm).sum())} differing matches"
        # point_ok=None reads the keyframe's has_mappoint
        n2, m2 = matcher.SearchByBoW(scene[0], scene[f])
        assert n2 == rn and np.array_equal(m2, rm)


@pytest.mark.parametrize("remap,min_node", [("mod3", 257), ("single", 1000)])
def test_large_nodes(pkg, big_scene, remap, min_node):
    """Nodes far beyond a wave's 64 lanes and beyond 256 features: node % 3 (~470 frame features per node)
    and a single node holding the whole frame (~1400)."""
    fn = (lambda node: node % 3) if remap == "mod3" else (lambda node: 5)
    kf = variant(pkg, big_scene[0], feat_vec=merge_nodes(big_scene[0].mFeatVec, fn))
    fr = variant(pkg, big_scene[1], feat_vec=merge_nodes(big_scene[1].mFeatVec, fn))
    st = {}
    rn, rm = ref.search_by_bow_kf(kf, fr, kf.has_mappoint, NNRATIO, True, st)
    assert st["max_node"] >= min_node and st["taken"] >= 1 and rn > 100
    n, m = pkg.ORBmatcher(NNRATIO, True).SearchByBoW(kf, fr, kf.has_mappoint)
    print(f"{remap}: {n} matches (restatement {rn}), stats {st}")
    assert n == rn and np.array_equal(m, rm), f"{n} vs {rn}, {int((m != rm).sum())} differing matches"


def test_edge_cases(pkg, scene):
    kf, fr = scene[0], scene[1]
    matcher = pkg.ORBmatcher(NNRATIO, True)
    ok = kf.has_mappoint
    shifted = variant(pkg, fr, feat_vec={node + 1000: idx for node, idx in fr.mFeatVec.items()})
    empty_f = variant(pkg, fr, keys_un=fr.mvKeysUn[:0], descriptors=fr.mDescriptors[:0], u_right=None,
                      has_mappoint=None, feat_vec={})
    empty_k = variant(pkg, kf, keys_un=kf.mvKeysUn[:0], descriptors=kf.mDescriptors[:0], u_right=None,
                      has_mappoint=None, feat_vec={})
    # a keyframe of one descriptor repeated: inside a node every frame feature is at the same distance, so
    # best == second and every ratio test fails (nodes with a single frame feature are left out: there the
    # second distance stays 256)
    multi = {node: idx for node, idx in fr.mFeatVec.items() if len(idx) >= 2}
    same_k = variant(pkg, kf, descriptors=np.repeat(kf.mDescriptors[:1], kf.N, 0))
    same_f = variant(pkg, fr, descriptors=np.repeat(kf.mDescriptors[:1], fr.N, 0), feat_vec=multi)
    cases = [("no shared node", kf, shifted, ok, True), ("empty frame", kf, empty_f, ok, True),
             ("empty keyframe", empty_k, fr, None, True), ("every flag 0", kf, fr, np.zeros(kf.N, np.uint8), True),
             ("duplicate descriptors, both sides", same_k, same_f, ok, True),
             # against the real frame the duplicates compete for the same frame features, one after the other
             ("duplicate descriptors, keyframe", same_k, fr, ok, False)]
    for name, a, b, flags, zero in cases:
        rn, rm = ref.search_by_bow_kf(a, b, flags, NNRATIO, True)
        n, m = matcher.SearchByBoW(a, b, flags)
        assert n == rn and m.shape == (b.N,) and np.array_equal(m, rm), name
        if zero:
            assert n == 0 and (m == -1).all(), name
    # no flags at all (has_mappoint None, point_ok None): no usable map point
    n, m = matcher.SearchByBoW(variant(pkg, kf, has_mappoint=None), fr)
    assert n == 0 and (m == -1).all()


def test_many_equals_single_calls(pkg, scene, expected):
    matcher = pkg.ORBmatcher(NNRATIO, True)
    # two keyframes against one frame: scene[0] with its flags, scene[2] with its own
    kfs, flags = [scene[0], scene[2]], [scene[0].has_mappoint, scene[2].has_mappoint]
    got = matcher.SearchByBoWMany(kfs, scene[1], flags)
    assert len(got) == 2
    for k, ok, (n, m) in zip(kfs, flags, got):
        sn, sm = matcher.SearchByBoW(k, scene[1], ok)
        rn, rm = ref.search_by_bow_kf(k, scene[1], ok, NNRATIO, True)
        assert n == sn == rn > 0 and np.array_equal(m, sm) and np.array_equal(m, rm)
    assert got[0][0] == expected[1, True][0]
    assert matcher.SearchByBoWMany([], scene[1]) == []


def test_device_entry(pkg, scene, expected):
    """DeviceKeyFrames over the same arrays (capacity past the counts, junk beyond): pairs (kf0, frame1),
    (kf0, frame2) through the pair_frame table equal the host entry and the restatement; a keyframe
    flagged ORB_ERR_CAPACITY (a negative FeatureVector size, a count above the capacity) reports it and
    gets no matches."""
    import torch
    cap = 512
    matcher = pkg.ORBmatcher(NNRATIO, True)
    kf = device_keyframe(pkg, scene[0], cap)
    f1, f2 = device_keyframe(pkg, scene[1], cap), device_keyframe(pkg, scene[2], cap - 64)
    bad_nodes = device_keyframe(pkg, scene[0], cap, n_nodes=pkg._lib.ORB_ERR_CAPACITY)
    bad_count = device_keyframe(pkg, scene[0], cap, count=cap + 1)
    ok = torch.from_numpy(np.concatenate([scene[0].has_mappoint, np.ones(cap - scene[0].N, np.uint8)])).cuda()
    m, cnt = matcher.SearchByBoWDevice([kf, kf, bad_nodes, bad_count, kf], [f1, f2], [ok, None, ok, ok, ok],
                                       pair_frame=[0, 1, 0, 1, 1])
    assert m.is_cuda and m.dtype == torch.int32 and tuple(m.shape) == (5, cap) and tuple(cnt.shape) == (5,)
    m, cnt = m.cpu().numpy(), cnt.cpu().numpy()
    for p, f in ((0, 1), (1, 2), (4, 2)):
        rn, rm, _ = expected[f, True]
        hn, hm = matcher.SearchByBoW(scene[0], scene[f], scene[0].has_mappoint)
        assert cnt[p] == rn == hn
        assert np.array_equal(m[p, :scene[f].N], rm) and np.array_equal(hm, rm)
        assert (m[p, scene[f].N:] == -1).all()
    for p in (2, 3):
        assert cnt[p] == pkg._lib.ORB_ERR_CAPACITY and (m[p] == -1).all()
    # a flagged frame side, and the default pair table (every pair against frames[0])
    bad_frame = device_keyframe(pkg, scene[1], cap, count=-3)
    m, cnt = matcher.SearchByBoWDevice([kf], bad_frame, [ok])
    assert int(cnt[0]) == pkg._lib.ORB_ERR_CAPACITY and bool((m == -1).all())
    m, cnt = matcher.SearchByBoWDevice([kf], f1)
    assert int(cnt[0]) == expected[1, True][0]
    assert np.array_equal(m[0, :scene[1].N].cpu().numpy(), expected[1, True][1])


def test_invalid_views_rejected(pkg, scene):
    kf, fr = scene[0], scene[1]
    matcher = pkg.ORBmatcher(NNRATIO, False)
    for side in ("keyframe", "frame"):
        base = kf if side == "keyframe" else fr
        fv = base.mFeatVec
        first = next(iter(fv))
        dup = dict(fv)
        dup[first] = list(fv[first]) + [fv[first][0]]  # a feature listed twice
        beyond = dict(fv)
        beyond[first] = [base.N] + list(fv[first])[1:]  # an index >= n
        for bad_fv in (dup, beyond):
            bad = variant(pkg, base, feat_vec=bad_fv)
            with pytest.raises(pkg.OrbGpuError) as e:
                matcher.SearchByBoW(bad if side == "keyframe" else kf, bad if side == "frame" else fr, kf.has_mappoint)
            assert e.value.code == pkg._lib.ORB_ERR_ARG
    with pytest.raises(ValueError):
        matcher.SearchByBoWMany([kf], fr, [kf.has_mappoint[:-1]])
