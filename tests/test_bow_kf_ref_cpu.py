"""Pins the restatement tests/bow_kf_ref.py (SearchByBoW(KeyFrame, KeyFrame), loop closing's window merge and the
Sim3Solver constructor's gather) and the scenes of tests/bow_kf_scenes.py on hand-computed values, and asserts that
each scene contains what it is for, so that a scene cannot silently lose its point."""
from __future__ import annotations

import numpy as np
import pytest

import bow_kf_ref as ref
import bow_kf_scenes as sc
import bow_search_ref as frame_ref


@pytest.fixture(scope="module")
def edges():
    a, b, nodes = sc.edge_pair()
    out = {}
    for ori in (False, True):
        st = {}
        n, m = sc.expected_search(ref, a, b, ori, stats=st)
        out[ori] = (n, m, st)
    return a, b, nodes, out


def test_scene_sizes():
    for name, (kf1, kfs2) in sc.search_scenes().items():
        assert len(kfs2) <= 4, name
        for k in [kf1] + kfs2:
            crowd = sum(len(v) for v in k["feat_vec"].values() if len(v) >= 65)
            assert len(k["ok"]) - crowd <= 200, name
    m = sc.merge_scene()
    assert len(m["group"]) - 1 <= 3 and max(np.diff(m["group"])) <= 4


def test_edge_cases_by_hand(edges):
    a, b, nodes, out = edges
    n, m, st = out[False]
    # best distance exactly 50: rejected (strict <), where the Frame form accepts the same pair
    node, i1 = nodes["exact50"]
    assert m[i1] == -1 and st["exact_th"] == 1
    g = b["feat_vec"][node]
    assert [ref.descriptor_distance(a["descriptors"][i1], b["descriptors"][j]) for j in g] == [50, 156]
    fn, fm = frame_ref.search_by_bow(a["descriptors"], a["keys_un"]["angle"], {node: [i1]}, a["ok"], b["descriptors"],
                                     b["keys_un"]["angle"], {node: g}, sc.NNRATIO, False)
    assert fn == 1 and fm[g[0]] == i1
    assert m[nodes["d49"][1]] == b["feat_vec"][11][0]
    # a tie on the best distance: best == second, the ratio test fails on the equal second best ...
    assert m[nodes["tie"][1]] == -1 and st["tie_first"] >= 1 and st["equal_second_fail"] >= 1
    # ... and with a ratio above 1 the first index wins
    st15 = {}
    _, m15 = sc.expected_search(ref, a, b, False, nnratio=1.5, stats=st15)
    assert m15[nodes["tie"][1]] == nodes["tie_first_idx2"] and st15["tie_accepted"] >= 1
    # the nearest candidate already claimed: the next one is taken
    _, i1, g1, g2 = nodes["claimed_best"]
    assert m[i1 - 1] == g1 and m[i1] == g2 and st["claimed_best"] >= 1
    # masks on either side
    _, i1, g2 = nodes["ok2_masked"]
    assert m[i1] == g2 and st["ok2_masked_best"] >= 1
    assert m[nodes["ok1_masked"][1]] == -1 and st["ok1_skipped"] >= 1
    # nodes on one side only; features no node lists
    assert st["only1"] >= 1 and st["only2"] >= 1
    # the crowded nodes: 65+ on either side, bests and claimed bests beyond position 64
    assert st["max_node1"] >= 65 and st["max_node2"] >= 65
    assert st["best_pos_ge64"] >= 3 and st["claimed_best_mem"] >= 2
    assert n == int((m >= 0).sum()) > 40


def test_rotation_check(edges):
    a, b, nodes, out = edges
    (n0, m0, st0), (n1, m1, st1) = out[False], out[True]
    i_rm, i_bl = nodes["rot_removed"][1], nodes["rot_blocked"][1]
    g = b["feat_vec"][20][0]
    # without the check the first feature keeps g; with it the match is removed, the claim is not released
    assert m0[i_rm] == g and m0[i_bl] == -1
    assert m1[i_rm] == -1 and m1[i_bl] == -1
    assert st1["rot_removed"] == 1 and st1["rot_removed_blocks"] == 1 and n1 == n0 - 1
    assert ref.rot_bin(270.0, sc.A2) == 6 and ref.rot_bin(sc.A1, sc.A2) == 0
    assert ref.rot_bin(10.0, 25.0) == 12 and ref.rot_bin(359.0, 0.0) == 12 and ref.rot_bin(14.9, 0.0) == 0


def test_other_scenes_contain_their_cases():
    scenes = sc.search_scenes()
    kf1, kfs2 = scenes["random"]
    tot = dict(claimed_best=0, rot_removed=0, equal_second_fail=0, n=0)
    for k2 in kfs2:
        st = {}
        n, m = sc.expected_search(ref, kf1, k2, True, stats=st)
        assert n == int((m >= 0).sum())
        assert len(set(m[m >= 0].tolist())) == n  # a KF2 feature is claimed once
        tot["n"] += n
        for k in ("claimed_best", "rot_removed", "equal_second_fail"):
            tot[k] += st[k]
    assert tot["n"] >= 40 and tot["claimed_best"] >= 1 and tot["rot_removed"] >= 1, tot
    # an empty FeatureVector on either side, and no usable map point on either side: no match
    a, kfs = scenes["edges_batch"]
    assert kfs[1]["feat_vec"] == {} and not kfs[3]["ok"].any()
    for k2 in (kfs[1], kfs[3]):
        n, m = sc.expected_search(ref, a, k2, True)
        assert n == 0 and (m == -1).all()
    for name in ("empty_fv1", "no_ok1"):
        k1, ks = scenes[name]
        for k2 in ks:
            n, m = sc.expected_search(ref, k1, k2, True)
            assert n == 0 and (m == -1).all(), name


def test_merge_by_hand():
    s = sc.merge_scene()
    exp = sc.expected_problems(ref, s, s["matches12"])
    e0, e1, e2 = exp
    # candidate 0: points 5, 6, 8 (j0), 9, 10 (j1), 11, 12, 13 (j2); 7 is bad; 5 and 8 come a second time
    assert e0["num_bow"] == 8
    assert e0["matched_point"].tolist() == [-1, 5, 9, -1, 8, -1, 10, 11, 12, 13, -1, -1]
    assert e0["matched_pair"].tolist() == [-1, 0, 1, -1, 0, -1, 1, 2, 2, 2, -1, -1]
    assert e0["num_bow"] > int((e0["matched_point"] >= 0).sum())  # the overwrite at k = 2
    # the gather drops k = 7 (ok1), k = 8 (the window keyframe's obs_ok) and k = 9 (KF1's obs_ok)
    assert e0["idx1"].tolist() == [1, 2, 4, 6] and e0["n"] == 4
    # candidate 1: only j0 counts (pair_ok of j1 is 0); candidate 2: nothing
    assert e1["num_bow"] == 2 and e1["matched_point"].tolist()[:7] == [5, -1, -1, -1, -1, -1, 6]
    assert e1["idx1"].tolist() == [0, 6]
    assert e2["num_bow"] == 0 and e2["n"] == 0 and (e2["matched_point"] == -1).all()
    # octaves of at least 3 levels on both sides, max_err = (float)(9.210 * sigma2)
    k1 = s["kf1"]
    o1 = k1["keys_un"]["octave"][e0["idx1"]]
    o2 = [s["kfs2"][j]["keys_un"]["octave"][s["matches12"][j, k]] for k, j in zip(e0["idx1"], e0["matched_pair"][e0["idx1"]])]
    assert len(set(o1.tolist())) >= 3 and len(set(int(o) for o in o2)) >= 3
    assert e0["max_err1"][0] == np.float32(9.210 * float(sc.LEVEL_SIGMA2[o1[0]]))
    assert e0["max_err2"][1] == np.float32(9.210 * float(sc.LEVEL_SIGMA2[o2[1]]))
    # the transform against float64: within the bound the GPU test uses
    T, X = s["Tcw1"].astype(np.float64), s["xyz"][k1["mp_id"][1]].astype(np.float64)
    assert np.all(np.abs(e0["x3dc1"][0] - (T[:, :3] @ X + T[:, 3])) <= e0["bound1"][0])
    # x3dc2 uses the candidate's pose
    X2 = s["xyz"][5].astype(np.float64)
    T2 = s["Tcw2"][0].astype(np.float64)
    assert np.all(np.abs(e0["x3dc2"][0] - (T2[:, :3] @ X2 + T2[:, 3])) <= e0["bound2"][0])


def test_chain_scene_contains_repeats():
    s = sc.chain_scene()
    rows = [sc.expected_search(ref, s["kf1"], k2, True)[1] for k2 in s["kfs2"]]
    exp = sc.expected_problems(ref, s, rows)
    for c, e in enumerate(exp):
        raw = sum(int((rows[p] >= 0).sum()) for p in range(s["group"][c], s["group"][c + 1]))
        assert e["n"] >= 6 and e["num_bow"] <= raw, (c, e["n"], e["num_bow"], raw)
    assert exp[0]["num_bow"] < sum(int((rows[p] >= 0).sum()) for p in (0, 1))  # repeated points were met
    assert any(e["n"] < int((e["matched_point"] >= 0).sum()) for e in exp)      # the gather dropped a slot
