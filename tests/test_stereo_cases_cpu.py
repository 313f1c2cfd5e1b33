"""The built stereo scenes (tests/stereo_cases.py) on the CPU: the oracle (oracle/orb_stereo_oracle.cpp)
equals the Python reference (tests/stereo_ref.py) bit for bit, every prescribed reason code occurs on
exactly the prescribed keypoints, and the tie cases really tie."""
from __future__ import annotations

import numpy as np
import pytest

import stereo_cases as cases
from stereo_ref import REASONS, stereo_ref


def oracle_planes(oracle, image):
    ex = oracle.OracleExtractor(200, 1.2, 8, 20, 7)
    ex(image, (0, 0))
    return [ex.level_padded(l) for l in range(8)], ex.params()


@pytest.fixture(scope="module")
def built(oracle):
    """name -> (group, left planes, right planes, oracle params): one extractor call per side per group."""
    out = {}
    for name, fn in cases.GROUPS.items():
        g = fn()
        pl, p = oracle_planes(oracle, g.left_image)
        pr, _ = oracle_planes(oracle, g.right_image)
        out[name] = (g, pl, pr, p)
    return out


def runs(g):
    """(label, left indices) of the calls a group is run as."""
    if g.subsets:
        return list(g.subsets.items())
    return [("all", np.arange(len(g.kps_l)))]


def check_against_ref(oracle, g, idx, pl, pr, p, label):
    r = stereo_ref(g.kps_l[idx], g.desc_l[idx], g.kps_r, g.desc_r, pl, pr, p["scale"], p["inv_scale"], g.bf, g.b)
    ur, dp, kept = oracle.compute_stereo_matches(g.kps_l[idx], g.desc_l[idx], g.kps_r, g.desc_r, pl, pr, p["scale"],
                                                 p["inv_scale"], g.bf, g.b)
    for k, i in enumerate(idx):
        msg = f"{label}: {g.names[i]} (reference: {r.reasons[k]})"
        assert ur[k].view(np.uint32) == r.u_right[k].view(np.uint32), msg
        assert dp[k].view(np.uint32) == r.depth[k].view(np.uint32), msg
    assert kept == r.kept == int((r.u_right >= 0).sum()), label
    return r


def test_frame_is_the_smallest_accepted(oracle):
    assert cases.geometry_accepts(cases.S, cases.S) and not cases.geometry_accepts(cases.S - 1, cases.S - 1)
    assert cases.S < 480
    planes, p = oracle_planes(oracle, cases.hamming().left_image)
    assert [pl.shape[1] - 38 for pl in planes] == cases.LW
    assert np.array_equal(p["scale"], np.array(cases.SCALE)) and np.array_equal(p["inv_scale"], np.array(cases.INV_SCALE))


@pytest.mark.parametrize("name", list(cases.GROUPS))
def test_group(oracle, built, name):
    g, pl, pr, p = built[name]
    seen = set()
    for label, idx in runs(g):
        r = check_against_ref(oracle, g, idx, pl, pr, p, f"{name}/{label}")
        for k, i in enumerate(idx):
            msg = f"{name}/{label}: {g.names[i]}"
            assert r.reasons[k] in REASONS, msg
            assert r.reasons[k] == g.expected_reasons[i], f"{msg}: {r.reasons[k]}, SADs {r.sads.get(k)}"
            if i in g.expected_idx:
                assert r.best_idx[k] == g.expected_idx[i], msg
            if i in g.expected_offset and i in range(len(g.kps_l)) and k in r.sads:
                assert int(np.argmin(r.sads[k])) - 5 == g.expected_offset[i], f"{msg}: SADs {r.sads[k]}"
            if g.expected_sad and r.sad[k] >= 0:
                assert r.sad[k] == g.expected_sad[i], msg
            seen.add(r.reasons[k])
        if g.subsets:
            assert r.kept == sum(g.expected_reasons[i] == "matched" for i in idx), label
    assert cases.GROUP_REASONS[name] <= seen, (name, cases.GROUP_REASONS[name] - seen)
    assert seen <= set(g.expected_reasons)


def test_every_reason_code_is_covered(built):
    seen = set()
    for g, *_ in built.values():
        seen |= set(g.expected_reasons)
    assert seen == set(REASONS)


def test_hamming_ties_exist(built):
    g, pl, pr, p = built["hamming"]
    r = stereo_ref(g.kps_l, g.desc_l, g.kps_r, g.desc_r, pl, pr, p["scale"], p["inv_scale"], g.bf, g.b)
    assert len(g.ties) == 2
    for i, tied in g.ties.items():
        cand = dict(r.candidates[i])
        best = min(cand.values())
        assert sorted(j for j, d in cand.items() if d == best) == sorted(tied), g.names[i]
        assert r.best_idx[i] == min(tied), g.names[i]
    assert {tuple(j // 64 for j in t) for t in g.ties.values()} == {(0, 0), (0, 1)}  # one chunk / two chunks
    # each gate case holds a closer descriptor that the gate (not the distance) removed
    for i, name in enumerate(g.names):
        if name.startswith("gate_") or name in ("uR_above_maxU", "uR_below_minU"):
            chosen = dict(r.candidates[i])[r.best_idx[i]]
            from stereo_ref import popcount_dist
            closer = [j for j in range(len(g.kps_r)) if popcount_dist(g.desc_l[i], g.desc_r[j]) < chosen]
            assert closer and all(j not in dict(r.candidates[i]) for j in closer), name


def test_window_ties_exist(built):
    g, pl, pr, p = built["window"]
    r = stereo_ref(g.kps_l, g.desc_l, g.kps_r, g.desc_r, pl, pr, p["scale"], p["inv_scale"], g.bf, g.b)
    assert sorted(len(t) for t in g.ties.values()) == [2, 3]
    for i, tied in g.ties.items():
        s = r.sads[i]
        assert [k - 5 for k in range(11) if s[k] == min(s)] == tied, (g.names[i], s)
        assert r.offset[i] == tied[0]


def test_batch_frames(oracle):
    g = cases.batch()
    counts_l, counts_r, cap_l, cap_r = g.counts
    assert cap_l > min(counts_l) and any(n % 4 for n in counts_l) and 0 in counts_l[1:-1] and 0 in counts_r[1:-1]
    kept = []
    for f in range(len(counts_l)):
        assert (len(g.kps_l[f]), len(g.kps_r[f])) == (counts_l[f], counts_r[f])
        pl, p = oracle_planes(oracle, g.left_image[f])
        pr, _ = oracle_planes(oracle, g.right_image[f])
        one = cases.Group(g.left_image[f], g.right_image[f], g.kps_l[f], g.desc_l[f], g.kps_r[f], g.desc_r[f], g.bf,
                          g.b, g.expected_reasons[f], g.names[f], g.expected_idx[f], g.expected_offset[f])
        r = check_against_ref(oracle, one, np.arange(counts_l[f]), pl, pr, p, f"batch/frame{f}")
        assert r.reasons == g.expected_reasons[f], f
        kept.append(r.kept)
    assert kept[1] == kept[2] == 0 and kept[0] == counts_l[0] and kept[3] == counts_l[3]
