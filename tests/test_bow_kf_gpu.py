"""GPU parity of ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) (k_bowkf_match / k_bowkf_finish, reference
src/ORBmatcher.cc:893-1044) and of loop closing's merge + Sim3 problem gather (k_lb_*, src/LoopClosing.cc:855-881,
src/Sim3Solver.cc:71-118) against the sequential restatement tests/bow_kf_ref.py on the scenes of
tests/bow_kf_scenes.py (tests/test_bow_kf_ref_cpu.py asserts what each scene contains).

Bar: every integer output equal; max_err bit-equal; x3dc within 4 * 2^-24 * (|r0 x| + |r1 y| + |r2 z| + |t|) per
component of the uncontracted float32 restatement (any contraction of the three products and three sums); through
the host entry and the device entry, batched and one by one, twice for the same bits.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import bow_kf_ref as ref
import bow_kf_scenes as sc
from bow_search_scenes import device_keyframe

pytestmark = pytest.mark.gpu

INT_KEYS = ("matched_point", "matched_pair", "num_bow", "n", "idx1")
ALL_KEYS = INT_KEYS + ("x3dc1", "x3dc2", "max_err1", "max_err2")


@pytest.fixture(scope="module")
def scenes():
    return sc.search_scenes()


@pytest.fixture(scope="module")
def expected(scenes):
    """The restatement on every pair of every scene, once: {(scene, check_ori, nnratio): [(n, matches12)]}."""
    out = {}
    for name, (kf1, kfs2) in scenes.items():
        for ori in (False, True):
            out[name, ori, sc.NNRATIO] = [sc.expected_search(ref, kf1, k2, ori) for k2 in kfs2]
    a, kfs2 = scenes["edges"]
    out["edges", False, 1.5] = [sc.expected_search(ref, a, k2, False, nnratio=1.5) for k2 in kfs2]
    return out


def _check_rows(got, exp, what):
    assert len(got) == len(exp)
    for p, ((n, m), (rn, rm)) in enumerate(zip(got, exp)):
        assert n == rn, f"{what} pair {p}: count {n} vs restatement {rn}"
        assert np.array_equal(m, rm), f"{what} pair {p}: {int((m != rm).sum())} differing matches"


@pytest.mark.parametrize("check_ori", [False, True])
def test_search_host_entry(pkg, scenes, expected, check_ori):
    matcher = pkg.ORBmatcher(sc.NNRATIO, check_ori)
    for name, (kf1, kfs2) in scenes.items():
        K1, K2 = sc.keyframe(pkg, kf1), [sc.keyframe(pkg, k) for k in kfs2]
        got = matcher.SearchByBoWKFMany(K1, K2, kf1["ok"], [k["ok"] for k in kfs2])
        assert all(m.dtype == np.int32 and m.shape == (K1.N,) for _, m in got)
        _check_rows(got, expected[name, check_ori, sc.NNRATIO], f"{name} batched")
        # the same pairs one by one, the masks read from has_mappoint; and a second batched call: the same bits
        _check_rows([matcher.SearchByBoWKF(K1, k) for k in K2], expected[name, check_ori, sc.NNRATIO], f"{name} single")
        again = matcher.SearchByBoWKFMany(K1, K2)
        assert all(a[0] == g[0] and np.array_equal(a[1], g[1]) for a, g in zip(again, got))
    assert matcher.SearchByBoWKFMany(sc.keyframe(pkg, scenes["edges"][0]), []) == []


def test_ratio_above_one_takes_first_index(pkg, scenes, expected):
    kf1, kfs2 = scenes["edges"]
    got = pkg.ORBmatcher(1.5, False).SearchByBoWKFMany(sc.keyframe(pkg, kf1), [sc.keyframe(pkg, k) for k in kfs2])
    _check_rows(got, expected["edges", False, 1.5], "nnratio 1.5")


def test_no_masks_no_matches(pkg, scenes):
    kf1, kfs2 = scenes["random"]
    K1, K2 = sc.keyframe(pkg, kf1), sc.keyframe(pkg, kfs2[0])
    K2.has_mappoint, K2._view = None, None
    n, m = pkg.ORBmatcher(sc.NNRATIO, True).SearchByBoWKF(K1, K2)
    assert n == 0 and (m == -1).all()


@pytest.mark.parametrize("check_ori", [False, True])
def test_search_device_entry(pkg, scenes, expected, check_ori):
    """DeviceKeyFrames over the same arrays (capacity past the counts, junk beyond); every scene in one call
    through the pair_kf1 table; masks as has_mappoint and as explicit tensors; twice for the same bits."""
    import torch
    matcher = pkg.ORBmatcher(sc.NNRATIO, check_ori)
    kf1s, kfs2, pair_kf1, exp, n1s = [], [], [], [], []
    for i, (name, (kf1, ks)) in enumerate(scenes.items()):
        kf1s.append(device_keyframe(pkg, sc.keyframe(pkg, kf1), 384 + 64 * (i % 2)))
        for k, e in zip(ks, expected[name, check_ori, sc.NNRATIO]):
            kfs2.append(device_keyframe(pkg, sc.keyframe(pkg, k), 320 + 32 * (len(kfs2) % 3)))
            pair_kf1.append(i)
            exp.append(e)
            n1s.append(len(kf1["ok"]))
    m, cnt = matcher.SearchByBoWKFDevice(kf1s, kfs2, pair_kf1)
    C = max(k.cap for k in kf1s)
    assert m.is_cuda and m.dtype == torch.int32 and tuple(m.shape) == (len(kfs2), C) and tuple(cnt.shape) == (len(kfs2),)
    mh, ch = m.cpu().numpy(), cnt.cpu().numpy()
    for p, ((rn, rm), n1) in enumerate(zip(exp, n1s)):
        assert ch[p] == rn, f"pair {p}: {ch[p]} vs {rn}"
        assert np.array_equal(mh[p, :n1], rm) and (mh[p, n1:] == -1).all(), f"pair {p}"
    m2, cnt2 = matcher.SearchByBoWKFDevice(kf1s, kfs2, pair_kf1)
    assert torch.equal(m, m2) and torch.equal(cnt, cnt2)
    # the same pairs as single-pair device calls: the batched rows, bit for bit
    for p in range(len(kfs2)):
        m1, c1 = matcher.SearchByBoWKFDevice(kf1s[pair_kf1[p]], [kfs2[p]])
        assert int(c1[0]) == int(cnt[p]) and torch.equal(m1[0], m[p, :m1.shape[1]]) and bool((m[p, m1.shape[1]:] == -1).all()), p
    # explicit mask tensors override has_mappoint: all-zero ok2 for pair 0
    zero = torch.zeros(kfs2[0].cap, dtype=torch.uint8, device="cuda")
    m3, cnt3 = matcher.SearchByBoWKFDevice(kf1s, kfs2, pair_kf1, ok2=[zero] + [None] * (len(kfs2) - 1))
    assert int(cnt3[0]) == 0 and bool((m3[0] == -1).all()) and torch.equal(m3[1:], m[1:])


def test_flagged_side_reports_capacity(pkg, scenes, expected):
    kf1, ks = scenes["random"]
    K1, K2 = sc.keyframe(pkg, kf1), [sc.keyframe(pkg, k) for k in ks]
    cap = 256
    good1, good2 = device_keyframe(pkg, K1, cap), [device_keyframe(pkg, k, cap) for k in K2]
    bad1 = device_keyframe(pkg, K1, cap, count=cap + 1)
    bad2 = device_keyframe(pkg, K2[1], cap, n_nodes=pkg._lib.ORB_ERR_CAPACITY)
    bad3 = device_keyframe(pkg, K2[2], cap, count=-3)
    m, cnt = pkg.ORBmatcher(sc.NNRATIO, True).SearchByBoWKFDevice([good1, bad1], [good2[0], bad2, good2[2], good2[0], bad3],
                                                                  [0, 0, 0, 1, 0])
    m, cnt = m.cpu().numpy(), cnt.cpu().numpy()
    exp = expected["random", True, sc.NNRATIO]
    for p, e in ((0, 0), (2, 2)):
        assert cnt[p] == exp[e][0] and np.array_equal(m[p, :K1.N], exp[e][1])
    for p in (1, 3, 4):
        assert cnt[p] == pkg._lib.ORB_ERR_CAPACITY and (m[p] == -1).all()


def test_search_argument_checks(pkg, scenes):
    import torch
    lib = pkg._lib.load()
    kf1, ks = scenes["random"]
    K1, K2 = sc.keyframe(pkg, kf1), sc.keyframe(pkg, ks[0])
    matcher = pkg.ORBmatcher(sc.NNRATIO, True)
    dup = dict(kf1["feat_vec"])
    first = next(iter(dup))
    dup[first] = list(dup[first]) + [dup[first][0]]
    for a, b in ((sc.keyframe(pkg, sc.variant(kf1, feat_vec=dup)), K2), (K2, sc.keyframe(pkg, sc.variant(kf1, feat_vec=dup)))):
        with pytest.raises(pkg.OrbGpuError) as e:
            matcher.SearchByBoWKF(a, b)
        assert e.value.code == pkg._lib.ORB_ERR_ARG
    with pytest.raises(ValueError):
        matcher.SearchByBoWKFMany(K1, [K2], kf1["ok"][:-1])
    # the raw entries: bad arguments return ORB_ERR_ARG and write nothing
    h = matcher._handle()
    m = np.full(K1.N, 77, np.int32)
    cnt = np.full(1, 77, np.int32)
    v1, v2 = K1.view(), K2.view()
    args = [h, ctypes.byref(v1), None, ctypes.byref(v2), None, 1, m.ctypes.data, cnt.ctypes.data]
    for i, bad in ((0, None), (1, None), (3, None), (5, -1), (5, 65536), (6, None), (7, None)):
        a = list(args)
        a[i] = bad
        assert lib.orb_search_by_bow_kf(*a) == pkg._lib.ORB_ERR_ARG, i
    assert (m == 77).all() and (cnt == 77).all()
    d1, d2 = device_keyframe(pkg, K1, 256), device_keyframe(pkg, K2, 256)
    dm = torch.full((1, 256), 77, dtype=torch.int32, device="cuda")
    dc = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    pk = (ctypes.c_int32 * 1)(3)
    bad_view = type(d2.view())()
    ctypes.memmove(ctypes.byref(bad_view), ctypes.byref(d2.view()), ctypes.sizeof(bad_view))
    bad_view.cap = 0
    base = [h, ctypes.byref(d1.view()), 1, None, ctypes.byref(d2.view()), None, None, 1, dm.data_ptr(), dc.data_ptr(), None]
    for i, bad in ((0, None), (1, None), (2, 0), (4, None), (4, ctypes.byref(bad_view)), (6, pk), (7, -1), (8, None),
                   (9, None)):
        a = list(base)
        a[i] = bad
        assert lib.orb_search_by_bow_kf_device(*a) == pkg._lib.ORB_ERR_ARG, i
    torch.cuda.synchronize()
    assert bool((dm == 77).all()) and bool((dc == 77).all())


# ---- the merge and the gather ----------------------------------------------------------------------------

def _host_kf(pkg, side):
    return pkg.LoopBowKeyFrame(side["mp_id"], side["keys_un"], side["level_sigma2"], side["obs_ok"])


def _run_host(pkg, matcher, s, m12, ok1="scene"):
    ok1 = s["kf1"]["ok"] if isinstance(ok1, str) else ok1
    return pkg.loop_bow_problems(matcher, _host_kf(pkg, s["kf1"]), s["Tcw1"], [_host_kf(pkg, k) for k in s["kfs2"]],
                                 s["group"], s["Tcw2"], s["xyz"], m12, ok1=ok1, bad=s["bad"], pair_ok=s["pair_ok"])


def _device_kf(pkg, side, cap, seed):
    """The side's arrays at capacity `cap` with junk past the count that must not be read."""
    import torch
    rng = np.random.default_rng(seed)
    n = len(side["ok"])
    k = np.zeros(cap, sc.KEYPOINT_DTYPE)
    k[:n] = side["keys_un"]
    k["octave"][n:] = 99
    mp = np.concatenate([side["mp_id"], rng.integers(0, 20, cap - n).astype(np.int32)])
    obs = np.concatenate([side["obs_ok"], np.ones(cap - n, np.uint8)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return pkg.LoopBowKeyFrame(up(mp), up(k.view(np.float32).reshape(cap, 7)), side["level_sigma2"], up(obs))


def _run_device(pkg, matcher, s, m12, cap=64, ok1="scene"):
    import torch
    n1 = len(s["kf1"]["ok"])
    rows = np.full((len(s["kfs2"]), cap), -1, np.int32)
    rows[:, :n1] = np.asarray(m12)[:, :n1]
    ok1 = s["kf1"]["ok"] if isinstance(ok1, str) else ok1
    if ok1 is not None:
        ok1 = torch.from_numpy(np.concatenate([ok1, np.ones(cap - n1, np.uint8)])).cuda()
    res = pkg.loop_bow_problems(matcher, _device_kf(pkg, s["kf1"], cap, 1), s["Tcw1"],
                                [_device_kf(pkg, k, len(k["ok"]) + 5 + p, 2 + p) for p, k in enumerate(s["kfs2"])],
                                s["group"], s["Tcw2"], torch.from_numpy(s["xyz"]).cuda(), torch.from_numpy(rows).cuda(),
                                ok1=ok1, bad=torch.from_numpy(s["bad"]).cuda(), pair_ok=s["pair_ok"])
    assert all(v.is_cuda for v in res.values())
    return res


def _check_problems(res, exp, n1, what):
    res = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}
    for c, e in enumerate(exp):
        n = e["n"]
        print(f"{what} candidate {c}: num_bow {res['num_bow'][c]} ({e['num_bow']}), n {res['n'][c]} ({n})")
        assert res["num_bow"][c] == e["num_bow"] and res["n"][c] == n, (what, c)
        assert np.array_equal(res["matched_point"][c, :n1], e["matched_point"]), (what, c)
        assert np.array_equal(res["matched_pair"][c, :n1], e["matched_pair"]), (what, c)
        assert (res["matched_point"][c, n1:] == -1).all() and (res["matched_pair"][c, n1:] == -1).all()
        assert np.array_equal(res["idx1"][c, :n], e["idx1"]) and (res["idx1"][c, n:] == -1).all(), (what, c)
        for k in ("max_err1", "max_err2"):
            assert np.array_equal(res[k][c, :n].view(np.uint32), e[k].view(np.uint32)), (what, c, k)
        for k, b in (("x3dc1", "bound1"), ("x3dc2", "bound2")):
            err = np.abs(res[k][c, :n].astype(np.float64) - e[k].astype(np.float64))
            if n:
                print(f"  {k}: max error / bound {float((err / e[b]).max()):.3f}")
            assert np.all(err <= e[b]), (what, c, k)


def _same_bits(a, b):
    import torch
    for k in ALL_KEYS:
        x, y = a[k], b[k]
        same = torch.equal(x, y) if hasattr(x, "is_cuda") else np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert same, k


@pytest.fixture(scope="module")
def merge_case():
    s = sc.merge_scene()
    return s, sc.expected_problems(ref, s, s["matches12"])


@pytest.fixture(scope="module")
def chain_case():
    s = sc.chain_scene()
    rows = np.stack([sc.expected_search(ref, s["kf1"], k2, True)[1] for k2 in s["kfs2"]])
    return s, rows, sc.expected_problems(ref, s, rows)


def test_problems_hand_scene(pkg, merge_case):
    import torch
    s, exp = merge_case
    matcher = pkg.ORBmatcher(sc.NNRATIO, True)
    n1 = len(s["kf1"]["ok"])
    host = _run_host(pkg, matcher, s, s["matches12"])
    _check_problems(host, exp, n1, "host")
    _same_bits(host, _run_host(pkg, matcher, s, s["matches12"]))
    dev = _run_device(pkg, matcher, s, s["matches12"])
    _check_problems(dev, exp, n1, "device")
    _same_bits(dev, _run_device(pkg, matcher, s, s["matches12"]))
    # the device entry one candidate at a time: the batched rows, bit for bit
    for c in range(3):
        lo, hi = s["group"][c], s["group"][c + 1]
        one = dict(s, kfs2=s["kfs2"][lo:hi], group=np.array([0, hi - lo], np.int32), pair_ok=s["pair_ok"][lo:hi],
                   Tcw2=s["Tcw2"][c:c + 1])
        d1 = _run_device(pkg, matcher, one, s["matches12"][lo:hi])
        for k in ALL_KEYS:
            assert torch.equal(d1[k][0], dev[k][c]), (c, k)
    # ok1 = None: derived from mp_id and the bad flags, which is this scene's ok1 except at k = 7
    ok = ((s["kf1"]["mp_id"] >= 0) & (s["bad"][np.maximum(s["kf1"]["mp_id"], 0)] == 0)).astype(np.uint8)
    exp2 = sc.expected_problems(ref, s, s["matches12"], ok1=ok)
    assert exp2[0]["n"] == exp[0]["n"] + 1
    _check_problems(_run_host(pkg, matcher, s, s["matches12"], ok1=None), exp2, n1, "host, ok1 None")
    # one candidate at a time equals the batch
    for c in range(3):
        lo, hi = s["group"][c], s["group"][c + 1]
        one = dict(s, kfs2=s["kfs2"][lo:hi], group=np.array([0, hi - lo], np.int32), pair_ok=s["pair_ok"][lo:hi],
                   Tcw2=s["Tcw2"][c:c + 1])
        _check_problems(_run_host(pkg, matcher, one, s["matches12"][lo:hi]), exp[c:c + 1], n1, f"candidate {c} alone")


def test_problems_from_search(pkg, chain_case):
    s, rows, exp = chain_case
    matcher = pkg.ORBmatcher(sc.NNRATIO, True)
    n1 = len(s["kf1"]["ok"])
    got = matcher.SearchByBoWKFMany(sc.keyframe(pkg, s["kf1"]), [sc.keyframe(pkg, k) for k in s["kfs2"]])
    m12 = np.stack([m for _, m in got])
    assert np.array_equal(m12, rows)
    host = _run_host(pkg, matcher, s, m12)
    _check_problems(host, exp, n1, "host")
    dev = _run_device(pkg, matcher, s, m12, cap=256)
    _check_problems(dev, exp, n1, "device")
    _same_bits(dev, _run_device(pkg, matcher, s, m12, cap=256))


def test_problems_argument_checks(pkg, merge_case):
    s, _ = merge_case
    lib = pkg._lib.load()
    matcher = pkg.ORBmatcher(sc.NNRATIO, True)
    L = pkg._lib
    kf1 = _host_kf(pkg, s["kf1"])
    kfs2 = [_host_kf(pkg, k) for k in s["kfs2"]]
    recs = (L.LoopBowKf * 6)(*[k.record() for k in kfs2])
    C, nc = 12, 3
    outs = {k: np.full((nc, C), 77, np.int32) for k in ("matched_point", "matched_pair", "num_bow", "n", "idx1")}
    outs.update({k: np.full((nc, C, 3), 77, np.float32) for k in ("x3dc1", "x3dc2", "max_err1", "max_err2")})
    out = L.LoopBowOut(*[v.ctypes.data for v in outs.values()])
    group, tcw2, m12 = s["group"], np.ascontiguousarray(s["Tcw2"], np.float32), np.ascontiguousarray(s["matches12"])

    def make(**over):
        a = L.LoopBowIn(kf1.record(), s["kf1"]["ok"].ctypes.data, (ctypes.c_float * 12)(*s["Tcw1"].reshape(12)), 6, 3,
                        ctypes.cast(recs, ctypes.c_void_p), s["pair_ok"].ctypes.data, group.ctypes.data, tcw2.ctypes.data, 20,
                        s["xyz"].ctypes.data, s["bad"].ctypes.data, m12.ctypes.data, C)
        for k, v in over.items():
            setattr(a, k, v)
        return a

    bad_group = np.array([0, 4, 3, 6], np.int32)
    short_group = np.array([0, 3, 5, 5], np.int32)
    cases = [make(n_pairs=-1), make(n_cand=70000), make(group=None), make(Tcw2=None), make(stride=0), make(stride=11),
             make(stride=1 << 20), make(xyz=None), make(matches12=None), make(kf2s=None), make(n_points=-1),
             make(group=bad_group.ctypes.data), make(group=short_group.ctypes.data)]
    k_bad = kf1.record()
    k_bad.nlevels = 13
    cases.append(make(kf1=k_bad))
    k_bad2 = kf1.record()
    k_bad2.mp_id = None
    cases.append(make(kf1=k_bad2))
    h = matcher._handle()
    for i, a in enumerate(cases):
        assert lib.orb_loop_bow_problems(h, ctypes.byref(a), ctypes.byref(out)) == L.ORB_ERR_ARG, i
        assert lib.orb_loop_bow_problems_device(h, ctypes.byref(a), ctypes.byref(out), None) == L.ORB_ERR_ARG, i
    out_bad = L.LoopBowOut(*[v.ctypes.data for v in outs.values()])
    out_bad.n = None
    good = make()
    assert lib.orb_loop_bow_problems(h, ctypes.byref(good), ctypes.byref(out_bad)) == L.ORB_ERR_ARG
    assert lib.orb_loop_bow_problems(None, ctypes.byref(good), ctypes.byref(out)) == L.ORB_ERR_ARG
    assert lib.orb_loop_bow_problems(h, None, ctypes.byref(out)) == L.ORB_ERR_ARG
    assert all((v == 77).all() for v in outs.values())
    assert lib.orb_loop_bow_problems(h, ctypes.byref(good), ctypes.byref(out)) == L.ORB_OK
    assert outs["num_bow"].flat[:3].tolist() == [8, 2, 0]


def test_chain_into_sim3_solver(pkg, chain_case):
    """SearchByBoWKFDevice -> loop_bow_problems (device) -> n read back -> triples -> Sim3Solver's device entry on
    the same tensors.  Equal, bit for bit, to the solver's host entry on the arrays read back (the device pointers
    go in unchanged), and equal to the solver on the restatement's problems in every integer output: the counts,
    the selection and the inlier masks.  The restatement's points differ from the device's by the contraction
    bound, and a hypothesis's transform has no input-independent bound on how far that moves it (a near-collinear
    triple amplifies it without limit), so the transforms are compared where the solver's decision rests on
    them: for the selected hypothesis, to 1e-3 of their magnitude."""
    import torch
    s, rows, exp = chain_case
    matcher = pkg.ORBmatcher(sc.NNRATIO, True)
    cap = 256
    n1 = len(s["kf1"]["ok"])
    K1 = device_keyframe(pkg, sc.keyframe(pkg, s["kf1"]), cap)
    K2 = [device_keyframe(pkg, sc.keyframe(pkg, k), cap) for k in s["kfs2"]]
    m12, cnt = matcher.SearchByBoWKFDevice(K1, K2)
    assert np.array_equal(m12.cpu().numpy()[:, :n1], rows)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ok1 = up(np.concatenate([s["kf1"]["ok"], np.ones(cap - n1, np.uint8)]))
    res = pkg.loop_bow_problems(matcher, _device_kf(pkg, s["kf1"], cap, 1), s["Tcw1"],
                                [_device_kf(pkg, k, cap, 2 + p) for p, k in enumerate(s["kfs2"])], s["group"], s["Tcw2"],
                                up(s["xyz"]), m12, ok1=ok1, bad=up(s["bad"]))
    n = res["n"].cpu().numpy()                    # the one host hop: a count per candidate
    assert n.tolist() == [e["n"] for e in exp]
    rng = np.random.default_rng(3)
    draw = lambda lo, hi: int(rng.integers(lo, hi + 1))  # noqa: E731
    samples = [pkg.draw_samples(int(k), 40, draw) for k in n]
    cam = (458.654, 457.296, 367.215, 248.375)
    dev_probs = pkg.loop_bow_sim3_problems(res, n, [up(x) for x in samples], cam, [cam, cam], False, 3)
    assert dev_probs[0].x3dc1.data_ptr() == res["x3dc1"].data_ptr()
    assert dev_probs[1].max_err2.data_ptr() == res["max_err2"].data_ptr() + 4 * cap
    dev_out = pkg.Sim3Solver(dev_probs).run()
    back = {k: v.cpu().numpy() for k, v in res.items()}
    host_same = pkg.Sim3Solver(pkg.loop_bow_sim3_problems(back, n, samples, cam, [cam, cam], False, 3)).run()
    host_ref = pkg.Sim3Solver([pkg.Sim3Problem(e["x3dc1"], e["x3dc2"], e["max_err1"], e["max_err2"], cam, cam, False, 3, x)
                               for e, x in zip(exp, samples)]).run()
    for c, (d, h, r) in enumerate(zip(dev_out, host_same, host_ref)):
        d = {k: v.cpu().numpy() for k, v in d.items()}
        print(f"candidate {c}: n {n[c]}, winner {int(d['winner'][0])}, best {int(d['best'][0])}, "
              f"max inliers {int(d['hyp_inliers'].max())}")
        assert int(d["winner"][0]) == h["winner"] == r["winner"] and int(d["best"][0]) == h["best"] == r["best"]
        for k in ("hyp_inliers", "inlier_mask"):
            assert np.array_equal(d[k], h[k]) and np.array_equal(d[k], r[k]), (c, k)
        assert int(d["hyp_inliers"].max()) >= 10  # the scene is a consistent Sim3: the chain's output is meaningful
        for k in ("hyp_t12", "hyp_scale"):
            assert np.array_equal(d[k].view(np.uint32), h[k].view(np.uint32)), (c, k)
            a, b = d[k][h["best"]], r[k][h["best"]]
            assert np.all(np.abs(a - b) <= 1e-3 * np.maximum(1.0, np.abs(b))), (c, k, a, b)
