"""orb_optimize_sim3 / orb_optimize_sim3_device against the float64 restatement (tests/optsim3_ref.py) on the
problems of tests/optsim3_scenes.py.

On a decisive problem: s12_out within 1e-6 of the restatement (the project's pose bar, the maximum over the 8
entries), n_bad equal, inlier equal on the pairs decisive at both culls, n_in equal up to the second cull's
non-decisive count.  The kernel differentiates numerically as the reference does; the measured worst difference
is printed here and recorded in DESIGN.md section 4n."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import optsim3_ref as ref
import optsim3_scenes as scenes

pytestmark = pytest.mark.gpu

BAR = 1e-6
KEYS = ("s12", "n_in", "n_bad", "inlier", "chi2_12", "chi2_21")


def check(p, ex, r):
    """Returns |s12 - s12_ref| max."""
    assert ex["decisive"]
    d = float(np.abs(r["s12"] - ex["s12"]).max())
    print(f"n={len(p['p1c'])} n_bad={r['n_bad']} n_in={r['n_in']} |s12 - ref|={d:.3e}")
    assert r["n_bad"] == ex["n_bad"]
    both = ex["decisive1"] & ex["decisive2"]
    assert np.array_equal(r["inlier"][both], ex["inlier"][both])
    assert abs(r["n_in"] - ex["n_in"]) <= int((~ex["decisive2"]).sum())
    assert r["n_in"] == (0 if ex["early"] else int(r["inlier"].sum()))
    if ex["early"]:
        assert np.array_equal(r["s12"], np.asarray(p["s12"], np.float64))    # bit-identical to the input
    assert d <= BAR
    return d


@pytest.mark.parametrize("name", list(scenes.HAND))
def test_hand_built(pkg, name):
    p, ex = scenes.hand(name)
    r = pkg.optimize_sim3([p], chi2=True)[0]
    check(p, ex, r)
    if len(p["p1c"]):
        both = ex["decisive1"] & ex["decisive2"]
        far = np.maximum(ex["chi2_12"], ex["chi2_21"])[both]
        got = np.maximum(r["chi2_12"], r["chi2_21"])[both]
        assert np.array_equal(far > p["th2"], got > p["th2"])


def test_left_9_returns_the_input_and_left_10_does_not(pkg):
    (p9, e9), (p10, e10) = scenes.hand("left_9"), scenes.hand("left_10")
    r9, r10 = pkg.optimize_sim3([p9, p10])
    assert r9["n_in"] == 0 and r9["n_bad"] == 5 and r9["s12"].tobytes() == np.asarray(p9["s12"], np.float64).tobytes()
    assert r9["inlier"].sum() == 9                       # vpMatches1 is culled all the same
    assert r10["n_in"] == 10 and r10["n_bad"] == 5 and not np.array_equal(r10["s12"], p10["s12"])


def test_seeded_batch(pkg):
    ps, exs = scenes.batch_results()
    rs = pkg.optimize_sim3(ps)
    worst = 0.0
    for p, ex, r in zip(ps, exs, rs):
        if ex["decisive"]:
            worst = max(worst, check(p, ex, r))
    print(f"seeded batch: worst |s12 - ref| = {worst:.3e}")


def to_host(r):
    import torch
    torch.cuda.synchronize()
    out = {k: r[k].cpu().numpy() for k in KEYS if k in r}
    out["n_in"], out["n_bad"], out["inlier"] = int(out["n_in"][0]), int(out["n_bad"][0]), out["inlier"].astype(bool)
    return out


def same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


def test_device_entry_and_a_second_call_give_the_same_bits(pkg):
    import torch
    ps, _ = scenes.batch_results()
    ps = list(ps) + [scenes.hand(k)[0] for k in ("n_0", "n_9", "left_9", "exact_free_scale_1p3")]
    a = pkg.optimize_sim3(ps, chi2=True)
    b = pkg.optimize_sim3(ps, chi2=True)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    dps = [{**p, **{k: up(p[k]) for k in ("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")}} for p in ps]
    d = [to_host(r) for r in pkg.optimize_sim3(dps, chi2=True)]
    for x, y, z in zip(a, b, d):
        assert same(x, y) and same(x, z)


def test_more_problems_than_one_launch_holds(pkg):
    p, ex = scenes.hand("n_11")
    q, eq = scenes.hand("wrong_pairs")
    rs = pkg.optimize_sim3([p, q] * 9)                     # 18 problems: two launches
    one = pkg.optimize_sim3([p, q])
    for i, r in enumerate(rs):
        assert same({**r, "chi2_12": 0, "chi2_21": 0}, {**one[i & 1], "chi2_12": 0, "chi2_21": 0})


def test_empty_batch(pkg):
    lib = pkg._lib.load()
    assert pkg.optimize_sim3([]) == []
    assert lib.orb_optimize_sim3(None, 0, None) == 0
    assert lib.orb_optimize_sim3_device(None, 0, None, None) == 0


def raw(pkg, p, n=None, **override):
    """One problem / output record pair on host arrays, with fields overridden (None: a NULL pointer)."""
    L = pkg._lib
    n = len(p["p1c"]) if n is None else n
    arrs = {k: np.ascontiguousarray(p[k], np.float64 if j < 4 else np.float32)
            for j, k in enumerate(("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"))}
    outs = {"s12_out": np.full(8, 7.0), "n_in": np.full(1, -7, np.int32), "n_bad": np.full(1, -7, np.int32),
            "inlier": np.full(max(n, 1), 7, np.uint8)}
    ptr = {k: v.ctypes.data for k, v in {**arrs, **outs}.items()}
    ptr.update({k: v for k, v in override.items() if k in ptr})
    th2 = override.get("th2", float(p["th2"]))
    prob = L.OptSim3Problem(n, ptr["p1c"], ptr["p2c"], ptr["obs1"], ptr["obs2"], ptr["inv_sigma2_1"], ptr["inv_sigma2_2"],
                            (ctypes.c_float * 4)(*p["cam1"]), (ctypes.c_float * 4)(*p["cam2"]),
                            (ctypes.c_double * 8)(*p["s12"]), th2, int(p["fix_scale"]))
    out = L.OptSim3Out(ptr["s12_out"], ptr["n_in"], ptr["n_bad"], ptr["inlier"], None, None)
    return prob, out, arrs, outs


@pytest.mark.parametrize("entry", ["host", "device"])
def test_argument_rejections_touch_nothing(pkg, entry):
    L = pkg._lib
    lib = L.load()
    p, _ = scenes.hand("n_11")

    def call(prob, out, k=1):
        probs, outs = (L.OptSim3Problem * 1)(prob), (L.OptSim3Out * 1)(out)
        if entry == "host":
            return lib.orb_optimize_sim3(probs, k, outs)
        return lib.orb_optimize_sim3_device(probs, k, outs, None)

    # (the device entry is only ever given records it rejects here: their host pointers are never read)
    cases = [dict(n=scenes.ROOM + 1), dict(n=-1), dict(th2=0.0), dict(th2=float("nan")), dict(p1c=None), dict(obs2=None),
             dict(inv_sigma2_2=None), dict(s12_out=None), dict(n_in=None), dict(n_bad=None), dict(inlier=None)]
    for c in cases:
        prob, out, arrs, outs = raw(pkg, p, **c)
        assert call(prob, out) == L.ORB_ERR_ARG, c
        assert (outs["s12_out"] == 7.0).all() and outs["n_in"][0] == -7 and outs["n_bad"][0] == -7 and (outs["inlier"] == 7).all()
    prob, out, arrs, outs = raw(pkg, p)
    assert call(prob, out, k=-1) == L.ORB_ERR_ARG
    if entry == "host":
        assert lib.orb_optimize_sim3(None, 1, None) == L.ORB_ERR_ARG
    else:
        assert lib.orb_optimize_sim3_device(None, 1, None, None) == L.ORB_ERR_ARG
    with pytest.raises(L.OrbGpuError):
        big = scenes.make(scenes.ROOM + 1, 9, fix_scale=True)
        pkg.optimize_sim3([big])


def test_room_boundary(pkg):
    """ORB_OPTSIM3_MAX_PAIRS pairs fill the LDS room and are solved; one more is ORB_ERR_ARG (above)."""
    p, ex = scenes.hand("room")
    assert len(p["p1c"]) == scenes.ROOM == pkg.optimizer.OPTSIM3_MAX_PAIRS
    check(p, ex, pkg.optimize_sim3([p])[0])
