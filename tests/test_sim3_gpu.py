"""orb_sim3_ransac / orb_sim3_ransac_device against the float64 restatement (tests/sim3_ref.py) on the scenes of
tests/sim3_scenes.py.

Mask parity is exact on every decisive pair (relative margin > 1e-3 in float64) and the counts lie in
[decided, decided + undecided].  Transform parity: |T12 - T12_ref| <= 1e-5 max(1, max |T12_ref|), and the same
bound on the scale -- derived, not measured: the closed form is FP64 rounded to float32 once (6e-8 relative), the
scenes' eigen-gaps are >= 1e-6 so the eigenvector is good to ~1e-10; 1e-5 leaves two orders of margin."""
from __future__ import annotations

import numpy as np
import pytest

import sim3_ref as ref
import sim3_scenes as scenes

pytestmark = pytest.mark.gpu

KEYS = ("hyp_inliers", "hyp_t12", "hyp_scale", "winner", "best", "inlier_mask")


def problem(pkg, sc, device=False, samples=None):
    import torch
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else (lambda a: a)
    smp = sc["samples"] if samples is None else samples
    return pkg.Sim3Problem(up(sc["x3dc1"]), up(sc["x3dc2"]), up(sc["max_err1"]), up(sc["max_err2"]), sc["cam1"], sc["cam2"],
                           sc["fix_scale"], sc["min_inliers"], up(np.asarray(smp, np.int32)))


def to_host(r):
    """A device result as the host form returns it (hyp_mask's int64 carrier back to uint64)."""
    import torch
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in r.items()}
    out["winner"], out["best"] = int(out["winner"][0]), int(out["best"][0])
    if "hyp_mask" in out:
        out["hyp_mask"] = out["hyp_mask"].view(np.uint64)
    return out


def unpack(words, n):
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")
    return bits[..., :n].astype(bool)


def same(a, b, keys=KEYS):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in keys)


def check_against_reference(sc, r):
    ev, n = sc["ev"], len(sc["x3dc1"])
    bits = unpack(r["hyp_mask"], n)
    decisive = ev["margin"] > ref.DECISIVE
    assert np.array_equal(bits[decisive], ev["bits"][decisive])
    cnt = r["hyp_inliers"]
    assert np.array_equal(cnt, bits.sum(1))
    assert ((cnt >= sc["lo"]) & (cnt <= sc["lo"] + sc["und"])).all()
    tol = 1e-5 * max(1.0, np.abs(ev["T12"]).max())
    assert np.abs(r["hyp_t12"] - ev["T12"]).max() <= tol
    assert np.abs(r["hyp_scale"] - ev["scale"]).max() <= tol
    if sc["fix_scale"]:
        assert (r["hyp_scale"] == 1.0).all()
    # the selection over the device's own counts, and against what the scene determines
    conv = np.flatnonzero(cnt > sc["min_inliers"])
    assert r["winner"] == (int(conv[0]) if len(conv) else -1) == sc["winner"]
    assert r["best"] == int(np.flatnonzero(cnt == cnt.max())[-1])
    if sc["best"] is not None:
        assert r["best"] == sc["best"]
    row = r["winner"] if r["winner"] >= 0 else r["best"]
    assert np.array_equal(r["inlier_mask"].astype(bool), bits[row])


@pytest.mark.parametrize("name", list(scenes.CASES))
def test_parity_host_form(pkg, name):
    sc = scenes.build(name)
    (r,) = pkg.Sim3Solver(problem(pkg, sc)).run(hyp_mask=True)
    check_against_reference(sc, r)
    if name == "n3":
        assert r["hyp_inliers"].tolist() == [3] and r["winner"] == -1 and r["best"] == 0 and r["inlier_mask"].all()


@pytest.mark.parametrize("name", ["n65", "h65", "n200_free"])
def test_forms_agree(pkg, name):
    sc = scenes.build(name)
    (host,) = pkg.Sim3Solver(problem(pkg, sc)).run(hyp_mask=True)
    (dev,) = pkg.Sim3Solver(problem(pkg, sc, device=True)).run(hyp_mask=True)
    assert same(host, to_host(dev), KEYS + ("hyp_mask",))
    (host0,) = pkg.Sim3Solver(problem(pkg, sc)).run()
    (dev0,) = pkg.Sim3Solver(problem(pkg, sc, device=True)).run()
    assert "hyp_mask" not in host0 and same(host, host0) and same(host, to_host(dev0))


def test_winner_is_the_first_to_converge(pkg):
    sc = scenes.outlier_then_inliers()
    (r,) = pkg.Sim3Solver(problem(pkg, sc)).run(hyp_mask=True)
    check_against_reference(sc, r)
    assert r["winner"] == 5 and r["hyp_inliers"][6] > sc["min_inliers"]


def test_later_tie_is_best(pkg):
    sc = scenes.repeated_triple()
    (r,) = pkg.Sim3Solver(problem(pkg, sc)).run(hyp_mask=True)
    check_against_reference(sc, r)
    assert r["winner"] == -1 and r["best"] == 6 and r["hyp_inliers"][2] == r["hyp_inliers"][6]
    assert np.array_equal(r["hyp_t12"][2], r["hyp_t12"][6])


def degenerate(sc, rows):
    """The scene with points 0 .. 2 of set 1 overwritten by set 2's (the triple (0, 1, 2) then has |v| = 0)."""
    d = dict(sc)
    d["x3dc1"] = sc["x3dc1"].copy()
    d["x3dc1"][:3] = sc["x3dc2"][:3]
    d["samples"] = np.array(rows, np.int32)
    d["min_inliers"] = len(d["x3dc1"])      # nothing converges
    return d


def test_identical_triple_scores_zero(pkg):
    sc = scenes.build("h64")
    # alone, and twice: everything scores 0, the last one is best
    for rows in ([[0, 1, 2]], [[0, 1, 2], [2, 0, 1]]):
        (r,) = pkg.Sim3Solver(problem(pkg, degenerate(sc, rows))).run()
        assert (r["hyp_inliers"] == 0).all() and not np.isfinite(r["hyp_t12"]).any() and not np.isfinite(r["hyp_scale"]).any()
        assert r["winner"] == -1 and r["best"] == len(rows) - 1 and not r["inlier_mask"].any()
    # before and after a hypothesis that scores: it loses both ways
    good = next(row.tolist() for h, row in enumerate(sc["samples"]) if sc["lo"][h] > 10 and row.min() >= 3)
    for rows, best in (([[0, 1, 2], good], 1), ([good, [0, 1, 2]], 0)):
        (r,) = pkg.Sim3Solver(problem(pkg, degenerate(sc, rows))).run()
        assert r["hyp_inliers"][1 - best] == 0 and r["hyp_inliers"][best] > 0 and r["best"] == best
        assert r["inlier_mask"].sum() == r["hyp_inliers"][best]


def test_batch_equals_single_calls(pkg):
    a, b = scenes.build("n130"), scenes.build("other_cam")
    skipped = dict(scenes.build("n20_h9"), min_inliers=21)            # n < min_inliers: bNoMore, not evaluated
    c = scenes.build("h65")
    batch = pkg.Sim3Solver([problem(pkg, s) for s in (a, skipped, b, c)]).run(hyp_mask=True)
    for sc, r in zip((a, skipped, b, c), batch):
        (single,) = pkg.Sim3Solver(problem(pkg, sc)).run(hyp_mask=True)
        assert same(single, r, KEYS + ("hyp_mask",))
    assert batch[1]["winner"] == -1 and batch[1]["best"] == -1 and not batch[1]["inlier_mask"].any()
    assert not batch[1]["hyp_inliers"].any()                          # not written
    dev = pkg.Sim3Solver([problem(pkg, s, device=True) for s in (a, skipped, b, c)]).run(hyp_mask=True)
    for r, d in zip(batch, dev):
        assert same(r, to_host(d), KEYS + ("hyp_mask",))
    # more problems than one launch carries (16)
    many = pkg.Sim3Solver([problem(pkg, s) for s in (a, b, c)] * 6).run()
    for k, r in enumerate(many):
        assert same(batch[(0, 2, 3)[k % 3]], r)
    assert pkg.Sim3Solver([]).run() == []


@pytest.mark.parametrize("bad", [[0, 1, 24], [0, -1, 2], [3, 7, 3]])
def test_invalid_triples(pkg, bad):
    sc = scenes.build("h64")                                           # n = 24
    smp = sc["samples"].copy()
    smp[0] = bad                                                       # hypothesis 0 would have been the winner
    with pytest.raises(pkg.OrbGpuError) as e:
        pkg.Sim3Solver(problem(pkg, sc, samples=smp)).run()
    assert e.value.code == pkg._lib.ORB_ERR_ARG
    (r,) = pkg.Sim3Solver(problem(pkg, sc, device=True, samples=smp)).run(hyp_mask=True)
    r = to_host(r)
    (ok,) = pkg.Sim3Solver(problem(pkg, sc)).run(hyp_mask=True)
    assert r["hyp_inliers"][0] == -1 and not np.isfinite(r["hyp_t12"][0]).any() and not r["hyp_mask"][0].any()
    assert np.array_equal(r["hyp_inliers"][1:], ok["hyp_inliers"][1:]) and np.array_equal(r["hyp_mask"][1:], ok["hyp_mask"][1:])
    conv = np.flatnonzero(r["hyp_inliers"] > sc["min_inliers"])
    assert r["winner"] == conv[0] > 0 and r["best"] > 0
    # every row invalid: nothing is chosen
    (r,) = pkg.Sim3Solver(problem(pkg, sc, device=True, samples=np.tile(np.array(bad, np.int32), (5, 1)))).run()
    r = to_host(r)
    assert (r["hyp_inliers"] == -1).all() and r["winner"] == -1 and r["best"] == -1 and not r["inlier_mask"].any()


def test_argument_errors(pkg):
    sc = scenes.build("h1")
    with pytest.raises(pkg.OrbGpuError) as e:
        pkg.Sim3Solver(problem(pkg, sc, samples=np.zeros((1025, 3), np.int32))).run()
    assert e.value.code == pkg._lib.ORB_ERR_ARG
