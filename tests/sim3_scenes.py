"""Seeded scenes for the Sim3Solver tests: two sets of camera-frame points related by a known Sim3, with noise and
gross outliers, and sample triples drawn by the reference's swap-with-back scheme (sim3_ref.draw_samples).

Points of set 2 lie in a 4 x 3 x 6 m box, 2 to 8 m deep; set 1 = s R X2 + t with a 0.3 rad rotation and s = 1.3
(1 when the scale is fixed) plus 4 mm of noise; 30 % of the correspondences are gross outliers (set 1 replaced
by an unrelated point of the box); sigma2 = 1.2^(2 octave) with octaves 0 .. 7; an EuRoC-like pinhole camera.

build() asserts what makes a scene a fair yardstick -- conditions on the inputs, met by the float64 restatement
alone, not tolerances on the kernel:
  (a) undecided pairs (relative margin <= 1e-3) are at most 0.5 % of all pairs;
  (b) every triple's eigen-gap is >= 1e-6;
  (c) no hypothesis's interval [decided inliers, decided + undecided] straddles the `> min_inliers` decision;
  (d) where no hypothesis converges, the maximum count beats the runner-up by more than the undecided pairs of
      both (so `best` is determined).
"""
from __future__ import annotations

import functools

import numpy as np

import sim3_ref as ref

f32 = np.float32
CAM_EUROC = (458.654, 457.296, 367.215, 248.375)
CAM_OTHER = (435.2, 435.2, 319.5, 239.5)


def rodrigues(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def random_problem(n, n_hyp, fix_scale, min_inliers, seed, noise=0.004, outliers=0.3, cam1=CAM_EUROC, cam2=CAM_EUROC):
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-2.0, -1.5, 2.0]), np.array([2.0, 1.5, 8.0])
    X2 = rng.uniform(lo, hi, (n, 3))
    s = 1.0 if fix_scale else 1.3
    R = rodrigues(rng.normal(size=3), 0.3)
    t = rng.uniform(-0.3, 0.3, 3) + np.array([0.0, 0.0, 0.5])
    X1 = s * X2 @ R.T + t + rng.normal(scale=noise, size=(n, 3))
    bad = rng.random(n) < outliers
    X1[bad] = s * rng.uniform(lo, hi, (int(bad.sum()), 3)) @ R.T + t
    sigma2 = (f32(1.2) ** (2 * np.arange(8))).astype(f32)
    o1, o2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    samples = ref.draw_samples(n, n_hyp, lambda a, b: int(rng.integers(a, b + 1)))
    return {"x3dc1": X1.astype(f32), "x3dc2": X2.astype(f32), "max_err1": ref.max_err(sigma2[o1]),
            "max_err2": ref.max_err(sigma2[o2]), "cam1": cam1, "cam2": cam2, "fix_scale": bool(fix_scale),
            "min_inliers": int(min_inliers), "samples": samples, "outlier": bad}


def with_reference(prob, ties=False):
    """prob plus its float64 evaluation (`ev`), the count bounds (`lo`, `und`) and the determined `winner` /
    `best`, after the scene assertions (a) - (d).  ties: the scene repeats a triple on purpose, so (d) compares
    with the runner-up among the other counts."""
    ev = ref.evaluate(prob)
    lo, und = ref.count_bounds(ev)
    m = prob["min_inliers"]
    assert (ev["margin"] <= ref.DECISIVE).mean() <= 5e-3, "(a) too many undecided pairs"
    assert ev["gap"].min() >= 1e-6, "(b) a triple with a small eigen-gap"
    assert not ((lo <= m) & (lo + und > m)).any(), "(c) a hypothesis straddles the min_inliers decision"
    conv = np.flatnonzero(lo > m)
    winner = int(conv[0]) if len(conv) else -1
    best = None   # not determined by the reference when a hypothesis converges: the tests use the device counts
    if winner < 0:
        top = int(lo.max())
        at_top = np.flatnonzero(lo == top)
        best = int(at_top[-1])
        same = (prob["samples"] == prob["samples"][best]).all(1) if ties else np.arange(len(lo)) == best
        assert len(at_top) == 1 or ties, "(d) an unplanned tie"
        rest = ~same
        if rest.any():
            assert (lo + und)[rest].max() < lo[same].min(), "(d) the runner-up is within the undecided pairs"
    return dict(prob, ev=ev, lo=lo, und=und, winner=winner, best=best)


# name: (n, n_hyp, fix_scale, min_inliers, seed, extra keywords) -- seeds for which (a) - (d) hold
CASES = {
    "n3": (3, 1, False, 3, 1, {"noise": 0.0, "outliers": 0.0}),
    "n20_h9": (20, 9, False, 15, 2, {}),
    "n64": (64, 16, False, 12, 1, {}),
    "n65": (65, 16, True, 12, 1, {}),
    "n130": (130, 16, False, 20, 1, {}),
    "h1": (24, 1, False, 6, 1, {}),
    "h64": (24, 64, False, 6, 1, {}),
    "h65": (24, 65, True, 6, 1, {}),
    "n200_free": (200, 300, False, 20, 1, {}),
    "n200_fixed": (200, 300, True, 20, 1, {}),
    "other_cam": (40, 30, True, 10, 1, {"cam2": CAM_OTHER}),
}


@functools.lru_cache(maxsize=None)
def build(name):
    n, n_hyp, fix_scale, min_inliers, seed, kw = CASES[name]
    if name == "n3":
        prob = random_problem(n, n_hyp, fix_scale, min_inliers, seed, **kw)
        prob["samples"] = np.array([[0, 1, 2]], np.int32)
        return with_reference(prob)
    return with_reference(random_problem(n, n_hyp, fix_scale, min_inliers, seed, **kw))


def outlier_then_inliers(k=5, n=60, seed=1):
    """Hypotheses 0 .. k-1 hold a gross outlier (none converges), k and k + 1 are all-inlier triples that both
    converge: winner == k."""
    prob = random_problem(n, k + 2, False, 12, seed)
    good, bad = np.flatnonzero(~prob["outlier"]), np.flatnonzero(prob["outlier"])
    rows = [[bad[h], good[2 * h], good[2 * h + 1]] for h in range(k)]
    # well spread inliers for the two converging triples
    X = prob["x3dc2"][good]
    far = [int(np.argmin(X[:, 0])), int(np.argmax(X[:, 0])), int(np.argmax(X[:, 1])), int(np.argmin(X[:, 1])),
           int(np.argmax(X[:, 2]))]
    assert len(set(far)) == 5
    rows += [[good[far[0]], good[far[1]], good[far[2]]], [good[far[3]], good[far[1]], good[far[4]]]]
    prob["samples"] = np.array(rows, np.int32)
    sc = with_reference(prob)
    assert sc["winner"] == k and sc["lo"][k + 1] > prob["min_inliers"] and (sc["lo"][:k] + sc["und"][:k]
                                                                            <= prob["min_inliers"]).all()
    return sc


def repeated_triple(i=2, j=6, n=40, n_hyp=8, seed=3):
    """Nothing converges (min_inliers above every count); the triple with the most inliers stands at rows i < j:
    best == j."""
    prob = random_problem(n, n_hyp, False, n, seed)
    ev = ref.evaluate(prob)
    lo, _ = ref.count_bounds(ev)
    top = int(np.argmax(lo))
    s = prob["samples"].copy()
    keep = s[top].copy()
    others = [r for h, r in enumerate(s) if h != top]
    rows = []
    for h in range(n_hyp):
        rows.append(keep if h in (i, j) else others.pop())
    prob["samples"] = np.array(rows, np.int32)
    sc = with_reference(prob, ties=True)
    assert sc["winner"] == -1 and sc["best"] == j
    return sc
