"""Sim3Solver on the CPU: the scenes of tests/sim3_scenes.py meet their own conditions, the kernel's per-lane
arithmetic (csrc/orb_sim3_math.h compiled for the host) agrees with the float64 restatement on them, and the
Python entries that need no GPU (ransac_max_its, draw_samples) and the replay of iterate() do what
src/Sim3Solver.cc does."""
from __future__ import annotations

import numpy as np
import pytest

import conftest
import sim3_ref as ref
import sim3_scenes as scenes

pkg = conftest.load_package()
from orbslam3_amd import sim3  # noqa: E402


@pytest.mark.parametrize("name", list(scenes.CASES))
def test_scene_conditions_and_host_arithmetic(name):
    sc = scenes.build(name)   # asserts (a) - (d)
    ev = sc["ev"]
    t12, scale, bits = ref.host_evaluate(sc)
    decisive = ev["margin"] > ref.DECISIVE
    assert np.array_equal(bits[decisive], ev["bits"][decisive])
    tol = 1e-5 * max(1.0, np.abs(ev["T12"]).max())
    assert np.abs(t12 - ev["T12"]).max() <= tol and np.abs(scale - ev["scale"]).max() <= tol


def test_selection_scenes():
    assert scenes.outlier_then_inliers()["winner"] == 5
    assert scenes.repeated_triple()["best"] == 6


def test_closed_form_does_not_depend_on_the_eigenvector_sign_or_the_solver():
    """A similarity applied to three points is recovered exactly (to float64 rounding) by both solvers."""
    rng = np.random.default_rng(5)
    X2 = rng.uniform(-2, 2, (3, 3)) + [0, 0, 5]
    R = scenes.rodrigues([0.2, -1.0, 0.4], 2.9)      # near pi: w is small and takes either sign
    X1 = (1.7 * X2 @ R.T + [0.3, -0.1, 0.8]).astype(np.float32)
    prob = {"x3dc1": X1, "x3dc2": X2.astype(np.float32), "max_err1": np.ones(3, np.float32), "max_err2": np.ones(3, np.float32),
            "cam1": scenes.CAM_EUROC, "cam2": scenes.CAM_EUROC, "fix_scale": False, "samples": np.array([[0, 1, 2]], np.int32)}
    ev = ref.evaluate(prob)
    t12, scale, bits = ref.host_evaluate(prob)
    assert abs(ev["scale"][0] - 1.7) < 1e-5 and np.abs(ev["T12"][0].reshape(3, 4)[:, :3] - 1.7 * R).max() < 1e-5
    assert np.abs(t12 - ev["T12"]).max() < 1e-5 and bits.all()


def test_identical_triples_give_a_non_finite_transform_on_the_host():
    X = np.array([[0.1, 0.2, 3.0], [1.0, -0.5, 4.0], [-0.7, 0.9, 5.0], [0.4, 0.4, 6.0]], np.float32)
    prob = {"x3dc1": X, "x3dc2": X.copy(), "max_err1": np.full(4, 9.21, np.float32), "max_err2": np.full(4, 9.21, np.float32),
            "cam1": scenes.CAM_EUROC, "cam2": scenes.CAM_EUROC, "fix_scale": False, "samples": np.array([[0, 1, 2]], np.int32)}
    t12, scale, bits = ref.host_evaluate(prob)
    assert not np.isfinite(t12).any() and not bits.any()


def test_ransac_max_its():
    for f in (sim3.ransac_max_its, ref.ransac_max_its):
        assert f(20, 0.99, 20, 300) == 1
        assert f(20, 0.99, 15, 300) == 9
        assert f(100, 0.99, 15, 300) == 300
        assert f(14, 0.99, 15, 300) is None
        assert f(100, 0.99, 15, 0) == 1       # max(1, min(nIterations, maxIts))


def test_draw_samples_swap_with_back():
    # n = 6, scripted draws.  Iteration 0: r = 5 -> 5, list [0 1 2 3 4]; r = 0 -> 0, list [4 1 2 3]; r = 0 -> 4.
    # Iteration 1 starts from the full list again: r = 2 -> 2, list [0 1 5 3 4]; r = 2 -> 5, list [0 1 4 3];
    # r = 3 -> 3.
    script = [5, 0, 0, 2, 2, 3]
    calls = []

    def rng(lo, hi):
        calls.append((lo, hi))
        return script[len(calls) - 1]

    for f in (sim3.draw_samples, ref.draw_samples):
        calls.clear()
        assert f(6, 2, rng).tolist() == [[5, 0, 4], [2, 5, 3]]
        assert calls == [(0, 5), (0, 4), (0, 3)] * 2


def test_replay_of_iterate_chunks():
    # min_inliers 10, 50 hypotheses, nothing converges until hypothesis 45
    counts = [0] * 50
    counts[3], counts[7], counts[12] = 4, 6, 6      # chunk 0: best 3, then 7, then 12 (a later tie wins)
    counts[25] = 5                                  # chunk 1: below the best carried over from chunk 0
    counts[45] = 11
    r = ref.Replay(counts, n=30, min_inliers=10, max_its=50)
    a = r.iterate(20, with_converge=True)
    assert a == {"hyp": 12, "no_more": False, "n_inliers": 0, "converge": False} and r.best == 12 and r.best_inliers == 6
    b = r.iterate(20, with_converge=True)
    assert b["hyp"] == -1 and not b["no_more"] and r.best == 12     # the best persists, the chunk set none
    c = r.iterate(20, with_converge=True)
    assert c == {"hyp": 45, "no_more": False, "n_inliers": 11, "converge": True} and r.iterations == 46
    # without convergence: bNoMore at the cap, the first overload returns the identity
    r = ref.Replay([0, 2, 2, 1], n=30, min_inliers=10, max_its=4)
    assert r.iterate(3) == {"hyp": -1, "no_more": False, "n_inliers": 0, "converge": False}
    d = r.iterate(20)
    assert d["no_more"] and d["hyp"] == -1 and r.best == 2 and r.iterations == 4
    # n < min_inliers: bNoMore at once
    assert ref.Replay([], n=5, min_inliers=6, max_its=10).iterate(20)["no_more"]
