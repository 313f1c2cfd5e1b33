"""OptimizeSim3 on the CPU: the restatement's controller is pinned to the pose oracle, g2o::Sim3 is checked against
closed forms, the kernel's arithmetic (csrc/orb_optsim3_math.h compiled for the host) agrees with the restatement
on one error pair, one 14-evaluation Jacobian and whole problems, and the scenes of tests/optsim3_scenes.py meet
their conditions."""
from __future__ import annotations

import numpy as np
import pytest

import conftest
import optsim3_ref as ref
import optsim3_scenes as scenes

pkg = conftest.load_package()


# ---- the controller's only independent anchor ------------------------------------------------------------------
def test_controller_is_pinned_to_the_pose_oracle(oracle, synth):
    """lm_optimize with the mono only-pose edge and PoseOptimization's four rounds against the existing oracle:
    poses within 1e-6 RMSE (the project's pose bar), flags and counts identical."""
    frames, edges, _ = synth.pose_opt_batch(n_frames=6, stereo_frac=0.0, seed=43, points_per_frame=[60, 120, 9, 2, 200, 35])
    poses, outl, inl = ref.pose_optimization(frames, edges)
    op, oo, oi = oracle.pose_optimization(frames, edges)
    for a, b in zip(poses, op):
        if np.dot(a[3:], b[3:]) < 0:
            a[3:] = -a[3:]
    rmse = np.sqrt(((poses - op) ** 2).mean(1))
    print("pose RMSE per frame", rmse)
    assert (rmse <= 1e-6).all()
    assert np.array_equal(outl, oo) and np.array_equal(inl, oi)
    assert outl.any() and not outl.all()


# ---- g2o::Sim3 ---------------------------------------------------------------------------------------------
def mat(S):
    M = np.eye(4)
    M[:3, :3] = S.s * ref.quat_to_rot(S.q)
    M[:3, 3] = S.t
    return M


def expm(A):
    """Scaling and squaring with a 24-term series."""
    k = max(0, int(np.ceil(np.log2(max(np.abs(A).sum(1).max(), 1e-300)))) + 4)
    B = A / 2.0 ** k
    E, T = np.eye(len(A)), np.eye(len(A))
    for i in range(1, 25):
        T = T @ B / i
        E = E + T
    for _ in range(k):
        E = E @ E
    return E


UPDATES = {0: [3e-6, -2e-6, 4e-6, 0.3, -0.2, 0.5, 2e-6], 1: [0.3, -0.5, 0.2, 0.3, -0.2, 0.5, -3e-6],
           2: [3e-6, -2e-6, 4e-6, 0.3, -0.2, 0.5, 0.25], 3: [0.3, -0.5, 0.2, 0.3, -0.2, 0.5, -0.4]}


@pytest.mark.parametrize("branch", [0, 1, 2, 3])
def test_sim3_exp_branches_against_the_matrix_exponential(branch):
    u = np.array(UPDATES[branch])
    S, taken = ref.Sim3.exp(u, return_branch=True)
    assert taken == branch
    G = np.zeros((4, 4))
    G[:3, :3] = ref._skew(u[:3]) + u[6] * np.eye(3)
    G[:3, 3] = u[3:6]
    # The reference's branches are approximations, kept as they are.  theta < eps: R = I + Omega + Omega^2 and
    # fixed A, B, off by theta^2 / 2 ~ 2e-11.  |sigma| < eps: C = 1 instead of (e^sigma - 1) / sigma, which moves
    # t = W upsilon by |sigma| / 2 of |upsilon| (and A, B by as much of their smaller terms).
    tol = {0: 1e-10, 1: 1e-13, 2: 1e-10, 3: 1e-13}[branch]
    if branch in (0, 1):
        tol += abs(u[6]) * np.abs(u[3:6]).sum()    # (W = A Omega + B Omega^2 + C I: every term within sigma of its own size)
    M, E = mat(S), expm(G)
    assert np.abs(M - E).max() <= tol
    assert np.abs(M[:3, :3] - E[:3, :3]).max() <= (1e-10 if branch in (0, 2) else 1e-13)
    out = np.zeros(8)
    ref.host_lib().optsim3_host_exp(u.ctypes.data, out.ctypes.data)
    assert np.abs(out - S.vector()).max() <= 1e-15


def test_sim3_inverse_product_and_map_against_closed_forms():
    rng = np.random.default_rng(3)
    A = ref.Sim3.exp(UPDATES[3]) * ref.Sim3([0, 0, 0, 1], [0.1, 0.2, -0.3], 1.3)
    B = ref.Sim3.exp(UPDATES[1])
    X = rng.uniform(-3, 3, (20, 3))
    assert np.abs(mat(A * B) - mat(A) @ mat(B)).max() <= 1e-14
    assert np.abs(mat(A.inverse()) - np.linalg.inv(mat(A))).max() <= 1e-14
    assert np.abs(A.map(X) - (X @ mat(A)[:3, :3].T + mat(A)[:3, 3])).max() <= 1e-14
    assert np.abs((A * A.inverse()).map(X) - X).max() <= 1e-12
    assert np.abs(A.inverse().map(A.map(X)) - X).max() <= 1e-12


# ---- the host build of the kernel's arithmetic -----------------------------------------------------------------
def test_host_arithmetic_one_error_pair_and_one_jacobian():
    """Errors: the same formulas in the same order, a few ulps of ~500 px.  Jacobian: both sides difference errors
    that carry ~1e-13 px of rounding and scale by 1 / 2e-9, so entries of magnitude 1e2-1e3 may differ by ~1e-4;
    the bound is 1e-3."""
    lib = ref.host_lib()
    p, _ = scenes.hand("wrong_pairs_free")
    M = ref.Sim3Model(p)
    P = ref._pairs(p)
    cam = np.asarray(p["cam1"], np.float32)
    s12 = np.asarray(p["s12"], np.float64)
    worst_e = worst_j = 0.0
    for i in (0, 3, 17):
        e = np.zeros(4)
        lib.optsim3_host_errors(s12.ctypes.data, P[i:i + 1].ctypes.data, cam.ctypes.data, cam.ctypes.data, e.ctypes.data)
        e12, e21 = M.edge_errors(M.S, slice(i, i + 1))
        worst_e = max(worst_e, np.abs(e[:2] - e12[0]).max(), np.abs(e[2:] - e21[0]).max())
        for fix in (0, 1):
            J12, J21 = np.zeros((2, 7)), np.zeros((2, 7))
            lib.optsim3_host_jacobian(s12.ctypes.data, fix, P[i:i + 1].ctypes.data, cam.ctypes.data, cam.ctypes.data,
                                      J12.ctypes.data, J21.ctypes.data)
            M.fix = bool(fix)
            R12, R21 = M.jacobians(M.S, slice(i, i + 1))
            worst_j = max(worst_j, np.abs(J12 - R12[0]).max(), np.abs(J21 - R21[0]).max())
            assert np.abs(R12).max() > 50
            if fix:
                assert (J12[:, 6] == 0).all() and (J21[:, 6] == 0).all() and (R12[0][:, 6] == 0).all()
            else:
                # (a left-multiplied scale step scales S12 P2c about camera 1's centre: e12 does not see it)
                assert np.abs(J21[:, 6]).max() > 1 and np.abs(J12[:, 6]).max() < 1e-3
    print(f"host vs restatement: errors {worst_e:.2e} px, Jacobian entries {worst_j:.2e}")
    assert worst_e <= 1e-11 and worst_j <= 1e-3


@pytest.mark.parametrize("name", ["exact_fixed", "exact_free_scale_1p3", "wrong_pairs_free", "left_9", "left_10",
                                  "i2_negative", "n_0", "n_1", "n_257"])
def test_host_arithmetic_full_problem(name):
    """The whole schedule on the host build: the counts and flags of the restatement, the Sim3 within 1e-9 (both
    are float64 with the same formulas; they differ by the summation order and the linear solver's rounding, each
    amplified by the numeric Jacobian's 1e-7 relative noise: three orders inside the GPU test's bar)."""
    p, ex = scenes.hand(name)
    h = ref.host_solve(p)
    d = np.abs(h["s12"] - ex["s12"]).max()
    print(f"{name}: host vs restatement |s12| {d:.2e}, trials {h['trials']} / {ex['trials']}")
    assert h["n_bad"] == ex["n_bad"] and h["n_in"] == ex["n_in"] and np.array_equal(h["inlier"], ex["inlier"])
    assert d <= 1e-9
    if ex["early"]:
        assert np.array_equal(h["s12"], np.asarray(p["s12"], np.float64))


# ---- the scenes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(scenes.HAND))
def test_hand_built_problems_are_decisive(name):
    p, ex = scenes.hand(name)
    n = len(p["p1c"])
    assert ex["decisive"] and ex["decisive1"].all() and ex["decisive2"].all()
    # far from th2, not only decisive: no chi2 of either cull within a factor 2 of it (the +-1e-6 steps of the
    # decisiveness test move a chi2 near th2 by ~1e-2: a factor 2 is three orders beyond that)
    for c in (ex["chi2_12"], ex["chi2_21"]):
        assert not ((c > p["th2"] / 2) & (c < p["th2"] * 2)).any()
    if n >= 10 and not ex["early"]:
        assert np.abs(ex["s12"] - p["truth"]).max() < 1e-5            # the optimisation did its work
        assert np.abs(np.asarray(p["s12"]) - p["truth"]).max() > 1e-2  # from a start a few degrees / cm away


def test_hand_built_paths():
    ex = {k: scenes.hand(k)[1] for k in scenes.HAND}
    assert ex["exact_fixed"]["n_bad"] == 0 and not ex["exact_fixed"]["early"]          # 5 more iterations
    assert ex["wrong_pairs"]["n_bad"] == 6 and ex["wrong_pairs"]["n_in"] == 54          # 10 more iterations
    assert ex["left_9"]["early"] and ex["left_9"]["n_bad"] == 5 and ex["left_9"]["inlier"].sum() == 9
    assert np.array_equal(ex["left_9"]["s12"], scenes.hand("left_9")[0]["s12"])
    assert not ex["left_10"]["early"] and ex["left_10"]["n_in"] == 10
    assert ex["i2_negative"]["n_bad"] == 8 and not ex["i2_negative"]["inlier"][2::5].any()
    p = scenes.hand("exact_free_scale_1p3")[0]
    assert abs(p["s12"][7] - 1.3) < 1e-12 and not p["fix_scale"]
    assert abs(ex["exact_free_scale_1p3"]["s12"][7] - p["truth"][7]) < 1e-6
    assert scenes.hand("exact_fixed")[0]["s12"][7] == 1.0 and ex["exact_fixed"]["s12"][7] == 1.0
    for n in (0, 1, 9):
        assert ex[f"n_{n}"]["early"] and ex[f"n_{n}"]["n_in"] == 0
    for n in (10, 11, 63, 64, 65, 255, 256, 257):
        assert ex[f"n_{n}"]["n_in"] == n
    assert len(scenes.hand("room")[0]["p1c"]) == scenes.ROOM
    # the second stage ran 5 or 10 iterations' worth of trials at the most
    assert ex["exact_fixed"]["trials"][0] >= 5


def test_seeded_batch_meets_its_caps():
    ps, exs = scenes.batch_results()
    assert len(ps) == 12 and all(40 <= len(p["p1c"]) <= 300 for p in ps)
    assert {bool(p["fix_scale"]) for p in ps} == {True, False}
    assert sum(not ex["decisive"] for ex in exs) <= 1
    pairs = sum(len(p["p1c"]) for p, ex in zip(ps, exs) if ex["decisive"])
    und = sum(int((~ex["decisive2"]).sum()) for ex in exs if ex["decisive"])
    assert und <= 0.02 * pairs
    assert all(ex["n_bad"] >= len(p["p1c"]) // 10 for p, ex in zip(ps, exs))       # the wrong pairs are found
