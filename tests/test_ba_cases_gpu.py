"""LocalBA on the cases of ba_cases.py -- problems on which g2o's LM loop rejects trials -- against the CPU
oracle at the bars of test_ba_gpu.py: the same LM path (iterations, trials, termination), final chi2 and
lambda to 1e-9 relative, poses, quaternions and points within 1e-6 RMSE, the edge chi2 tolerances of
test_local_ba_c5_parity, identical depth flags; and input bytes back where the run ends on a rejected trial
at qmax == 10.  test_ba_cases_cpu.py establishes from the oracle alone which path each case takes."""
from __future__ import annotations

import numpy as np
import pytest

import ba_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver(pkg):
    return pkg.LocalBA()


@pytest.fixture(scope="module")
def reference(oracle):
    """name -> (problem, oracle run with its trace), computed once per case."""
    memo = {}

    def get(name):
        if name not in memo:
            case = bc.get(name)
            prob = bc.build(case)
            memo[name] = (prob, bc.solve_oracle(oracle, case, prob))
        return memo[name]
    return get


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name)
def test_case_against_oracle(solver, reference, case):
    prob, ref = reference(case.name)
    assert bc.path_string(ref[5]) == case.path  # the path this case is here for
    got = solver.optimize(prob, case.iterations, user_lambda_init=case.user_lambda_init)
    bc.assert_matches_oracle(case, prob, got, ref)
    # the same case again on the same handle: a stale backup or LM state would show
    again = solver.optimize(prob, case.iterations, user_lambda_init=case.user_lambda_init)
    for a, b in zip(got[:4], again[:4]):
        assert a.tobytes() == b.tobytes()
    assert got[4] == again[4]


def test_rejecting_case_after_a_restored_one(pkg, reference):
    """A fresh handle solves the qmax == 10 case (its last launch restores the backups) and then a case that
    rejects and accepts: nothing of the first solve's LM state may reach the second."""
    solver = pkg.LocalBA()
    for name in ("qmax_unchanged", "lambda1e-8_rejects_from_the_start", "qmax_unchanged"):
        case = bc.get(name)
        prob, ref = reference(name)
        got = solver.optimize(prob, case.iterations, user_lambda_init=case.user_lambda_init)
        bc.assert_matches_oracle(case, prob, got, ref, tag="in sequence: ")


@pytest.mark.parametrize("name", ["negative_depth_points_mirrored", "poses_far_n30"])
def test_culling_erases_negative_depth(pkg, reference, name):
    case = bc.get(name)
    prob, ref = reference(name)
    _, _, rchi2, rdepth = ref[:4]
    pose, point, erase, res = pkg.local_bundle_adjustment(prob, case.iterations)
    assert 0 < (~rdepth).sum() < len(rdepth)
    assert 20 <= (~rdepth).sum() <= len(rdepth) - 20
    st = prob["edges"]["stereo"] != 0
    rerase = np.where(st, rchi2 > 7.815, rchi2 > 5.991) | ~rdepth
    # an edge whose oracle chi2 sits within the chi2 tolerance of its threshold is no decision of the culling
    th = np.where(st, 7.815, 5.991)
    assert np.all(np.abs(rchi2 - th) > 1e-3 + 1e-6 * rchi2), "a chi2 on the culling threshold: pick another case"
    assert np.array_equal(erase, rerase)
    assert np.all(erase[~rdepth])
