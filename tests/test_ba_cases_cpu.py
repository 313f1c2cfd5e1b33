"""The LocalBA cases of ba_cases.py, from the oracle alone: every case takes the path it states, is eligible
(no close LM decision; the reversed-edge run and the contracted build of the oracle agree on it), and the list as a whole covers every
path of the LM loop that the device restates.  test_ba_cases_gpu.py holds the device to the oracle on the
same cases; this file holds the coverage."""
from __future__ import annotations

import numpy as np
import pytest

import ba_cases as bc


@pytest.fixture(scope="module")
def solved(oracle):
    """name -> ((pose, point, chi2, depth, res, trace) of the forward run, eligibility failures)."""
    return {c.name: bc.check_eligible(oracle, c) for c in bc.CASES}


def test_trace_leaves_the_solve_unchanged(oracle):
    c = bc.get("lambda1e-8_rejects_from_the_start")
    prob = bc.build(c)
    a = oracle.local_ba(prob, c.iterations, c.user_lambda_init)
    b = oracle.local_ba(prob, c.iterations, c.user_lambda_init, trace=True)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert a[4] == b[4]
    tr = b[5]
    assert len(tr) == a[4]["trials"] and int(tr["iteration"][-1]) + 1 == a[4]["iterations"]
    # lambda follows the reject rule between the trials of an iteration: *2, *4, *8, ...
    for i in range(1, len(tr)):
        if tr["iteration"][i] == tr["iteration"][i - 1]:
            assert not tr["accepted"][i - 1] and tr["qmax"][i] == tr["qmax"][i - 1] + 1
            assert tr["lambda"][i] == tr["lambda"][i - 1] * 2.0 ** (tr["qmax"][i - 1] + 1)
    assert np.array_equal(tr["accepted"] != 0, (tr["rho"] > 0) & np.isfinite(tr["temp_chi"]))
    assert tr["lambda"][-1] != a[4]["lambda"]  # the record is the lambda before the trial


def test_contracted_build_is_another_rounding(oracle):
    """The contracted build takes the same path on an eligible case but not the same bits: if the compiler
    ignored the request to contract, the second yardstick would be the first one again."""
    c = bc.get("lambda1e-8_rejects_from_the_start")
    prob = bc.build(c)
    a = bc.solve_oracle(oracle, c, prob)
    b = bc.solve_oracle(oracle, c, prob, contracted=True)
    assert bc.path_string(a[5]) == bc.path_string(b[5]) == c.path
    assert not np.array_equal(a[2], b[2]) and not np.array_equal(a[1], b[1])
    assert np.allclose(a[2], b[2], rtol=1e-7, atol=1e-4)


@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name)
def test_case_takes_its_path_and_is_eligible(solved, case):
    (pose, point, chi2, depth, res, tr), bad = solved[case.name]
    assert bc.path_string(tr) == case.path
    assert bc.end_of(tr, res) == case.end
    assert int((~depth).sum()) == case.neg_depth
    assert res["iterations"] == case.path.count("|") + 1 and res["trials"] == len(case.path.replace("|", ""))
    assert tr["solve_ok"].all()
    assert not bad, bad
    assert not case.nonfinite_rho and np.isfinite(tr["rho"]).all()  # (see ba_cases: no such case is eligible)
    prob = bc.build(case)
    same = np.array_equal(pose, prob["pose"]) and np.array_equal(point, prob["point"])
    assert same == case.unchanged
    n_kf = len(prob["pose"])
    assert n_kf <= 12 or case.name == "pose_mode2_65_free"
    if case.structure is not None:
        assert case.structure in bc.STRUCTURES and "R" in case.path


def _free(case):
    prob = bc.build(case)
    seen = np.zeros(len(prob["pose"]), bool)
    seen[prob["edges"]["pose"]] = True
    return int((seen & (np.asarray(prob["pose_fixed"]) == 0)).sum())


def test_list_covers_every_path(solved):
    its = {c.name: c.path.split("|") for c in bc.CASES}
    covered = {
        "reject then accept in one iteration": [n for n, p in its.items() if any(i.startswith("R") and i.endswith("A") for i in p)],
        "two consecutive rejects (ni >= 8)": [n for n, p in its.items() if any("RR" in i for i in p)],
        "reject in the first iteration": [n for n, p in its.items() if "R" in p[0]],
        "reject in a later iteration": [n for n, p in its.items() if any("R" in i for i in p[1:])],
        "reject in the first and in a later iteration": [n for n, p in its.items()
                                                         if "R" in p[0] and any("R" in i for i in p[1:])],
        "iteration after a multi-trial iteration": [n for n, p in its.items() if any(len(i) > 1 for i in p[:-1])],
        "multi-trial iterations back to back": [n for n, p in its.items()
                                                if any(len(a) > 1 and len(b) > 1 for a, b in zip(p, p[1:]))],
        "last trial rejected (qmax == 10), state unchanged": [c.name for c in bc.CASES
                                                              if c.end == "qmax" and c.path.endswith("R") and c.unchanged],
        "qmax == 10 reached by an accepted tenth trial": [c.name for c in bc.CASES if c.end == "qmax" and c.path.endswith("A")],
        "ends by nBad >= 3": [c.name for c in bc.CASES if c.end == "nbad"],
        "ends by nBad >= 3 after rejects": [c.name for c in bc.CASES if c.end == "nbad" and "R" in c.path],
        "ends by running out of iterations": [c.name for c in bc.CASES if c.end == "iterations"],
        ">= 20 edges of depth <= 0 and >= 20 of depth > 0": [
            c.name for c in bc.CASES
            if c.neg_depth >= 20 and len(solved[c.name][0][3]) - c.neg_depth >= 20 and "R" in c.path],
        "pose_mode 2 (more than 64 free keyframes)": [c.name for c in bc.CASES if _free(c) > 64 and "R" in c.path],
    }
    for s in bc.STRUCTURES:
        covered[f"structure {s} with a reject"] = [c.name for c in bc.CASES if c.structure == s and "R" in c.path]
    for nf in (5, 7, 8):  # n = 30, 42 (no multiples of 16) and 48
        covered[f"{nf} free keyframes (n = {6 * nf}) with a reject"] = [c.name for c in bc.CASES
                                                                        if _free(c) == nf and "R" in c.path]
    missing = [k for k, v in covered.items() if not v]
    assert not missing, missing
    # the stated paths are the oracle's (test_case_takes_its_path_and_is_eligible); the subsets other files use exist
    assert set(bc.VARIANT_CASES) <= set(bc.BY_NAME) and bc.SHARDED_CASE in bc.BY_NAME
    assert any("RR" in i for i in its[bc.SHARDED_CASE])
    assert {"qmax"} <= {bc.get(n).end for n in bc.VARIANT_CASES}
    assert any(bc.get(n).neg_depth >= 20 for n in bc.VARIANT_CASES)
    assert any("RR" in bc.get(n).path for n in bc.VARIANT_CASES)
    big = [c for c in bc.CASES if _free(c) > 64]
    assert all(65 <= _free(c) <= 70 for c in big)
    # a run whose last trial is rejected has work for the restore launch: the oracle's final state is the
    # backup, not the trial's state
    for c in bc.CASES:
        tr = solved[c.name][0][5]
        assert (not tr["accepted"][-1]) == c.path.endswith("R") == c.unchanged
