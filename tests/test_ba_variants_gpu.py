"""The LocalBA paths a plain C5 solve does not take, each against the CPU oracle at the 1e-6 bar:
  * ORBGPU_BA_CHOL=rows: the tile-row multi-workgroup Cholesky (k_ba_chol_rows), which windows above
    48 free keyframes use, here at n = 288;
  * ORBGPU_BA_FAST_UNIT=0: the 6-launch LM unit (the one sharded solves and windows above 48 free
    keyframes run) on one process;
  * ORBGPU_BA_UNITS=1 / 8: one and eight LM trials per graph launch.
The switches are read once per process, so each variant solves in a child process (tools/ba_dump.py:
the C5 problem, mono and 50 % stereo) and the saved results are compared here.

The 6-launch unit and the tile-row Cholesky also solve ba_cases.VARIANT_CASES -- runs that reject LM trials, end
on a rejected trial at qmax == 10 and leave edges behind the camera -- in that same child process, and
test_ba_variant_case_against_oracle holds each to the bars of test_ba_cases_gpu.py."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


_WITH_CASES = ("rows", "unit6")  # the variants whose child process also solves ba_cases.VARIANT_CASES
_MEMO = {}


def _solve(tmp_path, name, env_extra):
    if name not in _MEMO:  # one child process per switch, shared by the tests of this module
        _MEMO[name] = _solve_once(tmp_path, name, env_extra)
    return _MEMO[name]


def _solve_once(tmp_path, name, env_extra):
    out = tmp_path / f"{name}.npz"
    env = dict(os.environ)
    for k in ("ORBGPU_BA_CHOL", "ORBGPU_BA_TRACE", "ORBGPU_BA_FAST_UNIT", "ORBGPU_BA_UNITS"):
        env.pop(k, None)
    env.update(env_extra)
    import ba_cases
    extra = [",".join(ba_cases.VARIANT_CASES)] if name in _WITH_CASES else []
    subprocess.run([sys.executable, str(ROOT / "tools" / "ba_dump.py"), str(out)] + extra, env=env, check=True,
                   timeout=100)
    return dict(np.load(out))


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


@pytest.mark.gpu
# (explicit ids: the ones these cases had while the retired variants stood between them in this list, so
# that their test ids, which pytest would otherwise number by position, did not change when those left)
@pytest.mark.parametrize("name,env", [pytest.param("rows", {"ORBGPU_BA_CHOL": "rows"}, id="rows-env0"),
                                      pytest.param("unit6", {"ORBGPU_BA_FAST_UNIT": "0"}, id="unit6-env3"),
                                      pytest.param("units1", {"ORBGPU_BA_UNITS": "1"}, id="units1-env5"),
                                      pytest.param("units8", {"ORBGPU_BA_UNITS": "8"}, id="units8-env6")])
def test_ba_variant_against_oracle(tmp_path, oracle, synth, name, env):
    got = _solve(tmp_path, name, env)
    for st in (0.0, 0.5):
        tag = f"s{int(st * 10)}"
        prob = synth.local_ba_problem(stereo_frac=st)
        rpose, rpoint, rchi2, rdepth, rres = oracle.local_ba(prob, 10)
        pose, point, chi2, depth = (got[f"{tag}_{i}"] for i in range(4))
        it, trials = got[f"{tag}_it"]
        assert (it, trials) == (rres["iterations"], rres["trials"]), f"{name} {tag}: LM path"
        assert _rmse(pose[:, :3], rpose[:, :3]) < 1e-6
        q = np.where((np.sum(pose[:, 3:] * rpose[:, 3:], axis=1) < 0)[:, None], -pose[:, 3:], pose[:, 3:])
        assert _rmse(q, rpose[:, 3:]) < 1e-6
        assert _rmse(point, rpoint) < 1e-6
        assert np.array_equal(depth, rdepth)
        if st == 0.0:
            assert np.allclose(chi2, rchi2, rtol=1e-9, atol=1e-12)
        else:
            assert np.allclose(chi2, rchi2, rtol=1e-6, atol=1e-3)


_ENVS = {"rows": {"ORBGPU_BA_CHOL": "rows"}, "unit6": {"ORBGPU_BA_FAST_UNIT": "0"}}


def _variant_case_params():
    import ba_cases
    return [pytest.param(v, c, id=f"{v}-{c}") for v in _WITH_CASES for c in ba_cases.VARIANT_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("name,case_name", _variant_case_params())
def test_ba_variant_case_against_oracle(tmp_path, oracle, name, case_name):
    import ba_cases
    got = _solve(tmp_path, name, _ENVS[name])
    case = ba_cases.get(case_name)
    prob = ba_cases.build(case)
    ref = ba_cases.solve_oracle(oracle, case, prob)
    assert ba_cases.path_string(ref[5]) == case.path
    r = got[f"case_{case_name}_res"]
    f = got[f"case_{case_name}_f"]
    res = {"iterations": int(r[0]), "trials": int(r[1]), "terminated": int(r[2]), "stopped": int(r[3]),
           "initial_chi2": float(f[0]), "final_chi2": float(f[1]), "lambda": float(f[2])}
    dev = tuple(got[f"case_{case_name}_{i}"] for i in range(4)) + (res,)
    ba_cases.assert_matches_oracle(case, prob, dev, ref, tag=f"{name}: ")
