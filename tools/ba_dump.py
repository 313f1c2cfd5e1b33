"""Solve the C5 problem (mono and 50 % stereo) once and save poses / points / summary to an .npz:
    tools/ba_dump.py OUT.npz [CASE,CASE,...]
With a second argument, the named cases of tests/ba_cases.py (problems whose LM loop rejects trials) are solved
too, on one handle, and saved as case_<name>_0..3 (pose, point, chi2, depth), case_<name>_res (iterations,
trials, terminated, stopped) and case_<name>_f (initial chi2, final chi2, lambda).
Run under different ORBGPU_BA_* switches and compare the files (tools/ab_w.sh)."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from conftest import load_package  # noqa: E402

pkg = load_package()
from orbslam3_amd import synth  # noqa: E402

out = {}
for st in (0.0, 0.5):
    prob = synth.local_ba_problem(stereo_frac=st)
    res = pkg.LocalBA().optimize(prob, 10)
    for i, a in enumerate(res[:4]):
        out[f"s{int(st * 10)}_{i}"] = np.asarray(a)
    out[f"s{int(st * 10)}_it"] = np.array([res[4]["iterations"], res[4]["trials"]])
if len(sys.argv) > 2:
    import ba_cases  # noqa: E402
    solver = pkg.LocalBA()
    for name in sys.argv[2].split(","):
        case = ba_cases.get(name)
        res = solver.optimize(ba_cases.build(case), case.iterations, user_lambda_init=case.user_lambda_init)
        for i, a in enumerate(res[:4]):
            out[f"case_{name}_{i}"] = np.asarray(a)
        out[f"case_{name}_res"] = np.array([res[4][k] for k in ("iterations", "trials", "terminated", "stopped")])
        out[f"case_{name}_f"] = np.array([res[4][k] for k in ("initial_chi2", "final_chi2", "lambda")])
np.savez(sys.argv[1], **out)
