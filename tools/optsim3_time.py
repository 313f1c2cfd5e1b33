"""Device time of orb_optimize_sim3_device for 1, 3 and 6 loop-closing candidates of 150 pairs each (DESIGN.md
section 4n), on the scene generator of tests/optsim3_scenes.py (1 px noise scaled by level, 10 % wrong pairs, so the
second stage runs its 10 iterations).  HIP events around `reps` back-to-back calls after a warm-up call, repeated
`rounds` times; the median round is reported with the fastest and the slowest beside it.  A figure holds a call's
host enqueue, the one kernel launch (the problems travel as kernel arguments: there is no upload) and the Python
entry's four zero-filled output tensors per problem -- four small fill kernels each.  The kernel alone is not timed.

    python tools/optsim3_time.py [reps] [rounds]
"""
import pathlib
import statistics
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import conftest  # noqa: E402

pkg = conftest.load_package()
import optsim3_scenes as scenes  # noqa: E402

KEYS = ("p1c", "p2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")


def device_problem(seed, n=150):
    p = scenes.make(n, seed, fix_scale=bool(seed & 1), noise=1.0, wrong=range(3, n, 10), wrong_px=20.0)
    return {**p, **{k: torch.from_numpy(np.ascontiguousarray(p[k])).cuda() for k in KEYS}}


def run(n_problems, reps, rounds):
    probs = [device_problem(1 + k) for k in range(n_problems)]
    out = pkg.optimize_sim3(probs)
    torch.cuda.synchronize()
    counts = [(int(r["n_bad"].item()), int(r["n_in"].item())) for r in out]
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            pkg.optimize_sim3(probs)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / reps * 1000)
    print(f"{n_problems} problem(s) x 150 pairs: median {statistics.median(times):.1f} us per call "
          f"(min {min(times):.1f}, max {max(times):.1f}; {rounds} rounds of events around {reps} calls; "
          f"(n_bad, n_in) {counts})", flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    for k in (1, 3, 6):
        run(k, reps, rounds)
