"""Device time of orb_sim3_ransac_device for 1, 3 and 6 loop-closing candidates of 200 correspondences and 300
hypotheses each, on the scene generator of tests/sim3_scenes.py.  HIP events around `reps`
back-to-back calls after a warm-up call, repeated `rounds` times; the median round is reported with the fastest and
the slowest beside it.  A figure holds a call's host enqueue, the stream-ordered scratch allocation and the two
kernels (the problems travel as kernel arguments: there is no upload), and the Python entry's six zero-filled
output tensors per problem -- six small fill kernels each, which is why the figure grows with the problems.

    python tools/sim3_time.py [reps] [rounds]
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
import sim3_scenes as scenes  # noqa: E402


def device_problem(seed, n=200, n_hyp=300):
    sc = scenes.random_problem(n, n_hyp, False, 20, seed)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return pkg.Sim3Problem(up(sc["x3dc1"]), up(sc["x3dc2"]), up(sc["max_err1"]), up(sc["max_err2"]), sc["cam1"], sc["cam2"],
                           False, 20, up(sc["samples"]))


def run(n_problems, reps, rounds):
    solver = pkg.Sim3Solver([device_problem(1 + k) for k in range(n_problems)])
    out = solver.run()
    torch.cuda.synchronize()
    winners = [int(r["winner"].item()) for r in out]
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            solver.run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / reps * 1000)
    print(f"{n_problems} problem(s) x 200 correspondences x 300 hypotheses: median {statistics.median(times):.1f} us per call "
          f"(min {min(times):.1f}, max {max(times):.1f}; {rounds} rounds of events around {reps} calls; winners {winners})",
          flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    for k in (1, 3, 6):
        run(k, reps, rounds)
