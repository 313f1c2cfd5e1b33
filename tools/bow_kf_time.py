"""Device time of loop closing's BoW head on 33 pairs: 3 candidates x 11 window keyframes
against one current keyframe, keyframes of synth.keyframe_scene (1,500 points plus clutter, 80 % with a map point).
HIP events around one call, 10 warm calls, the median of `runs` with the fastest and slowest beside it:

  - orb_search_by_bow_kf_device, the 33 pairs in one call, and the same pairs as 33 single-pair calls;
  - orb_loop_bow_problems_device on that batch's matches;
  - orb_search_by_bow_device (the KeyFrame / Frame overload, the same node walk) on the same shapes, for comparison.

A figure holds the call's host enqueue, its argument upload and stream-ordered scratch, the fills and the kernels.

    python tools/bow_kf_time.py [runs]
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
from orbslam3_amd import synth  # noqa: E402
from bow_search_scenes import device_keyframe  # noqa: E402

N_CAND, N_WIN, CAP = 3, 11, 2048


def timed(fn, runs):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1000)
    return f"median {statistics.median(t):.1f} us (min {min(t):.1f}, max {max(t):.1f}; {runs} runs)"


def main(runs):
    kfs = [pkg.KeyFrame(**k) for k in synth.keyframe_scene(n_kf=1 + N_WIN, n_points=1500, seed=201, mappoint_frac=0.8,
                                                           clutter=250)]
    dk = [device_keyframe(pkg, k, CAP) for k in kfs]
    window = dk[1:] * N_CAND
    n_pairs = len(window)
    matcher = pkg.ORBmatcher(0.9, True)  # loop closing's matcherBoW(0.9, true)
    out = matcher.SearchByBoWKFDevice(dk[0], window)
    shared = [len(set(kfs[0].mFeatVec) & set(k.mFeatVec)) for k in kfs[1:]]
    print(f"{n_pairs} pairs; features {[k.N for k in kfs]}; nodes {[len(k.fv_node) for k in kfs]}; shared nodes with the "
          f"current keyframe {shared}; matches {out[1].cpu().tolist()[:N_WIN]}", flush=True)
    print("SearchByBoWKFDevice, one call of 33 pairs:   ", timed(lambda: matcher.SearchByBoWKFDevice(dk[0], window, out=out), runs),
          flush=True)
    singles = [(torch.empty((1, CAP), dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"))
               for _ in range(n_pairs)]

    def one_by_one():
        for k, o in zip(window, singles):
            matcher.SearchByBoWKFDevice(dk[0], [k], out=o)

    print("SearchByBoWKFDevice, 33 single-pair calls:   ", timed(one_by_one, runs), flush=True)
    print("SearchByBoWKFDevice, one single-pair call:   ",
          timed(lambda: matcher.SearchByBoWKFDevice(dk[0], [window[0]], out=singles[0]), runs), flush=True)

    # the merge and the gather on that batch: every feature with a map point gets a pool point
    rng = np.random.default_rng(1)
    n_points = 20000
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def lb(k, d):
        mp = np.full(CAP, -1, np.int32)
        mp[:k.N] = np.where(k.has_mappoint != 0, rng.integers(0, n_points, k.N), -1)
        return pkg.LoopBowKeyFrame(up(mp), d._keep[0][0], k.mvLevelSigma2)

    l1 = lb(kfs[0], dk[0])
    l2 = [lb(k, d) for k, d in zip(kfs[1:], dk[1:])] * N_CAND
    xyz = up(rng.uniform(-4, 4, (n_points, 3)).astype(np.float32))
    group = np.arange(N_CAND + 1) * N_WIN
    Tcw2 = np.stack([k.Tcw for k in kfs[1:1 + N_CAND]])
    run = lambda: pkg.loop_bow_problems(matcher, l1, kfs[0].Tcw, l2, group, Tcw2, xyz, out[0])  # noqa: E731
    res = run()
    print(f"loop_bow_problems: num_bow {res['num_bow'].cpu().tolist()}, n {res['n'].cpu().tolist()}", flush=True)
    print("loop_bow_problems (device), 3 x 11 pairs:    ", timed(run, runs), flush=True)

    # the KeyFrame / Frame overload on the same shapes: 33 keyframes against the current keyframe as the frame
    fout = matcher.SearchByBoWDevice(window, dk[0])
    print("SearchByBoWDevice (Frame form), one call of 33:", timed(lambda: matcher.SearchByBoWDevice(window, dk[0], out=fout), runs),
          flush=True)
    print("SearchByBoWDevice (Frame form), one single call:",
          timed(lambda: matcher.SearchByBoWDevice([window[0]], dk[0], out=(fout[0][:1], fout[1][:1])), runs), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 100)
