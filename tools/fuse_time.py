"""Device time of orb_fuse_device for the two shapes of LocalMapping::SearchInNeighbors:
forward, 20 target keyframes x 1,500 points, and reverse, 1 keyframe x 30,000 points, on the synthetic scenes
of tests/fuse_scenes.py.  HIP events around `reps` back-to-back calls after one warm-up call, so a figure
holds a call's host enqueue, stream-ordered scratch allocation, argument upload and both kernels.

    python tools/fuse_time.py [reps]
"""
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import conftest  # noqa: E402

pkg = conftest.load_package()
import fuse_scenes  # noqa: E402


def device_frame(kf, cap):
    pad = cap - kf.N
    k = np.concatenate([kf.mvKeysUn, kf.mvKeysUn[:1].repeat(pad)])
    d = np.concatenate([kf.mDescriptors, np.zeros((pad, 32), np.uint8)])
    ur = np.concatenate([kf.mvuRight, -np.ones(pad, np.float32)])

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    return pkg.DeviceFrame(up(k.view(np.float32).reshape(1, cap, 7)), up(d.reshape(1, cap, 32)),
                           up(np.array([[kf.N, 0]], np.int32)), 0, kf.Tcw, (kf.fx, kf.fy, kf.cx, kf.cy), kf.mvScaleFactors,
                           kf.mvScaleFactors * kf.mvScaleFactors, fuse_scenes.WIDTH, fuse_scenes.HEIGHT, bf=kf.mbf,
                           u_right=up(ur.reshape(1, cap)))


def run(name, n_kfs, n_points, cap, p_obs, reps):
    sc = fuse_scenes.make_scene(n_kfs=n_kfs, n_points=n_points, seed=3, n_clutter=300, p_obs=p_obs)
    kfs, pts = sc["kfs"], sc["points"]
    frames = [device_frame(k, cap) for k in kfs]
    Ow = np.stack([k.Ow for k in kfs])
    t = tuple(torch.from_numpy(a).cuda() for a in (pts.pos, pts.normal, pts.min_dist, pts.max_dist, pts.desc))
    sk = torch.from_numpy(sc["skip"]).cuda()
    m = pkg.ORBmatcher()
    out = m.FuseDevice(frames, t, 3.0, sk, Ow=Ow)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        m.FuseDevice(frames, t, 3.0, sk, Ow=Ow, out=out)
    e1.record()
    torch.cuda.synchronize()
    print(f"{name}: {n_kfs} x {n_points}, keypoints {[k.N for k in kfs][:3]}..., fused {int((out[0] >= 0).sum())}, "
          f"{e0.elapsed_time(e1) / reps * 1000:.1f} us per call (events around {reps} calls)", flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    run("forward", 20, 1500, 2048, 0.8, reps)
    run("reverse", 1, 30000, 4096, 0.1, reps)
