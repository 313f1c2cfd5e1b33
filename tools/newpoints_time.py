"""Device time of orb_create_new_map_points_device for two shapes of LocalMapping::CreateNewMapPoints (DESIGN.md
section 4l): 10 neighbours x ~1,200 keypoints with stereo keypoints, and 30 neighbours x ~1,000 keypoints
monocular, on the synthetic scene of tests/newpoints_scenes.py.  HIP events around `reps` back-to-back calls
after one warm-up call, so a figure holds a call's host enqueue, stream-ordered scratch allocation, argument
upload, the three kernels and, from the second call on, the host's wait for the previous call's argument
upload to leave the handle's pinned slot.  Beside it, on one host core: the kernel's null-vector routine (csrc/orb_svd4.h
compiled for the host, tests/native/svd4_host.cpp) over the same jobs' matrices -- the SVD alone, not the
whole per-pair loop.

    python tools/newpoints_time.py [reps]
"""
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import conftest  # noqa: E402

pkg = conftest.load_package()
import newpoints_ref as ref  # noqa: E402
import newpoints_scenes as scenes  # noqa: E402


def device_keyframe(kf, cap):
    pad = cap - kf.N

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    k = np.concatenate([kf.mvKeysUn, kf.mvKeysUn[:1].repeat(pad)])
    extracted = (up(k.view(np.float32).reshape(1, cap, 7)), up(np.zeros((1, cap, 32), np.uint8)),
                 up(np.array([[kf.N, 0]], np.int32)))
    z = torch.zeros((1, cap + 1), dtype=torch.int32, device="cuda")
    bow = (None, None, z, z, z, torch.zeros((1, 2), dtype=torch.int32, device="cuda"))  # (not read by this call)
    ur = dp = None
    if kf.mvuRight is not None:
        ur = up(np.concatenate([kf.mvuRight, -np.ones(pad, np.float32)]).reshape(1, cap))
        dp = up(np.concatenate([kf.mvDepth, -np.ones(pad, np.float32)]).reshape(1, cap))
    return pkg.DeviceKeyFrame(extracted, bow, 0, kf.Tcw, (kf.fx, kf.fy, kf.cx, kf.cy), kf.mvScaleFactors, kf.mvLevelSigma2,
                              u_right=ur, Ow=kf.Ow, mb=kf.mb, mbf=kf.mbf, depth=dp)


def run(name, n_neighbours, n_points, cap, p_stereo, reps):
    kf1, kf2s, m12, prm = scenes.random_scene(seed=3, n_neighbours=n_neighbours, n_points=n_points, p_stereo=p_stereo)
    d1, d2 = device_keyframe(kf1, cap), [device_keyframe(k, cap) for k in kf2s]
    dm = torch.full((n_neighbours, cap), -1, dtype=torch.int32, device="cuda")
    dm[:, :kf1.N] = torch.from_numpy(m12).cuda()
    cnt = torch.from_numpy((m12 >= 0).sum(1).astype(np.int32)).cuda()
    m = pkg.ORBmatcher(0.6, False)
    out = m.CreateNewMapPointsDevice(d1, d2, dm, cnt, ratio_factor=prm.ratio_factor)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        m.CreateNewMapPointsDevice(d1, d2, dm, cnt, ratio_factor=prm.ratio_factor, out=out)
    e1.record()
    torch.cuda.synchronize()
    print(f"{name}: {n_neighbours} neighbours x {n_points} keypoints, {int((m12 >= 0).sum())} matches, "
          f"{int(out['n_new'].item())} new points, {e0.elapsed_time(e1) / reps * 1000:.1f} us per call "
          f"(events around {reps} calls)", flush=True)
    # one host core: the null vectors of (up to) 2,000 of the jobs' matrices
    jobs = [(p, i) for p in range(n_neighbours) for i in np.flatnonzero(m12[p] >= 0)][:2000]
    As = np.ascontiguousarray([ref.matrix_a32(kf1, kf2s[p], i, int(m12[p, i])) for p, i in jobs], dtype=np.float32)
    x = np.zeros((len(As), 4), np.float32)
    lib = ref.host_svd4()
    lib.svd4_null_vectors(As.ctypes.data, len(As), x.ctypes.data)
    t0 = time.perf_counter()
    for _ in range(20):
        lib.svd4_null_vectors(As.ctypes.data, len(As), x.ctypes.data)
    per = (time.perf_counter() - t0) / (20 * len(As))
    print(f"{name}: host null vector alone {per * 1e9:.0f} ns per match on one core "
          f"({per * int((m12 >= 0).sum()) * 1e6:.0f} us for this call's matches; 20 passes over {len(As)} matrices)", flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    run("stereo", 10, 1200, 2048, 0.5, reps)
    run("mono", 30, 1000, 1024, 0.0, reps)
