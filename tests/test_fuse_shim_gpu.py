"""ORBmatcher::Fuse of the C++ drop-in (include/orbgpu_matcher.hpp) driven against the real liborbgpu.so on
the GPU (tests/native/fuse_shim_gpu.cpp, built by `make shims`, linking only liborbgpu): the mock object graph
is built from the main Fuse scene's first keyframe, and the return value and the graph after step 7 are
compared with what the best_idx of the Python restatement (tests/fuse_ref.py) gives."""
from __future__ import annotations

import numpy as np
import pytest

import fuse_ref as ref
import fuse_scenes
from test_shims_gpu import _run, shim_binary


def write_fuse_scene(kf, pts, state, holder, path):
    """The scene file of fuse_shim_gpu (layout in its header comment).  Returns the expected best_idx."""
    kf.fuse_view()
    best = ref.fuse_search([kf], pts, 3.0, (state != 0).astype(np.uint8))[0][0]
    geom = np.concatenate([kf.Tcw.reshape(-1), kf.Ow, [kf.fx, kf.fy, kf.cx, kf.cy, kf.mbf, kf.mnMinX, kf.mnMaxX,
                                                        kf.mnMinY, kf.mnMaxY, kf.mfGridElementWidthInv,
                                                        kf.mfGridElementHeightInv, kf.mfLogScaleFactor]]).astype(np.float32)
    assert len(geom) == 27
    with open(path, "wb") as f:
        np.array([0x46757365, kf.N, pts.n, len(kf.mvScaleFactors)], np.int32).tofile(f)
        for a in (geom, kf.mvScaleFactors, kf.mvInvLevelSigma2, kf.mvKeysUn, kf.mDescriptors, kf.mvuRight,
                  holder.astype(np.uint8), pts.pos, pts.normal, pts.min_dist, pts.max_dist, pts.desc,
                  state.astype(np.uint8), best.astype(np.int32)):
            np.ascontiguousarray(a).tofile(f)
    return best


@pytest.mark.gpu
def test_fuse_shim_on_device(pkg, tmp_path):
    sc = fuse_scenes.make_scene(n_kfs=3, n_points=300, seed=0)
    kf, pts = sc["kfs"][0], sc["points"]
    rng = np.random.default_rng(7)
    state = np.where(sc["skip"][0] != 0, rng.integers(1, 4, pts.n), 0)  # NULL / isBad / already in the keyframe
    holder = rng.choice(4, size=kf.N, p=[0.4, 0.25, 0.25, 0.1])
    path = tmp_path / "fuse_scene.bin"
    best = write_fuse_scene(kf, pts, state, holder, path)
    fused = best[best >= 0]
    # every branch of step 7 is reached: free keypoints, map points with fewer and with more observations, bad ones
    assert len(fused) >= 60 and all((holder[fused] == k).any() for k in range(4))
    assert all((state == k).any() for k in range(4))
    r = _run(shim_binary("fuse_shim_gpu"), path)
    assert r.returncode == 0 and "OK fuse_shim_gpu" in r.stdout, r.stdout + r.stderr
