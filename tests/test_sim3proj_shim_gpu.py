"""The Sim3 search members of the C++ drop-in (include/orbgpu_matcher.hpp) against the real liborbgpu.so on
the GPU (tests/native/sim3proj_shim_gpu.cpp, built by `make shims`, linking only liborbgpu): the mock object
graph is built from a scene file, and the expected matches come from the Python restatement
tests/sim3_projection_ref.py."""
from __future__ import annotations

import numpy as np
import pytest

import sim3_projection_ref as ref
import sim3_projection_scenes as scenes
from test_shims_gpu import _run, shim_binary


def write_scene(path, seed=0):
    """The scene file of sim3proj_shim_gpu (layout in its header comment)."""
    sc = scenes.make_scene(seed)
    kf, P = sc["kf"], sc["points"]
    rng = np.random.default_rng(seed + 100)
    Tcw, Ow = scenes.candidate_pose(sc["T"], 1.25)
    holder = rng.choice([0, 1, 3], kf.N, p=[0.6, 0.3, 0.1]).astype(np.uint8)
    state = rng.choice([0, 2, 3], P.n, p=[0.9, 0.05, 0.05]).astype(np.uint8)
    prematch = np.full(kf.N, -2, np.int32)
    taken = np.flatnonzero(rng.random(kf.N) < 0.06)
    prematch[taken] = np.where(rng.random(len(taken)) < 0.5, -1, rng.choice(P.n, len(taken), replace=False))
    found = np.zeros(P.n, bool)
    found[prematch[prematch >= 0]] = True
    skip_claim = ((state == 2) | found).astype(np.uint8)
    taken0 = (prematch != -2).astype(np.uint8)
    r1 = ref.search_by_projection(kf, Tcw, Ow, P, 0, P.n, 5.0, 1.0, skip_claim, taken0)
    r2 = ref.search_by_projection_kfs(kf, Tcw, Ow, P, 0, P.n, 8.0, 1.5, skip_claim, taken0)
    # Fuse: the state-3 points sit in the keyframe's first free slots, as the program places them
    free = np.flatnonzero(holder == 0)
    in_kf = np.flatnonzero(state == 3)[:len(free)]
    skip_fuse = (state == 2)
    skip_fuse[in_kf] = True
    rf = ref.fuse(kf, Tcw, Ow, P, 0, P.n, 4.0, skip_fuse.astype(np.uint8))
    assert r1["nmatches"] >= 40 and r2["nmatches"] > r1["nmatches"] and rf["nmatches"] >= 60
    assert ref.displacement(r2)[0].sum() >= 0.1 * r2["nmatches"]
    with open(path, "wb") as f:
        np.array([0x53335072, kf.N, P.n, len(kf.mvScaleFactors)], np.int32).tofile(f)
        np.concatenate([Tcw.reshape(-1), Ow, [kf.fx, kf.fy, kf.cx, kf.cy, kf.mnMinX, kf.mnMaxX, kf.mnMinY, kf.mnMaxY,
                                              kf.mfGridElementWidthInv, kf.mfGridElementHeightInv,
                                              kf.mfLogScaleFactor]]).astype(np.float32).tofile(f)
        kf.mvScaleFactors.tofile(f)
        kf.mvKeysUn.tofile(f)
        kf.mDescriptors.tofile(f)
        holder.tofile(f)
        prematch.tofile(f)
        for a in (P.pos, P.normal, P.min_dist, P.max_dist, P.desc, state):
            a.tofile(f)
        r1["matched"].tofile(f)
        np.array([r1["nmatches"]], np.int32).tofile(f)
        r2["matched"].tofile(f)
        np.array([r2["nmatches"]], np.int32).tofile(f)
        rf["best_idx"].tofile(f)


@pytest.mark.gpu
def test_sim3proj_shim_on_device(pkg, tmp_path):
    """Both SearchByProjection forms (vpMatched / vpMatchedKF, pre-filled entries, bad and already-found points),
    the batched form, Fuse with step 7 against the expected best_idx, and an ORB_ERR_ARG from the library."""
    path = tmp_path / "sim3proj.bin"
    write_scene(path)
    r = _run(shim_binary("sim3proj_shim_gpu"), path)
    assert r.returncode == 0 and "OK sim3proj_shim_gpu" in r.stdout, r.stdout + r.stderr
