"""The loop-closing BoW members of the C++ drop-ins (SearchByBoW(KeyFrame*, KeyFrame*, ...) and its batched form
in include/orbgpu_matcher.hpp, LoopBowProblems in include/orbgpu_sim3.hpp) against the real liborbgpu.so on the GPU
(tests/native/bowkf_shim_gpu.cpp, built by `make shims`, linking only liborbgpu): the mock object graph is built
from a scene file, and the expected values come from the Python restatement tests/bow_kf_ref.py."""
from __future__ import annotations

import numpy as np
import pytest

import bow_kf_ref as ref
import bow_kf_scenes as sc
from test_shims_gpu import _run, shim_binary


def mock_level_sigma2():
    """mvLevelSigma2 as the mock keyframe builds it: scale[l] = scale[l-1] * 1.2f, sigma2 = scale * scale."""
    s, out = np.float32(1.0), []
    for level in range(8):
        if level:
            s = np.float32(s * np.float32(1.2))
        out.append(np.float32(s * s))
    return np.asarray(out, np.float32)


def write_scene(path):
    """The scene file of bowkf_shim_gpu (layout in its header comment): chain_scene() with the mock's level table
    and `observed` per (keyframe, point), as a map stores it."""
    s = sc.chain_scene()
    sig = mock_level_sigma2()
    for i, k in enumerate([s["kf1"]] + s["kfs2"]):
        k["level_sigma2"] = sig
        hidden = set(range(i, 144, 9)) if i in (0, 3) else set()  # points that do not list this keyframe
        k["obs_ok"] = np.array([0 if int(m) in hidden else 1 for m in k["mp_id"]], np.uint8)
    kf1, kfs2 = s["kf1"], s["kfs2"]
    n1 = len(kf1["ok"])
    rows = [sc.expected_search(ref, kf1, k2, True) for k2 in kfs2]
    exp = sc.expected_problems(ref, s, [m for _, m in rows])
    assert all(e["n"] >= 6 for e in exp) and any(e["n"] < int((e["matched_point"] >= 0).sum()) for e in exp)
    with open(path, "wb") as f:
        np.array([0x426b6631, 1 + len(kfs2), len(exp), len(s["xyz"]), n1], np.int32).tofile(f)
        s["group"].astype(np.int32).tofile(f)
        np.concatenate([s["Tcw1"].reshape(-1), np.asarray(s["Tcw2"], np.float32).reshape(-1)]).astype(np.float32).tofile(f)
        s["xyz"].astype(np.float32).tofile(f)
        s["bad"].astype(np.uint8).tofile(f)
        for k in [kf1] + kfs2:
            fv = k["feat_vec"]
            np.array([len(k["ok"]), len(fv)], np.int32).tofile(f)
            k["keys_un"].tofile(f)
            k["descriptors"].tofile(f)
            k["mp_id"].astype(np.int32).tofile(f)
            k["obs_ok"].astype(np.uint8).tofile(f)
            for node in sorted(fv):
                np.array([node, len(fv[node])] + list(fv[node]), np.int32).tofile(f)
        np.stack([m for _, m in rows]).astype(np.int32).tofile(f)
        np.array([n for n, _ in rows], np.int32).tofile(f)
        for e in exp:
            np.array([e["num_bow"], e["n"]], np.int32).tofile(f)
            for key in ("matched_point", "matched_pair", "idx1"):
                e[key].astype(np.int32).tofile(f)
            for key in ("max_err1", "max_err2", "x3dc1", "x3dc2"):
                e[key].astype(np.float32).tofile(f)
            for key in ("bound1", "bound2"):
                e[key].astype(np.float64).tofile(f)


@pytest.mark.gpu
def test_bowkf_shim_on_device(pkg, tmp_path):
    """SearchByBoW(KF, KF) single and batched (a NULL and a bad window keyframe skipped), LoopBowProblems' vectors,
    counts and solver arrays against the restatement, the solvers run through Batch and iterate, and an
    ORB_ERR_ARG from the library."""
    path = tmp_path / "bowkf.bin"
    write_scene(path)
    r = _run(shim_binary("bowkf_shim_gpu"), path)
    assert r.returncode == 0 and "OK bowkf_shim_gpu" in r.stdout, r.stdout + r.stderr
