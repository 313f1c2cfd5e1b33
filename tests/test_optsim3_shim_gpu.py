"""orbgpu::OptimizeSim3<S> of the C++ drop-in (include/orbgpu_optimizer.hpp).  On the CPU: the mock-graph check
against a scripted ABI double (tests/native/optsim3_shim_check.cpp).  On the GPU: the shim driven against the real
liborbgpu.so (tests/native/optsim3_shim_gpu.cpp, built by `make shims`) on a two-keyframe graph; what it must return
comes from the library's Python entry for the same gathered graph, itself held to the restatement."""
from __future__ import annotations

import pathlib
import subprocess

import numpy as np
import pytest

import optsim3_ref as ref
import optsim3_scenes as scenes
from test_shims_gpu import _run, shim_binary

ROOT = pathlib.Path(__file__).resolve().parents[1]
BUILD = ROOT / "build" / "tests"
f32 = np.float32


def test_optsim3_shim_on_mock_objects():
    BUILD.mkdir(parents=True, exist_ok=True)
    exe = BUILD / "optsim3_shim_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I" + str(ROOT / "include"), "-Wall",
                    "-Werror", str(ROOT / "tests" / "native" / "optsim3_shim_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK optsim3_shim_check" in r.stdout, r.stdout + r.stderr


def camera_points(R, t, X):
    """Rcw X + tcw in float32, summed as the shim sums it."""
    R, t, X = R.astype(f32), t.astype(f32), X.astype(f32)
    return np.stack([((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)], 1)


def graph(seed=11, n=70):
    """Two keyframes over the pairs of a scene with wrong pairs; rows 5.. carry one skip rule each, rows 40, 44, 48
    have no keypoint in keyframe 2 (the i2 < 0 rule)."""
    p = scenes.make(n, seed, fix_scale=False, wrong=range(4, n, 11), start=(0.02, -0.03, 0.02, 0.03, -0.02, 0.02, 0.02))
    rng = np.random.default_rng(seed)
    R1, R2 = ref.quat_to_rot(np.array([0.1, -0.2, 0.05, 0.97])), ref.quat_to_rot(np.array([-0.15, 0.1, 0.2, 0.96]))
    t1, t2 = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    table = scenes.inv_sigma2(np.arange(8))
    octave = lambda v: np.abs(table[None] - np.asarray(v, f32)[:, None]).argmin(1)  # noqa: E731
    flags = np.full(n, 1 | 2 | 16, np.int32)
    flags[5] &= ~1          # no match
    flags[6] &= ~2          # no pMP1
    flags[7] |= 4           # bad pMP1
    flags[8] |= 8           # bad pMP2
    flags[[40, 44, 48]] &= ~16
    g = {"R1": R1.astype(f32), "t1": t1.astype(f32), "R2": R2.astype(f32), "t2": t2.astype(f32), "cam": np.array(scenes.CAM, f32),
         "table": table, "pos1": ((p["p1c"] - t1) @ R1).astype(f32), "pos2": ((p["p2c"] - t2) @ R2).astype(f32),
         "kp1": np.column_stack([p["obs1"], octave(p["inv_sigma2_1"])]).astype(f32),
         "kp2": np.column_stack([p["obs2"], octave(p["inv_sigma2_2"])]).astype(f32), "flags": flags, "s12": p["s12"]}
    g["pos2"][9] = ((np.array([0.1, 0.1, -2.0]) - t2) @ R2).astype(f32)     # behind camera 2
    return g


def expected(pkg, g, fix, all_points, th2):
    """The gather of src/Optimizer.cc:4254-4407 in numpy, then the library's Python entry."""
    fl = g["flags"]
    P1, P2 = camera_points(g["R1"], g["t1"], g["pos1"]), camera_points(g["R2"], g["t2"], g["pos2"])
    rows = [i for i in range(len(fl)) if (fl[i] & 1) and (fl[i] & 2) and not (fl[i] & 12)
            and ((fl[i] & 16) or all_points) and not P2[i, 2] < 0]
    obs2 = g["kp2"][rows, :2].astype(np.float64)
    is2 = g["table"][g["kp2"][rows, 2].astype(int)].copy()
    for k, i in enumerate(rows):
        if not fl[i] & 16:
            invz = f32(1) / P2[i, 2]
            obs2[k] = [P2[i, 0] * invz, P2[i, 1] * invz]
            is2[k] = g["table"][0]
    prob = {"p1c": P1[rows].astype(np.float64), "p2c": P2[rows].astype(np.float64), "obs1": g["kp1"][rows, :2].astype(np.float64),
            "obs2": obs2, "inv_sigma2_1": g["table"][g["kp1"][rows, 2].astype(int)], "inv_sigma2_2": is2, "cam1": g["cam"],
            "cam2": g["cam"], "s12": g["s12"], "th2": th2, "fix_scale": fix}
    ex = ref.optimize_sim3(prob)
    (r,) = pkg.optimize_sim3([prob])
    assert ex["decisive"] and r["n_bad"] == ex["n_bad"] and np.abs(r["s12"] - ex["s12"]).max() <= 1e-6
    kept = (fl & 1).astype(np.uint8)
    kept[np.array(rows)[~r["inlier"]]] = 0
    early = len(rows) - r["n_bad"] < 10
    return len(rows), (0 if early else r["n_in"]), (np.asarray(g["s12"], np.float64) if early else r["s12"]), kept


@pytest.mark.gpu
def test_optsim3_shim_on_device(pkg, tmp_path):
    g = graph()
    configs = [(1, 0, 10.0), (0, 1, 10.0)]
    want = [expected(pkg, g, bool(fix), bool(allp), th2) for fix, allp, th2 in configs]
    print("gathered pairs, return value:", [(w[0], w[1]) for w in want])
    assert want[1][0] == want[0][0] + 3 and want[0][1] > 10 and want[0][0] == len(g["flags"]) - 8
    path = tmp_path / "optsim3_graph.bin"
    with open(path, "wb") as f:
        np.array([0x4f533300, len(g["flags"]), len(configs)], np.int32).tofile(f)
        for k in ("1", "2"):
            for a in (g["R" + k], g["t" + k], g["cam"], g["table"]):
                np.ascontiguousarray(a, f32).tofile(f)
        for k in ("pos1", "pos2", "kp1", "kp2"):
            np.ascontiguousarray(g[k], f32).tofile(f)
        g["flags"].tofile(f)
        np.ascontiguousarray(g["s12"], np.float64).tofile(f)
        for (fix, allp, th2), (_, ret, s12, kept) in zip(configs, want):
            np.array([fix, allp], np.int32).tofile(f)
            np.array([th2], f32).tofile(f)
            np.array([ret], np.int32).tofile(f)
            np.ascontiguousarray(s12, np.float64).tofile(f)
            kept.tofile(f)
    r = _run(shim_binary("optsim3_shim_gpu"), path)
    assert r.returncode == 0 and "OK optsim3_shim_gpu" in r.stdout, r.stdout + r.stderr
