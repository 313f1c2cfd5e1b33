"""orbgpu::Sim3Solver<A> of the C++ drop-in (include/orbgpu_sim3.hpp).  On the CPU: the mock-graph check against an
ABI test double (tests/native/sim3_shim_check.cpp).  On the GPU: the class driven against the real liborbgpu.so
(tests/native/sim3_shim_gpu.cpp, built by `make shims`, linking only liborbgpu) on a two-keyframe graph with a
scripted RandomInt; what the reference's caller loop must return comes from the library's Python entry for the
same draws and the replay of tests/sim3_ref.py."""
from __future__ import annotations

import pathlib
import subprocess

import numpy as np
import pytest

import sim3_ref as ref
import sim3_scenes as scenes
from test_shims_gpu import _run, shim_binary

ROOT = pathlib.Path(__file__).resolve().parents[1]
BUILD = ROOT / "build" / "tests"
f32 = np.float32


def test_sim3_shim_on_mock_objects():
    BUILD.mkdir(parents=True, exist_ok=True)
    exe = BUILD / "sim3_shim_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I" + str(ROOT / "include"), "-Wall",
                    "-Werror", str(ROOT / "tests" / "native" / "sim3_shim_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK sim3_shim_check" in r.stdout, r.stdout + r.stderr


def camera_points(R, t, X):
    """Rcw X + tcw in float32, summed as the shim sums it."""
    R, t, X = R.astype(f32), t.astype(f32), X.astype(f32)
    return np.stack([((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2]) + t[r] for r in range(3)], 1)


def graph(seed=4, n=60):
    """World points seen by two keyframes: keyframe 2's map points are keyframe 1's moved by a Sim3 (the drift a
    loop closure corrects), 55 % of them gross outliers, so that the loop needs more than one chunk."""
    sc = scenes.random_problem(n, 1, False, 15, seed, outliers=0.55)
    rng = np.random.default_rng(seed)
    R1, R2 = scenes.rodrigues(rng.normal(size=3), 0.2), scenes.rodrigues(rng.normal(size=3), 0.4)
    t1, t2 = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    g = {"R1": R1.astype(f32), "t1": t1.astype(f32), "R2": R2.astype(f32), "t2": t2.astype(f32),
         "pos1": ((sc["x3dc1"].astype(float) - t1) @ R1).astype(f32), "pos2": ((sc["x3dc2"].astype(float) - t2) @ R2).astype(f32),
         "oct1": rng.integers(0, 8, n).astype(np.int32), "oct2": rng.integers(0, 8, n).astype(np.int32),
         "sigma2": (f32(1.2) ** (2 * np.arange(8))).astype(f32), "cam1": scenes.CAM_EUROC, "cam2": scenes.CAM_OTHER,
         "script": rng.integers(0, 1 << 20, 3 * 600).astype(np.int32)}
    g["x3dc1"], g["x3dc2"] = camera_points(g["R1"], g["t1"], g["pos1"]), camera_points(g["R2"], g["t2"], g["pos2"])
    return g


def expected(pkg, g, fix_scale, min_inliers, max_iterations, pos):
    """What `while (!bConverge && !bNoMore) iterate(20, ...)` returns, and the script position after the draws."""
    n = len(g["pos1"])
    H = pkg.ransac_max_its(n, 0.99, min_inliers, max_iterations)
    script = g["script"]

    def random_int(lo, hi):
        nonlocal pos
        v = lo + int(script[pos % len(script)]) % (hi - lo + 1)
        pos += 1
        return v

    samples = pkg.draw_samples(n, H, random_int)
    assert np.array_equal(samples, ref.draw_samples(n, H, iter_script(script, pos - 3 * H)))
    prob = {"x3dc1": g["x3dc1"], "x3dc2": g["x3dc2"], "max_err1": ref.max_err(g["sigma2"][g["oct1"]]),
            "max_err2": ref.max_err(g["sigma2"][g["oct2"]]), "cam1": g["cam1"], "cam2": g["cam2"], "fix_scale": fix_scale,
            "min_inliers": min_inliers, "samples": samples}
    sc = scenes.with_reference(prob)      # the scene's own conditions: the counts below are not borderline
    (r,) = pkg.Sim3Solver(pkg.Sim3Problem(prob["x3dc1"], prob["x3dc2"], prob["max_err1"], prob["max_err2"], prob["cam1"],
                                          prob["cam2"], fix_scale, min_inliers, samples)).run(hyp_mask=True)
    assert ((r["hyp_inliers"] >= sc["lo"]) & (r["hyp_inliers"] <= sc["lo"] + sc["und"])).all()
    replay = ref.Replay(r["hyp_inliers"], n, min_inliers, H)
    while True:
        step = replay.iterate(20, with_converge=True)
        if step["converge"] or step["no_more"]:
            break
    T = np.eye(4, dtype=f32)
    if step["hyp"] >= 0:
        T[:3] = r["hyp_t12"][step["hyp"]].reshape(3, 4)
    bits = np.unpackbits(r["hyp_mask"].view(np.uint8), axis=-1, bitorder="little")[:, :n]
    inl = bits[step["hyp"]] if step["converge"] else np.zeros(n, np.uint8)
    head = np.array([H, step["hyp"] if step["converge"] else -1, step["n_inliers"], replay.iterations], np.int32)
    return (head, T, inl.astype(np.uint8)), pos


def iter_script(script, pos):
    def random_int(lo, hi):
        nonlocal pos
        v = lo + int(script[pos % len(script)]) % (hi - lo + 1)
        pos += 1
        return v
    return random_int


@pytest.mark.gpu
def test_sim3_shim_on_device(pkg, tmp_path):
    g = graph()
    configs = [(False, 15, 300), (True, 12, 200)]
    pos, want = 0, []
    for fix, m, its in configs:
        w, pos = expected(pkg, g, fix, m, its, pos)
        want.append(w)
    print("expected (max its, hypothesis, inliers, iterations):", [w[0].tolist() for w in want])
    assert want[0][0][3] > 20 and want[0][0][1] >= 0        # more than one chunk, then a convergence
    path = tmp_path / "sim3_graph.bin"
    with open(path, "wb") as f:
        np.array([0x53696d33, len(g["pos1"]), len(g["script"]), 2], np.int32).tofile(f)
        for k in ("1", "2"):
            for a in (g["R" + k], g["t" + k], np.array(g["cam" + k], f32), g["sigma2"]):
                np.ascontiguousarray(a, f32).tofile(f)
        for k in ("1", "2"):
            g["oct" + k].tofile(f)
            np.ascontiguousarray(g["pos" + k], f32).tofile(f)
        g["script"].tofile(f)
        for (fix, m, its), (head, T, inl) in zip(configs, want):
            np.array([fix, m, its], np.int32).tofile(f)
            head.tofile(f)
            T.tofile(f)
            inl.tofile(f)
    r = _run(shim_binary("sim3_shim_gpu"), path)
    assert r.returncode == 0 and "OK sim3_shim_gpu" in r.stdout, r.stdout + r.stderr
