"""ORBmatcher::CreateNewMapPoints of the C++ drop-in (include/orbgpu_matcher.hpp).  On the CPU: the mock-graph
check of step 6 against ABI test doubles (tests/native/newpoints_shim_check.cpp).  On the GPU: the member
driven against the real liborbgpu.so (tests/native/newpoints_shim_gpu.cpp, built by `make shims`, linking only
liborbgpu) on the random scene of tests/newpoints_scenes.py given descriptors and FeatureVectors, so that the
real batched search finds the matches; the records and the graph after step 6 are compared with what the
Python entries (SearchForTriangulationMany, CreateNewMapPoints) give for the same keyframes."""
from __future__ import annotations

import pathlib
import subprocess

import numpy as np
import pytest

import newpoints_scenes as scenes
from test_shims_gpu import _run, shim_binary

ROOT = pathlib.Path(__file__).resolve().parents[1]
BUILD = ROOT / "build" / "tests"


def test_newpoints_shim_on_mock_objects():
    BUILD.mkdir(parents=True, exist_ok=True)
    exe = BUILD / "newpoints_shim_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I" + str(ROOT / "include"), "-Wall",
                    "-Werror", str(ROOT / "tests" / "native" / "newpoints_shim_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK newpoints_shim_check" in r.stdout, r.stdout + r.stderr


def searchable_scene(pkg):
    """The random scene with descriptors and FeatureVectors under which the search finds (about) its synthetic
    matches: a matched pair shares a descriptor up to 3 bits and a node; everything else is random."""
    kf1, kf2s, m12, prm = scenes.random_scene()
    rng = np.random.default_rng(11)

    def with_features(kf, desc, node_of):
        fv = {}
        for j, node in enumerate(node_of):
            fv.setdefault(int(node), []).append(j)
        return pkg.KeyFrame(kf.mvKeysUn, desc, kf.Tcw, (kf.fx, kf.fy, kf.cx, kf.cy), kf.mvScaleFactors, kf.mvLevelSigma2,
                            u_right=kf.mvuRight, feat_vec=fv, Ow=kf.Ow, mb=kf.mb, mbf=kf.mbf, depth=kf.mvDepth)

    d1 = rng.integers(0, 256, (kf1.N, 32), dtype=np.uint8)
    # two idx1 sharing one idx2: keypoint b, unmatched in the synthetic scene, becomes a copy of keypoint a (whose
    # match in neighbour 0 triangulates) 0.3 px to the right with a's descriptor, so the search gives both a's idx2
    truth = scenes.random_truth()["truth"]
    a = next(i for i in range(kf1.N) if truth[0][i]["status"] == scenes.NP_OK)
    b = next(i for i in range(kf1.N) if (m12[:, i] < 0).all())
    kf1.mvKeysUn[b] = kf1.mvKeysUn[a]
    kf1.mvKeysUn[b]["x"] += np.float32(0.3)
    kf1.mvuRight[b] = kf1.mvuRight[a] + np.float32(0.3) if kf1.mvuRight[a] >= 0 else -1.0
    kf1.mvDepth[b] = kf1.mvDepth[a]
    d1[b] = d1[a]
    d1[b, 0] ^= np.uint8(1)
    out2 = []
    for p, kf in enumerate(kf2s):
        d2 = rng.integers(0, 256, (kf.N, 32), dtype=np.uint8)
        node = np.arange(kf.N) % 4
        for i in np.flatnonzero(m12[p] >= 0):
            j = int(m12[p, i])
            d2[j] = d1[i]
            for bit in rng.integers(0, 256, 3):
                d2[j, bit // 8] ^= np.uint8(1 << (bit % 8))
            node[j] = i % 4
        out2.append(with_features(kf, d2, node))
    node1 = np.arange(kf1.N) % 4
    node1[b] = node1[a]
    return with_features(kf1, d1, node1), out2, prm


def write_scene(kf1, kf2s, prm, new, path):
    with open(path, "wb") as f:
        np.array([0x4e657750, len(kf2s), len(kf1.mvScaleFactors)], np.int32).tofile(f)
        kf1.mvScaleFactors.tofile(f)
        kf1.mvLevelSigma2.tofile(f)
        np.array([prm.th_far_points, prm.ratio_factor], np.float32).tofile(f)
        np.array([prm.inertial, prm.far_points], np.int32).tofile(f)
        for k in [kf1] + list(kf2s):
            np.array([k.N, len(k.fv_node), len(k.fv_index)], np.int32).tofile(f)
            np.concatenate([k.Tcw.reshape(-1), k.Ow, [k.mb, k.mbf, k.fx, k.fy, k.cx, k.cy]]).astype(np.float32).tofile(f)
            for a in (k.mvKeysUn, k.mDescriptors, k.mvuRight, k.mvDepth, k.fv_node, k.fv_offset, k.fv_index):
                np.ascontiguousarray(a).tofile(f)
        np.array([len(new)], np.int32).tofile(f)
        np.ascontiguousarray(new).tofile(f)


@pytest.mark.gpu
def test_newpoints_shim_on_device(pkg, tmp_path):
    kf1, kf2s, prm = searchable_scene(pkg)
    m = pkg.ORBmatcher(0.6, False)
    found = m.SearchForTriangulationMany(kf1, kf2s, False)
    m12 = np.stack([r[1] for r in found])
    cnt = np.array([r[0] for r in found], np.int32)
    out = m.CreateNewMapPoints(kf1, kf2s, m12, cnt, prm.inertial, prm.far_points, float(prm.th_far_points),
                               float(prm.ratio_factor))
    new = out["new"]
    shared = len(new) - len({(int(r["p"]), int(r["idx2"])) for r in new})
    print(f"{int(cnt.sum())} matches found, {len(new)} new points, {shared} sharing an idx2 with an earlier record")
    assert cnt.sum() >= 500 and len(new) >= 250 and shared >= 1 and len(set(new["p"].tolist())) == len(kf2s)
    path = tmp_path / "newpoints_scene.bin"
    write_scene(kf1, kf2s, prm, new, path)
    r = _run(shim_binary("newpoints_shim_gpu"), path)
    assert r.returncode == 0 and "OK newpoints_shim_gpu" in r.stdout, r.stdout + r.stderr
