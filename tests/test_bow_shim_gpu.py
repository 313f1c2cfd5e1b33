"""ORBmatcher::SearchByBoW of the C++ drop-in (include/orbgpu_matcher.hpp) driven against the real
liborbgpu.so on the GPU (tests/native/bow_shim_gpu.cpp, built by `make shims`, linking only liborbgpu): the
mock object graph is built from the 300-point scene and vpMapPointMatches is compared with the matches the
Python restatement (tests/bow_search_ref.py) expects, with and without the orientation check."""
from __future__ import annotations

import numpy as np
import pytest

import bow_search_ref as ref
from test_shims_gpu import _run, shim_binary


def write_bow_scene(kf, fr, usable, path):
    """The scene file of bow_shim_gpu (layout in its header comment)."""
    exp = [ref.search_by_bow_kf(kf, fr, usable, 0.7, ori) for ori in (False, True)]
    with open(path, "wb") as f:
        np.array([0x426f5753, kf.N, fr.N, len(kf.fv_node), len(fr.fv_node), len(kf.fv_index), len(fr.fv_index)],
                 np.int32).tofile(f)
        kf.mvKeysUn.tofile(f)
        kf.mDescriptors.tofile(f)
        np.ascontiguousarray(usable, np.uint8).tofile(f)
        for a in (kf.fv_node, kf.fv_offset, kf.fv_index):
            a.tofile(f)
        fr.mvKeysUn.tofile(f)
        fr.mDescriptors.tofile(f)
        for a in (fr.fv_node, fr.fv_offset, fr.fv_index):
            a.tofile(f)
        for n, m in exp:
            m.astype(np.int32).tofile(f)
            np.array([n], np.int32).tofile(f)
    return exp


@pytest.mark.gpu
def test_bow_shim_on_device(pkg, synth, tmp_path):
    scene = [pkg.KeyFrame(**k) for k in synth.keyframe_scene(n_kf=2, n_points=300, seed=201, mappoint_frac=0.8,
                                                            clutter=60)]
    path = tmp_path / "bow_scene.bin"
    exp = write_bow_scene(scene[0], scene[1], scene[0].has_mappoint, path)
    assert exp[0][0] > exp[1][0] >= 20  # the orientation check removes matches on this scene
    r = _run(shim_binary("bow_shim_gpu"), path)
    assert r.returncode == 0 and "OK bow_shim_gpu" in r.stdout, r.stdout + r.stderr
