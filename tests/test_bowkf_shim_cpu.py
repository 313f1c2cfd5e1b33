"""CPU tests of the loop-closing BoW shims that need no GPU: the C++ drop-in's SearchByBoW(KeyFrame*, KeyFrame*,
...) with its batched form and orbgpu::LoopBowProblems on a mock object graph against sequential ABI test doubles
(tests/native/bowkf_shim_check.cpp), the scene file of the GPU program, and the existing mocks still compiling
against the extended headers."""
from __future__ import annotations

import pathlib
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
BUILD = ROOT / "build" / "tests"


def _compile(src: pathlib.Path, out: pathlib.Path):
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I" + str(ROOT / "include"), "-Wall",
                    "-Werror", str(src), "-o", str(out)], check=True)
    return out


def test_bowkf_shim_on_mock_objects():
    """The views, masks and mp_id arrays built from KeyFrame / MapPoint, vpMatches12 written back, the skipped
    window keyframes, LoopBowProblems' outputs and solver, and the injected ORB_ERR_* paths."""
    exe = _compile(ROOT / "tests" / "native" / "bowkf_shim_check.cpp", BUILD / "bowkf_shim_check")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK bowkf_shim_check" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", ["bow_shim_check", "sim3_shim_check", "sim3proj_shim_check"])
def test_existing_mocks_still_compile(name):
    """The earlier mocks have no IsBad(KeyFrame*) and no double of the new entries: they must keep compiling and
    linking against the extended headers (the new members are instantiated lazily)."""
    exe = _compile(ROOT / "tests" / "native" / f"{name}.cpp", BUILD / f"{name}_bowkf")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and f"OK {name}" in r.stdout, r.stdout + r.stderr


def test_gpu_program_scene_file(tmp_path):
    """The scene the GPU program reads contains what it checks: every candidate has a problem, the gather drops
    slots (GetIndexInKeyFrame < 0), and the file is written whole."""
    from test_bowkf_shim_gpu import write_scene
    path = tmp_path / "bowkf.bin"
    write_scene(path)
    assert path.stat().st_size > 50000
