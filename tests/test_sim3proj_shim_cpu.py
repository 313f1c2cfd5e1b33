"""CPU tests of the Sim3 search shims that need no GPU: the C++ drop-in's SearchByProjection(KF, Scw, ...),
its vpMatchedKF overload, Fuse(KF, Scw, ...) and their batched forms on a mock object graph against a scalar
ABI test double (tests/native/sim3proj_shim_check.cpp), and the existing mocks still compiling against the
extended header."""
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


def test_sim3proj_shim_on_mock_objects():
    """skip / taken0 construction, vpMatched / vpMatchedKF, Fuse's step-7 order with the AddMapPoint-then-replace
    case, the batched forms, and the injected ORB_ERR_* paths."""
    exe = _compile(ROOT / "tests" / "native" / "sim3proj_shim_check.cpp", BUILD / "sim3proj_shim_check")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK sim3proj_shim_check" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", ["fuse_shim_check", "matcher_shim_check"])
def test_existing_mocks_still_compile(name):
    """The earlier mocks have neither Sim3Pose / MapPointSet nor an orb_sim3_projection double: they must keep
    compiling and linking against the extended header (the new members are instantiated lazily)."""
    exe = _compile(ROOT / "tests" / "native" / f"{name}.cpp", BUILD / f"{name}_sim3proj")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and f"OK {name}" in r.stdout, r.stdout + r.stderr
