"""CPU tests of the Fuse plumbing that needs no GPU: the C++ drop-in's Fuse (single keyframe and batched)
on a mock object graph against a scalar ABI test double (tests/native/fuse_shim_check.cpp), the existing
mocks still compiling against the extended header, and the new entry points' host-side argument
rejection."""
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


def test_fuse_shim_on_mock_objects():
    """include/orbgpu_matcher.hpp Fuse: step 7's rules, the apply-time skip tests, the batched overload equal
    to the sequence of single calls where a survivor's descriptor changed, and the injected ORB_ERR_* paths."""
    exe = _compile(ROOT / "tests" / "native" / "fuse_shim_check.cpp", BUILD / "fuse_shim_check")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK fuse_shim_check" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", ["matcher_shim_check", "bow_shim_check"])
def test_existing_mocks_still_compile(name):
    """The earlier mocks have none of the Fuse accessors and no orb_fuse double: they must keep compiling
    and linking against the extended header (template members are instantiated lazily)."""
    exe = _compile(ROOT / "tests" / "native" / f"{name}.cpp", BUILD / f"{name}_fuse")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and f"OK {name}" in r.stdout, r.stdout + r.stderr


def test_fuse_entries_reject_bad_arguments(pkg):
    """No device work: NULL handles, views and point sets give ORB_ERR_ARG."""
    from orbslam3_amd import _lib
    lib = _lib.load()
    assert lib.orb_fuse(None, None, 1, None, None, 3.0, None, None) == _lib.ORB_ERR_ARG
    assert lib.orb_fuse_device(None, None, 1, None, None, 3.0, None, None, None) == _lib.ORB_ERR_ARG
    assert {"orb_fuse", "orb_fuse_device"} <= set(_lib.header_symbols()) & set(_lib.PROTOTYPES)
