"""CPU tests of the SearchByBoW plumbing that needs no GPU: the C++ drop-in's SearchByBoW on a mock object
graph against an ABI test double (tests/native/bow_shim_check.cpp), the existing matcher mock still
compiling against the extended header (template members are instantiated lazily), and the new entry
points' host-side argument rejection."""
from __future__ import annotations

import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]
BUILD = ROOT / "build" / "tests"


def _compile(src: pathlib.Path, out: pathlib.Path):
    BUILD.mkdir(parents=True, exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-I" + str(ROOT / "include"), "-Wall",
                    "-Werror", str(src), "-o", str(out)], check=True)
    return out


def test_bow_shim_on_mock_objects():
    """include/orbgpu_matcher.hpp SearchByBoW: the keyframe / frame views and usable flags handed across
    the ABI, the NULL fill, the write-back and the injected ORB_ERR_* paths."""
    exe = _compile(ROOT / "tests" / "native" / "bow_shim_check.cpp", BUILD / "bow_shim_check")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK bow_shim_check" in r.stdout, r.stdout + r.stderr


def test_existing_matcher_mock_still_compiles():
    """The mock of tests/native/matcher_shim_check.cpp has no FeatVec(const Frame&) and no
    orb_search_by_bow double: it must keep compiling and linking against the extended header."""
    exe = _compile(ROOT / "tests" / "native" / "matcher_shim_check.cpp", BUILD / "matcher_shim_check_bow")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "OK matcher_shim_check" in r.stdout, r.stdout + r.stderr


def test_new_entries_reject_bad_arguments(pkg):
    """No device work: NULL handles and views give ORB_ERR_ARG, the scratch size is positive and grows."""
    from orbslam3_amd import _lib
    lib = _lib.load()
    assert lib.orb_search_by_bow(None, None, None, 1, None, None, None) == _lib.ORB_ERR_ARG
    assert lib.orb_search_by_bow_device(None, None, None, 1, None, 1, None, None, None, None) == _lib.ORB_ERR_ARG
    assert lib.orb_track_reference_kf_device(None, None, None, None, None, None, None, None, None, 0, None,
                                             None) == _lib.ORB_ERR_ARG
    assert lib.orb_track_reference_kf_scratch_bytes(0) == 0
    a, b = lib.orb_track_reference_kf_scratch_bytes(1000), lib.orb_track_reference_kf_scratch_bytes(2000)
    assert 8 * 1000 <= a < b
    from orbslam3_amd import tracking
    assert (tracking.ORB_TRACK_REF_FAIL_BOW, tracking.ORB_TRACK_REF_FAIL_MAP) == (8, 16)
    assert not {tracking.ORB_TRACK_REF_FAIL_BOW, tracking.ORB_TRACK_REF_FAIL_MAP} & {
        tracking.ORB_TRACK_RETRIED, tracking.ORB_TRACK_FAIL_SEARCH, tracking.ORB_TRACK_FAIL_MAP}
