"""csrc/stash.h -- the two contexts the one-shot calls keep between them -- is plain host C++: tests/cpp/test_stash.cpp drives it with fake
contexts, every transition on one thread and then the call shapes of csrc/oneshot.hip on eight, built once with the address and
undefined-behaviour sanitizers and once with the thread sanitizer."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "mvs-texturing_amd", "csrc")


@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_stash_under_sanitizers(tmp_path, sanitizers):
    exe = str(tmp_path / "test_stash")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=" + sanitizers, "-fno-sanitize-recover=all", "-pthread",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "test_stash.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_stash_header_has_no_device_code():
    """it is included by the stand-alone program above as it is: no HIP in it"""
    text = open(os.path.join(CSRC, "stash.h")).read()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
