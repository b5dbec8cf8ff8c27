"""csrc/view_batches.h -- the batch cut, the place of an item inside its batch and the prefix array and grid bound of a span launch, which
every view input shares (csrc/view_input.h) -- is plain host C++: tests/cpp/test_view_batches.cpp is compiled against it with the address and
undefined-behaviour sanitizers and run.  The counts around 2^32 and the grid bound run here and nowhere else (no test scene reaches them)."""
import os
import subprocess

from conftest import ROOT


def test_cut_layout_and_spans_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_view_batches")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mvs-texturing_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_view_batches.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_header_has_no_device_code():
    """it is included by the stand-alone program above as it is: no HIP in it"""
    text = open(os.path.join(ROOT, "mvs-texturing_amd", "csrc", "view_batches.h")).read()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
