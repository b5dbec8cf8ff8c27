"""The parts of csrc/rows.h and csrc/image_routes.h that make no HIP call -- for_each_on_threads, the hand-over of a route's files and of a
host twin's bytes, the rules of an image set -- in tests/cpp/test_image_routes.cpp, a stand-alone program with its own main: compiled for
the host alone (the headers include the HIP runtime's, so by hipcc) with the address and undefined-behaviour sanitizers, and run."""
import os
import subprocess

from conftest import ROOT
from mvs_texturing_amd.build import _hipcc

CSRC = os.path.join(ROOT, "mvs-texturing_amd", "csrc")


def test_host_parts_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_image_routes")
    subprocess.check_call([_hipcc(), "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-pthread",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "test_image_routes.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
