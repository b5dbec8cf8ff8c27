"""csrc/dc_ranges.h -- the planner and the 64-bit accounting of the ranged data-cost pass -- is plain host C++: tests/cpp/test_dc_ranges.cpp
is compiled against it with the address and undefined-behaviour sanitizers and run.  The branches that need 2^32 (face, view) pairs or 2^32
kept entries run here and nowhere else (no test scene reaches them).  csrc/dc_counters.h -- the counter slots of a pass and the
statistics made of them -- gets the same treatment through tests/cpp/test_dc_counters.cpp."""
import os
import subprocess

from conftest import ROOT


def _run_under_sanitizers(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mvs-texturing_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_planner_and_accounting_under_sanitizers(tmp_path):
    _run_under_sanitizers(tmp_path, "test_dc_ranges")


def test_counter_slots_and_stats_under_sanitizers(tmp_path):
    _run_under_sanitizers(tmp_path, "test_dc_counters")


def _no_device_code(header):
    text = open(os.path.join(ROOT, "mvs-texturing_amd", "csrc", header)).read()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text


def test_planner_header_has_no_device_code():
    """it is included by the stand-alone program above as it is: no HIP in it"""
    _no_device_code("dc_ranges.h")


def test_counters_header_has_no_device_code():
    _no_device_code("dc_counters.h")
