"""csrc/shard_lists.h -- the key layout of the sharded driver's lists (phase << 40 | peer << 32 | index: written on the device, decoded
on the host), the per (phase, peer) offsets of a sorted list and the byte ranges of a phase's chunk -- is plain host C++:
tests/cpp/test_shard_lists.cpp is compiled against it with the address and undefined-behaviour sanitizers and run.  The edges of the bit
fields, 64 ranks and record lengths past 2^32 run here and nowhere else (no test scene reaches them)."""
import os
import subprocess

from conftest import ROOT


def test_keys_segments_and_phase_offsets_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_shard_lists")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "mvs-texturing_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_shard_lists.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_header_has_no_device_code():
    """it is included by the stand-alone program above as it is: no HIP in it"""
    text = open(os.path.join(ROOT, "mvs-texturing_amd", "csrc", "shard_lists.h")).read()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
