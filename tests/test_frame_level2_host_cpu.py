"""The host side of rhccq_encode_frame's level-2 stage without a device (tests/native/frame_level2_host_test.cpp): the hand-over of the
classes' components and level-2 jobs with the clocks behind the `level2_cluster` / `level2_finish` timing keys (csrc/frame_level2_host.h),
and the launch schedule of a batch of overlapped mini-batch fits, which must give every problem the launches it gets alone
(csrc/mbk_schedule.h).  A stand-alone program compiled with plain g++ and the host sanitizers: neither header needs HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level2_handover_and_batch_schedule(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path / "frame_level2_host_test"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "roibasedimagecompression_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "frame_level2_host_test.cpp"), "-o", str(exe)]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "frame_level2_host ok", (r.returncode, r.stdout, r.stderr)
