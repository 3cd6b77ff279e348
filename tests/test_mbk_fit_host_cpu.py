"""The host rules of the MiniBatchKMeans fits of rhccq_encode_frame without a device (csrc/mbk_fit_host.h, tests/native/mbk_fit_host_test.cpp):
the constants of a problem against sklearn's rules, the chunk planner replayed as a lone problem and as a batch over scripted state snapshots
(a problem gets in a batch the schedule and steps it gets alone), the layout of a batch, and the stop codes that are errors.  A stand-alone
program compiled with plain g++ and the host sanitizers: the header needs no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mbk_fit_host_rules(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path / "mbk_fit_host_test"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "roibasedimagecompression_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "mbk_fit_host_test.cpp"), "-o", str(exe)]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "mbk_fit_host ok", (r.returncode, r.stdout, r.stderr)
