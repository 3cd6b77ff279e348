"""csrc/km_wide_host.h without a device: which problems of a rhccq_kmeans call take the wide Lloyd path, their tiles, and the loop that
enqueues (E, M) launches in chunks and reads the state records back (tests/native/km_wide_host_test.cpp: problems ending in different
chunks, a stop on a chunk's last iteration by either rule, the 300-iteration limit, a call with no wide problem).  Compiled with plain
g++, which also pins that the header needs no HIP header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_rule_tiles_and_host_loop(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path / "km_wide_host_test"
    cmd = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "roibasedimagecompression_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "km_wide_host_test.cpp"), "-o", str(exe)]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "km_wide_host ok", (r.returncode, r.stdout, r.stderr)
