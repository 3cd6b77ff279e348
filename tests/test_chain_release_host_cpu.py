"""The host wait of a lane of rhccq_encode_frame for its problem's k-means++ chain inside the frame's chain launch, without a device
(tests/native/chain_release_host_test.cpp over csrc/chain_release_host.h): the flag fires before the event; the event completes with the
flag never set (the fallback for kernels that publish nothing); the previous frame's tag is not taken; a failing event query throws; nothing
sleeps once either condition holds.  A stand-alone program compiled with plain g++ and the host sanitizers: the header needs no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_release_wait_policy(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path / "chain_release_host_test"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "roibasedimagecompression_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "chain_release_host_test.cpp"), "-o", str(exe)]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "chain_release_host ok", (r.returncode, r.stdout, r.stderr)
