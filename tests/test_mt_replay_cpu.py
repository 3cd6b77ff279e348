"""The one replay of RandomState(42) (csrc/mt_replay.h) without a device: rhccq_mbk_draws against numpy's RandomState itself, draw by
draw as sklearn's MiniBatchKMeans.fit makes them ahead of k-means++, and the header's own stand-alone program (tests/native/
mt_replay_test.cpp: plain g++ and the host sanitizers, no HIP header)."""
import ctypes as C
import math
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, k, the first centre numpy gives): init_size == n, 3 k > 3000, a rejection mask at a power-of-two boundary, the one-value range
CASES = ((1500000, 30000, 3714), (10000, 20, 649), (999, 5, 551), (2500, 1000, 646), (65537, 40, 2904), (3, 2, 2), (12000, 130, 1809), (1, 1, 0))
FIELDS = ("batch", "limit", "init_size", "n_uniforms", "pos", "cursor0", "T", "first")


def _position(rs, limit):
    """raw words `rs` has consumed since RandomState(42) was seeded: the place of its next word in the generator's own stream"""
    w = np.random.RandomState(42).randint(0, 1 << 32, size=limit + 8, dtype=np.uint32)
    nxt = rs.randint(0, 1 << 32, size=8, dtype=np.uint32)
    hits = [p for p in np.flatnonzero(w[:limit + 1] == nxt[0]) if np.array_equal(w[p:p + 8], nxt)]
    assert len(hits) == 1
    return int(hits[0])


def _numpy_draws(n, k):
    """sklearn MiniBatchKMeans(k, batch_size=1000, random_state=42).fit ahead of its k-means++ uniforms, on numpy's generator"""
    batch = min(1000, n)
    init_size = 3 * batch
    if init_size < k:
        init_size = 3 * k
    init_size = min(init_size, n)
    rs = np.random.RandomState(42)
    rs.randint(0, n, init_size)                            # validation_indices: moves the stream only
    init_idx = rs.randint(0, n, init_size) if init_size < n else np.arange(n)
    first = int(rs.choice(init_size, p=np.full(init_size, 1.0) / init_size))
    T = 2 + int(math.log(k))
    pos = _position(rs, 8 * init_size + 64)
    return init_idx, dict(batch=batch, limit=(100 * n) // batch, init_size=init_size, n_uniforms=max((k - 1) * T, 1), pos=pos,
                          cursor0=pos + 2 * (k - 1) * T, T=T, first=first)


def _draws(lib, n, k):
    from roibasedimagecompression_amd._lib import MbkDraw
    d = MbkDraw()
    assert lib.rhccq_mbk_draws(n, k, C.byref(d), None, 0) == 0
    idx = np.full(d.init_size + 1, -7, np.int32)
    full = MbkDraw()
    assert lib.rhccq_mbk_draws(n, k, C.byref(full), idx.ctypes.data, d.init_size) == 0
    assert idx[-1] == -7
    return d, full, idx[:-1]


@pytest.fixture(scope="module")
def lib():
    from roibasedimagecompression_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("n,k,first", CASES)
def test_mbk_draws_equal_numpy_randomstate(lib, n, k, first):
    from roibasedimagecompression_amd._lib import MbkDraw
    sized, full, idx = _draws(lib, n, k)
    want_idx, want = _numpy_draws(n, k)
    assert want["first"] == first
    assert np.array_equal(idx, want_idx)
    assert {f: getattr(full, f) for f in FIELDS} == want
    # the NULL-buffer form: what follows from (n, k) alone, the rest untouched at 0
    for f in ("batch", "limit", "init_size", "n_uniforms", "T"):
        assert getattr(sized, f) == want[f]
    assert (sized.pos, sized.cursor0, sized.first) == (0, 0, 0)
    # a buffer one too small, and bad arguments: refused without a write
    if want["init_size"] > 1:
        d, small = MbkDraw(batch=-5, first=-5), np.full(want["init_size"], -7, np.int32)
        assert lib.rhccq_mbk_draws(n, k, C.byref(d), small.ctypes.data, want["init_size"] - 1) == -1
        assert (d.batch, d.first) == (-5, -5) and (small == -7).all()
    for bad_n, bad_k in ((n, 0), (n, n + 1), (0, 1), (1 << 31, 5)):
        d = MbkDraw(batch=-5)
        assert lib.rhccq_mbk_draws(bad_n, bad_k, C.byref(d), None, 0) == -1 and d.batch == -5
    assert lib.rhccq_mbk_draws(n, k, None, None, 0) == -1


def test_mbk_draws_from_eight_threads(lib):
    """eight threads drawing different problems at once (ctypes releases the interpreter lock) get the single-thread results"""
    alone = [_draws(lib, n, k) for n, k, _ in CASES]
    with ThreadPoolExecutor(max_workers=8) as pool:
        for _ in range(3):
            together = list(pool.map(lambda c: _draws(lib, c[0], c[1]), CASES))
            for (_, a, ai), (_, b, bi) in zip(alone, together):
                assert all(getattr(a, f) == getattr(b, f) for f in FIELDS) and np.array_equal(ai, bi)


def test_first_centre_index_equals_numpy_choice(lib):
    for n in (1, 2, 3, 999, 3000, 90000):
        for u in (0.0, 0.25, 0.3745401188473625, 0.5, 0.9999999999999999):
            p = np.full(n, 1.0) / n
            cdf = np.cumsum(p)
            cdf /= cdf[-1]
            assert lib.rhccq_first_centre_index(n, u) == min(int(np.searchsorted(cdf, u, side="right")), n - 1), (n, u)
    assert lib.rhccq_first_centre_index(0, 0.5) == -1


def test_mt_replay_header_program(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    exe = tmp_path / "mt_replay_test"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", os.path.join(ROOT, "roibasedimagecompression_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "mt_replay_test.cpp"), "-o", str(exe)]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "mt_replay ok", (r.returncode, r.stdout, r.stderr)
