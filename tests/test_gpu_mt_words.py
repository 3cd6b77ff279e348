"""rhccq_mt_words: the process's one table of raw MT19937(42) words on a device (csrc/mt_replay.h, api.hip) against numpy's generator,
across one growth: a pointer handed out before the growth still reads what it read.  The table belongs to the process, so the check runs in
a child that starts without one.  GPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def check():
    from roibasedimagecompression_amd.ops import Rhccq
    rh = Rhccq(0)
    big = (1 << 22) + 1
    # (full-range uint32 draws are the raw 32-bit outputs, one word each)
    want = np.random.RandomState(42).randint(0, 1 << 32, size=big, dtype=np.uint32)

    memcpy = rh._raw.hipMemcpy                             # (the HIP runtime the library is linked with: the handle resolves it)
    memcpy.restype, memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def read(ptr, first, count):
        out = np.zeros(count, np.uint32)
        assert memcpy(out.ctypes.data, ptr.value + 4 * first, 4 * count, 2) == 0      # device to host, blocking
        return out

    p1, n1 = rh._mt_words(10)
    assert p1.value and 10 <= n1 < big
    assert np.array_equal(read(p1, 0, 10), want[:10])
    p2, n2 = rh._mt_words(big)                             # one growth
    assert p2.value and p2.value != p1.value and n2 >= big
    assert np.array_equal(read(p2, 0, 10), want[:10])
    assert read(p2, big - 1, 1)[0] == want[big - 1]
    assert np.array_equal(read(p1, 0, 10), want[:10])      # the superseded table stays allocated
    p3, n3 = rh._mt_words(10)                              # no growth: the same table
    assert (p3.value, n3) == (p2.value, n2)
    words, count = C.c_void_p(), C.c_int64()
    assert rh._raw.rhccq_mt_words(rh.ctx, 0, C.byref(words), C.byref(count)) == -1
    assert rh._raw.rhccq_mt_words(rh.ctx, 10, None, C.byref(count)) == -1
    print("mt_words ok")


def test_mt_words_on_the_device_across_a_growth():
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_mt_words as t; t.check()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0 and r.stdout.strip().endswith("mt_words ok"), (r.returncode, r.stdout[-400:], r.stderr[-2000:])
