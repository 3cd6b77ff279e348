"""Host-only sizing of the device zlib encoder (rhccq_zlib_sizes): no GPU needed."""
import ctypes as C

import pytest


def _sizes(n):
    from roibasedimagecompression_amd import _lib
    ws, bound = C.c_int64(), C.c_int64()
    rc = _lib.load().rhccq_zlib_sizes(n, C.byref(ws), C.byref(bound))
    return rc, ws.value, bound.value


@pytest.mark.parametrize("n", [0, 1, 3, 4096, 65535, 65536, 65537, 16588800, 5 * 2 ** 20 + 3])
def test_bound_covers_stored_blocks(n):
    rc, ws, bound = _sizes(n)
    assert rc == 0
    pieces = max(1, -(-n // 65535))
    # 2-byte header, 4-byte Adler-32, and per stored piece 3 header bits + alignment + LEN / NLEN
    assert bound >= n + 6 + 5 * pieces
    assert ws >= 4 * n


def test_negative_size_is_refused():
    assert _sizes(-1)[0] == -1
