"""The serial host forms of the optimising JPEG writer (csrc/jpeg_optimize.h; include/rhccq.h "JPEG files written with optimised Huffman
tables"): whole files against Pillow's save(optimize=True), the table construction against libjpeg's rule on synthetic counts.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases as J
import jpegopt_cases as O
import jpegwrite_cases as W


@pytest.mark.parametrize("name", list(O.CASES))
def test_host_form_equals_pillow(name):
    _, counts, data = O.host(name)
    assert data == O.pillow(name), name
    assert len(data) <= len(W.save(O.image(name), *[O.CASES[name][i] for i in (3, 2, 4)])), name
    assert int(counts[0].sum()) + int(counts[2].sum()) == O.host(name)[0].shape[0], "one DC symbol a block"


@pytest.mark.parametrize("name", list(O.COUNT_CASES))
def test_host_tables_equal_libjpegs_rule(name):
    deepest = O.check_tables(name, O.host_tables(name))
    assert name != "fold_ties" or deepest > 16, "the fold did not run"


def test_optimize_off_is_the_writer():
    lib, name = J.lib(), "17x33_420"
    H, Wd, mode, quality, rows, _ = W.CASES[name]
    out, n = np.zeros(1 << 16, np.uint8), C.c_int64()
    assert lib.rhccq_jpeg_encode_optimize_host(J._ptr(W.image(name)), H, Wd, W.MODE[mode], quality, rows, 0, J._ptr(out), out.size, C.byref(n)) == 0
    assert out[:n.value].tobytes() == W.pillow(name)


def test_refusals():
    lib, img, out, n = J.lib(), np.zeros((8, 8, 3), np.uint8), np.zeros(4096, np.uint8), C.c_int64()
    small, counts, sizes = np.zeros((3, 64), np.int16), np.zeros((4, 256), np.uint32), [C.c_int64() for _ in range(4)]
    for H, Wd, mode, q, rows in ((8, 8, 1, 0, 0), (8, 8, 1, 101, 0), (8, 8, 4, 75, 0), (8, 8, -1, 75, 0), (0, 8, 1, 75, 0), (8, 65536, 1, 75, 0), (8, 8, 1, 75, -1)):
        assert lib.rhccq_jpeg_encode_optimize_host(J._ptr(img), H, Wd, mode, q, rows, 1, J._ptr(out), out.size, C.byref(n)) == -1, (H, Wd, mode, q, rows)
        assert lib.rhccq_jpeg_optimize_sizes(H, Wd, mode, q, rows, *[C.byref(s) for s in sizes]) == -1
        if 1 <= q <= 100:
            assert lib.rhccq_jpeg_histogram_host(J._ptr(small), H, Wd, mode, rows, J._ptr(counts)) == -1
    # 3125 x 5000 blocks: 64 * 15625000 + 1 >= 10^9, where libjpeg's search for the least count starts (refused before anything is read)
    assert lib.rhccq_jpeg_histogram_host(J._ptr(small), 40000, 25000, 0, 0, J._ptr(counts)) == -3
    assert lib.rhccq_jpeg_optimize_sizes(40000, 25000, 0, 75, 0, *[C.byref(s) for s in sizes]) == -3
    assert lib.rhccq_jpeg_encode_optimize_host(J._ptr(img), 40000, 25000, 0, 75, 0, 1, J._ptr(out), out.size, C.byref(n)) == -3
    big = np.zeros((4, 256), np.uint32)
    big[1, :2] = 500000000
    std = O.standard_tables("444")
    assert lib.rhccq_jpeg_huffman_host(J._ptr(big), 16, 16, 1, 0, J._ptr(std), J._ptr(std.copy())) == -3
    assert lib.rhccq_jpeg_huffman_host(J._ptr(counts), 16, 16, 1, 0, J._ptr(std), J._ptr(std)) == -1
    assert lib.rhccq_jpeg_optimize_sizes(8, 8, 1, 75, 0, *[C.byref(s) for s in sizes]) == 0 and sizes[3].value > 640
