"""The serial host forms of the JPEG writer (csrc/jpeg_write.h; include/rhccq.h "JPEG files written on the device") against Pillow: the whole
file byte for byte, and the coefficients against those the reader's host form takes from Pillow's file.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases as J
import jpegwrite_cases as W


@pytest.mark.parametrize("name", W.names())
def test_host_forms_equal_pillow(name):
    _, _, mode, quality, rows, _ = W.CASES[name]
    coef, data = W.host_encode(W.image(name), mode, quality, rows)
    assert np.array_equal(coef, W.pillow_coefficients(name)), name
    assert data == W.pillow(name), name


def test_the_cases_hold_what_they_are_for():
    zz = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22,
                   15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
    nz = W.pillow_coefficients("impulses")[:, zz[1:]] != 0
    runs = [np.diff(np.flatnonzero(np.concatenate(([True], row)))).max(initial=0) for row in nz]
    assert max(runs) > 16, "no ZRL in Pillow's scan"
    loud = W.pillow("noise_q100")
    scan = loud[loud.index(b"\xff\xda"):]
    assert len(scan) > 2 * 4096 and W.pillow_coefficients("noise_q100").shape[0] > 32 and b"\xff\x00" in scan
    assert np.abs(np.diff(W.pillow_coefficients("checker")[:, 0].astype(np.int32))).max() >= 1024, "no DC category 11"


def test_refusals():
    lib, img, out, n = J.lib(), np.zeros((8, 8, 3), np.uint8), np.zeros(4096, np.uint8), C.c_int64()
    coef = np.zeros((3, 64), np.int16)
    for H, Wd, mode, q, rows in ((8, 8, 1, 0, 0), (8, 8, 1, 101, 0), (8, 8, 4, 75, 0), (8, 8, -1, 75, 0), (0, 8, 1, 75, 0), (8, 65536, 1, 75, 0), (8, 8, 1, 75, -1)):
        assert lib.rhccq_jpeg_encode_host(J._ptr(img), H, Wd, mode, q, rows, J._ptr(out), out.size, C.byref(n)) == -1, (H, Wd, mode, q, rows)
        if rows == 0:
            assert lib.rhccq_jpeg_blocks_host(J._ptr(img), H, Wd, mode, q, J._ptr(coef)) == -1
        sizes = [C.c_int64() for _ in range(4)]
        assert lib.rhccq_jpeg_write_sizes(H, Wd, mode, q, rows, *[C.byref(s) for s in sizes]) == -1
    assert lib.rhccq_jpeg_encode_host(J._ptr(img), 8, 8, 1, 75, 0, J._ptr(out), out.size, C.byref(n)) == 0 and n.value > 600
