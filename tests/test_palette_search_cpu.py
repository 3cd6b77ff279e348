"""The three host forms that run the one nearest-colour search (csrc/palette_remap.h: remap_search_host) against one another:
rhccq_palette_moments_host assigns every pixel of every remap case to the row rhccq_palette_remap_host gives it, and the error
rhccq_palette_refine_host reports for its first assignment under unit weights is the remap's total.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ladder_cases as LD
import remap_cases as RM


@pytest.mark.parametrize("name", RM.names())
def test_remap_moments_and_refine_assign_alike(name):
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    rgb, pal, cls, nc, _ = RM.case(name)
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 3)
    cls = None if cls is None else np.ascontiguousarray(cls, np.uint8).reshape(-1)
    n, K = len(rgb), len(pal)
    width = RM.index_bytes(K)[0]
    rc, idx_m, _ = LD.host_moments(rgb, pal, cls, nc, width)
    assert rc == 0, name
    if n == 0:                                            # (an empty array need not have an address)
        rgb, cls = np.zeros((1, 3), np.uint8), None if cls is None else np.zeros(1, np.uint8)
    idx_r = np.full(max(n, 1), 0xAB, {1: np.uint8, 2: np.uint16, 4: np.uint32}[width])
    sums = np.full((nc + 1, 2), 0x5555, np.uint64)
    assert lib.rhccq_palette_remap_host(LD.ptr(rgb), n, LD.ptr(pal), K, LD.ptr(cls), nc, LD.ptr(idx_r), width, LD.ptr(sums)) == 0, name
    assert np.array_equal(idx_m, idx_r[:n].astype(np.int64)), name
    rows = np.array(pal)                                  # IN/OUT: a copy
    history, n_iter = np.full((1, 2), 0x5555, np.uint64), np.full(1, -7, np.int32)
    assert lib.rhccq_palette_refine_host(LD.ptr(rgb), n, LD.ptr(rows), K, C.c_void_p(0), 0, C.c_void_p(0), 1, LD.ptr(history), LD.ptr(n_iter)) == 0, name
    assert int(history[0, 0]) == int(sums[nc, 1]) and int(n_iter[0]) == (1 if n else 0), name
