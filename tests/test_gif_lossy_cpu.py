"""The lossy GIF step (include/rhccq.h "lossy") in its host forms, rhccq_gif_encode_lossy_host and rhccq_gif_lzw_lossy_host, against the dict
reference of tests/gif_lossy_cases.py: the file's bytes, the written pixels, Pillow's picture and the bound.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import gif_cases as G
import gif_lossy_cases as L


@pytest.mark.parametrize("name", L.names())
def test_host_file_equals_reference(name):
    rcs, data, streams, (wr_file, wr_lzw) = L.host(name)
    assert rcs == (0, 0)
    L.check(name, data, wr_file)
    assert streams == L.reference(name)[1] and np.array_equal(wr_lzw, wr_file)


@pytest.mark.parametrize("eb,shift", [(1, 0), (1, 1), (1, 15), (2, 0), (2, 6), (4, 12)])
def test_host_index_maps(eb, shift):
    name = "k64" if eb == 1 else "clamp"                                # (clamp holds indices past 255)
    rcs, data, _, (wr, _) = L.host(name, eb, shift)
    assert rcs == (0, 0)
    L.check(name, data, wr)


def test_slack0_is_the_lossless_entry_and_bad_arguments_are_refused():
    v = L.case("slack0")
    n, H, W = v["frames"].shape
    pal, stride, rows, flags = L.block("slack0")
    bound = G.sizes(n, H, W, flags)[3]
    out, length = np.zeros(bound, np.uint8), C.c_int64(0)
    assert G.lib().rhccq_gif_encode_host(G._ptr(G.index_array(v["frames"], 4)), 4, n, H, W, G._ptr(pal), stride, G._ptr(rows),
                                         G._ptr(np.array(v["delays"], np.int32)), v["loop"], flags, G._ptr(out), bound, C.byref(length), None) == 0
    assert out[:length.value].tobytes() == L.host("slack0")[1]
    assert L.host("k64", flags_or=G.TRIE)[0] == (G.E_ARG, G.E_ARG)
    for slack in (-1, L.MAX_SLACK + 1):
        assert L.host("k64", slack=slack)[0] == (G.E_ARG, G.E_ARG)
