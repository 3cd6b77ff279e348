"""rhccq_palette_refine_host (the device kernels' pack / evaluate / carry / update functions run serially: csrc/palette_refine.hip)
against the numpy reference of tests/refine_cases.py, bit for bit: palette bytes, history, n_iter; the argument errors; the
zero-pixel call; and the property the rounding rule buys, a history whose errors never increase.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import refine_cases as RF


def _ptr(a, off=0):
    return C.c_void_p(a.ctypes.data + off) if a is not None else C.c_void_p(0)


def _weights(w):
    return None if w is None else np.asarray(w, np.int32)


def host_refine(rgb, pal, cls, weights, max_iter):
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    pal = np.array(np.asarray(pal, np.uint8).reshape(-1, 3))                 # IN/OUT: a copy
    cls = None if cls is None else np.ascontiguousarray(cls, np.uint8).reshape(-1)
    w = _weights(weights)
    history = np.full((max_iter, 2), 0x5555, np.uint64)                      # (the call zeroes them)
    n_iter = np.full(1, -7, np.int32)
    rc = lib.rhccq_palette_refine_host(_ptr(rgb), len(rgb), _ptr(pal), len(pal), _ptr(cls), 0 if w is None else len(w) - 1, _ptr(w), max_iter,
                                       _ptr(history), _ptr(n_iter))
    return rc, pal, history.astype(np.int64), int(n_iter[0])


def test_sizes_are_exported():
    from roibasedimagecompression_amd import _lib
    assert 0 < RF.T <= RF.L
    lib = _lib.load()
    assert lib.rhccq_palette_refine_bytes(1) >= 32 and lib.rhccq_palette_refine_bytes(65536) >= 65536 * 32


@pytest.mark.parametrize("name", RF.names())
def test_host_equals_reference(name):
    c = RF.case(name)
    want_pal, want_hist, want_n = RF.reference(name)
    rc, pal, hist, n = host_refine(c["rgb"], c["pal"], c["cls"], c["weights"], c["max_iter"])
    assert rc == 0, name
    assert n == want_n and np.array_equal(hist, want_hist), (name, hist.tolist(), want_hist.tolist())
    assert np.array_equal(pal, want_pal), name
    dup = RF.later_duplicates(c["pal"])                                      # unchanged by the first iteration (refine_cases.reference)
    if len(dup):
        rc, one, _, _ = host_refine(c["rgb"], c["pal"], c["cls"], c["weights"], 1)
        assert rc == 0 and np.array_equal(one[dup], c["pal"][dup]), name


@pytest.mark.parametrize("name", RF.names())
def test_error_never_increases(name):
    """the nearest integer to the weighted mean minimises a row's error over the integers, so neither step of an iteration can raise E
    (a floor mean would: see round_half_up)"""
    c = RF.case(name)
    rc, _, hist, n = host_refine(c["rgb"], c["pal"], c["cls"], c["weights"], c["max_iter"])
    assert rc == 0 and (np.diff(hist[:n, 0]) <= 0).all(), (name, hist[:n, 0].tolist())
    assert (hist[n:] == 0).all()
    assert n == c["max_iter"] or n == 0 or hist[n - 1, 1] == 0


def test_early_stop():
    c = RF.case("early_stop")
    want_pal, want_hist, want_n = RF.reference("early_stop")
    assert want_n < c["max_iter"] and want_hist[want_n - 1, 1] == 0 and (want_hist[:want_n - 1, 1] > 0).all()
    rc, pal, hist, n = host_refine(c["rgb"], c["pal"], None, None, want_n)   # max_iter = n_iter: the same palette
    assert rc == 0 and n == want_n and np.array_equal(pal, want_pal) and np.array_equal(hist, want_hist[:want_n])


def _error_call(over, fn, device_only_args):
    rgb, pal = np.zeros((4, 3), np.uint8), np.zeros((3, 3), np.uint8)
    cls = np.zeros(4, np.uint8) if over.get("cls") else None
    bufs = {"rgb": rgb, "palette": pal, "history": np.zeros((65, 2), np.uint64), "n_iter": np.zeros(2, np.int32)}
    bufs.update({k: v for k, v in over.items() if k in bufs})
    off = {k: 0 for k in bufs}
    if over.get("misalign") in off:
        off[over["misalign"]] = 2 if over["misalign"] == "n_iter" else 1
    w = _weights(over.get("weights"))
    return fn(_ptr(bufs["rgb"]), over.get("n_pixels", 4), _ptr(bufs["palette"]), over.get("K", 3), _ptr(cls), over.get("n_classes", 0), _ptr(w),
              over.get("max_iter", 2), _ptr(bufs["history"], off["history"]), _ptr(bufs["n_iter"], off["n_iter"]))


@pytest.mark.parametrize("what,over,code", [e[:3] for e in RF.ERRORS if not e[3]], ids=[e[0] for e in RF.ERRORS if not e[3]])
def test_host_argument_errors(what, over, code):
    from roibasedimagecompression_amd import _lib
    assert _error_call(over, _lib.load().rhccq_palette_refine_host, False) == code, what


def test_host_accepts_the_valid_call_the_errors_vary():
    """the call every error case changes one argument of succeeds, with and without its class map; no pixels: n_iter = 0, a zero
    history, the palette untouched"""
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    assert _error_call({}, lib.rhccq_palette_refine_host, False) == 0
    assert _error_call({"cls": True, "n_classes": 2, "weights": [0, 0, 255]}, lib.rhccq_palette_refine_host, False) == 0
    assert _error_call({"max_iter": 64}, lib.rhccq_palette_refine_host, False) == 0
    assert _error_call({"K": 65536, "palette": np.zeros((65536, 3), np.uint8)}, lib.rhccq_palette_refine_host, False) == 0
    pal0 = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    rc, pal, hist, n = host_refine(np.zeros((0, 3), np.uint8), pal0, None, None, 5)
    assert rc == 0 and n == 0 and not hist.any() and np.array_equal(pal, pal0)


def test_device_entry_points_raise_without_a_gpu():
    """no CPU fallback: Rhccq.palette_refine and encode_with_palette(refine=N) need the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError
    from roibasedimagecompression_amd.image import ImageEncoder

    def run():
        return ImageEncoder().encode_with_palette(np.full((4, 4, 3), 9, np.uint8), np.zeros((1, 3), np.uint8), refine=2)
    if torch.cuda.is_available():
        out = run()
        assert out["palette"].tolist() == [[9, 9, 9]] and out["stats"]["refine"]["iterations"] == 2 and out["stats"]["remap"]["all"]["sse"] == 0
    else:
        with pytest.raises(RhccqError):
            run()
