"""Shared cases of the resize tests (tests/test_resize_cpu.py, tests/test_gpu_resize.py): a plain helper module, not a conftest.

`resize_reference` is the numpy statement of rhccq_resize (include/rhccq.h "resize"): the taps in Python floats, the sums in int64.
Every case's input and reference are computed once per process and shared (do not modify what `case` and `reference` return)."""
import ctypes as C
import functools
import math

import numpy as np

FILTERS = ("box", "triangle", "cubic", "lanczos")
SUPPORT = {"box": 0.5, "triangle": 1.0, "cubic": 2.0, "lanczos": 3.0}
E_ARG, E_LIMIT = -1, -3
TILE_ROWS, RUN_COLS, STRIP = 64, 32, 1024      # the kernels' constants (csrc/resize.h), exported by ops.resize_tile()


def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(x * math.pi) / (x * math.pi)


def _filter(name, x):
    if name == "box":
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "triangle":
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if name == "cubic":
        a, x = -0.5, abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a if x < 2.0 else 0.0
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


@functools.lru_cache(maxsize=None)
def taps_reference(n, m, name):
    """-> (first, count, weights): lists over the m output samples, weights one list of ints per sample"""
    scale = n / m
    fs, support = max(scale, 1.0), SUPPORT[name] * max(scale, 1.0)
    first, count, weights = [], [], []
    for i in range(m):
        centre = (i + 0.5) * scale
        lo, hi = max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), n)
        w = [_filter(name, (t + lo - centre + 0.5) / fs) for t in range(max(hi - lo, 0))]
        total = 0.0
        for v in w:                                                          # (in order, as the C loop adds them; sum() compensates)
            total += v
        w = [v / total for v in w] if total != 0.0 else w
        first.append(lo)
        count.append(len(w))
        weights.append([int(0.5 + v * 4194304.0) if v >= 0 else int(-0.5 + v * 4194304.0) for v in w])
    return first, count, weights


def _axis(a, axis, m, name):
    n = a.shape[axis]
    if n == m:
        return a
    first, count, weights = taps_reference(n, m, name)
    src = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((m,) + src.shape[1:], np.int64)
    for i in range(m):
        w = np.array(weights[i], np.int64).reshape((-1,) + (1,) * (src.ndim - 1))
        out[i] = (w * src[first[i]:first[i] + count[i]]).sum(axis=0)
    return np.moveaxis(np.clip((out + (1 << 21)) >> 22, 0, 255).astype(np.uint8), 0, axis)


def resize_reference(a, OH, OW, name):
    """a uint8 [H, W], [H, W, C] or [B, H, W, C] -> the same rank with OH, OW: the rows pass (width) first, through a uint8 intermediate"""
    a = np.asarray(a, np.uint8)
    h = a.ndim - 3 if a.ndim == 4 else 0
    return np.ascontiguousarray(_axis(_axis(a, h + 1, OW, name), h, OH, name))


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def host_resize(a, OH, OW, name):
    """rhccq_resize_host on [B, H, W, C] -> (return code, out); the output is pre-filled"""
    from roibasedimagecompression_amd import _lib
    a = np.ascontiguousarray(a, np.uint8)
    B, H, W, Cn = a.shape
    out = np.full((B, OH, OW, Cn), 0xAB, np.uint8)
    rc = _lib.load().rhccq_resize_host(_ptr(a), B, H, W, Cn, _ptr(out), OH, OW, FILTERS.index(name))
    return rc, out


# the ten shape pairs on which the definition was checked against Pillow: ((H, W), (OH, OW))
PILLOW_SHAPES = [((1, 1), (1, 1)), ((1, 7), (3, 2)), ((5, 1), (2, 4)), ((37, 53), (11, 7)), ((64, 65), (8, 9)), ((9, 11), (40, 33)),
                 ((130, 257), (17, 16)), ((33, 31), (33, 10)), ((256, 256), (255, 257)), ((600, 17), (3, 17))]

# name -> (B, H, W, C, OH, OW, saturated): what each case is there for is in its name
SHAPES = {
    "one": (1, 1, 1, 3, 1, 1, False),
    "row_in": (1, 1, 40, 3, 5, 13, False),                 # 1 x W input
    "column_in": (1, 40, 1, 3, 13, 5, False),              # H x 1 input
    "ow1": (1, 20, 50, 3, 10, 1, False),
    "oh1": (1, 50, 20, 3, 1, 10, False),
    "h63": (1, 63, 20, 3, 30, 9, False),                   # the rows pass's lane-per-row tile: one short, full, one over, two tiles and one
    "h64": (1, 64, 20, 4, 30, 9, False),
    "h65": (1, 65, 20, 1, 30, 9, False),
    "h129": (1, 129, 20, 3, 40, 9, False),
    "run-1": (1, 9, 70, 3, 5, RUN_COLS - 1, False),        # the rows pass's column run: one short, full, one over
    "run": (1, 9, 70, 3, 5, RUN_COLS, False),
    "run+1": (1, 9, 70, 3, 5, RUN_COLS + 1, False),
    "strip1023": (1, 7, 1200, 1, 3, STRIP - 1, False),     # row bytes around the columns pass's dword and strip edges
    "strip1025": (1, 7, 1200, 1, 3, STRIP + 1, False),
    "strip1023c3": (1, 7, 400, 3, 3, 341, False),
    "strip1026c3": (1, 7, 400, 3, 3, 342, False),
    "strip1024c4": (1, 7, 300, 4, 3, 256, False),
    "bytes3": (1, 12, 9, 1, 5, 3, False),                  # a row shorter than a dword
    "bytes2": (1, 12, 9, 1, 5, 2, False),
    "long_rows": (1, 17, 600, 3, 17, 3, False),            # a window longer than one LDS tile: chunked sums
    "long_cols": (1, 600, 17, 3, 3, 17, False),
    "aligned16": (1, 70, 304, 4, 21, 40, False),           # rows of a multiple of 16 bytes: the 16-byte staging, two chunks a run
    "upscale": (1, 9, 11, 3, 40, 33, False),               # windows clipped at both borders
    "copy_rows": (1, 33, 31, 3, 10, 31, False),            # one axis unchanged: the copy pass
    "copy_cols": (1, 33, 31, 3, 33, 10, False),
    "copy_both": (1, 33, 31, 3, 33, 31, False),
    "batch3": (3, 21, 35, 3, 8, 13, False),
    "saturated": (1, 66, 70, 3, 19, 23, True),             # 0 and 255 only: both sides of the clamp under cubic and lanczos
}


@functools.lru_cache(maxsize=None)
def case(name):
    B, H, W, Cn, _, _, saturated = SHAPES[name]
    a = np.random.default_rng(sum(map(ord, name))).integers(0, 256, (B, H, W, Cn), dtype=np.uint8)
    a = np.where(a < 128, 0, 255).astype(np.uint8) if saturated else a
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(name, filt):
    out = resize_reference(case(name), *SHAPES[name][4:6], filt)
    out.setflags(write=False)
    return out


# the argument errors of rhccq_resize_host: (what, overrides of a valid call, return code).  A valid call: B = 1, 4 x 5 x 3 -> 2 x 3, lanczos
ERRORS = [
    ("null src", {"src": None}, E_ARG), ("null dst", {"dst": None}, E_ARG), ("B = 0", {"B": 0}, E_ARG), ("H = 0", {"H": 0}, E_ARG),
    ("W = 65536", {"W": 65536}, E_ARG), ("OH = 0", {"OH": 0}, E_ARG), ("OW = 65536", {"OW": 65536}, E_ARG), ("C = 2", {"C": 2}, E_ARG),
    ("C = 5", {"C": 5}, E_ARG), ("filter -1", {"filter": -1}, E_ARG), ("filter 4", {"filter": 4}, E_ARG), ("B = 65536", {"B": 65536}, E_LIMIT),
    ("B = 65536 and C = 2", {"B": 65536, "C": 2}, E_ARG),
]
