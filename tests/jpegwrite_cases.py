"""The JPEG writer's cases (include/rhccq.h "JPEG files written on the device"): images from seeded noise on a ramp as jpeg_cases makes them,
the reference the bytes Pillow saves from them."""
import ctypes as C
import functools
import io

import numpy as np
from PIL import Image

import jpeg_cases as J

MODE = {"grey": 0, "444": 1, "422": 2, "420": 3}

# name -> (H, W, mode, quality, restart rows, kind): every shape with every mode, quality and restart rows taken round and round
CASES = {}
for i, (H, W) in enumerate(J.SHAPES):
    for j, mode in enumerate(J.MODES):
        t = 4 * i + j
        CASES[f"{H}x{W}_{mode}"] = (H, W, mode, (30, 95, 100)[(t + i) % 3], (t + j // 2) % 2, "noise")
for H, W in ((7, 3), (8, 4)):                                # a chroma component narrower than a block
    for mode in ("422", "420"):
        CASES[f"{H}x{W}_{mode}_narrow"] = (H, W, mode, 95, 0, "noise")
CASES["flat"] = (40, 24, "420", 90, 0, "flat")              # every block DC difference 0 and EOB: the scan ends inside a byte
CASES["checker"] = (24, 40, "444", 100, 1, "checker")       # blocks alternately 0 and 255: DC category 11
CASES["impulses"] = (32, 48, "grey", 30, 0, "impulses")     # single bright pixels: runs of 16 zeros and more in front of a value
CASES["noise_q100"] = (64, 72, "444", 100, 0, "loud")       # a scan of several stuffing tiles, more blocks than a pack workgroup, stuffed 0xFF


def names():
    return list(CASES)


@functools.lru_cache(maxsize=None)
def image(name):
    H, W, mode, _, _, kind = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "flat":
        img = np.full((H, W, 3), 97, np.uint8)
    elif kind == "checker":
        img = np.repeat((((yy // 8 + xx // 8) % 2) * 255).astype(np.uint8)[..., None], 3, 2)
    elif kind == "impulses":
        img = np.zeros((H, W, 3), np.uint8)
        at = np.random.default_rng(0)                        # (chosen so that Pillow's scan holds ZRL codes: test_jpeg_write_cpu checks it)
        img[at.integers(0, H, 12), at.integers(0, W, 12)] = 255
    else:
        amp = 255 if kind == "loud" else 128
        img = (rng.integers(0, amp + 1, (H, W, 3)) + (0 if kind == "loud" else (yy + 2 * xx)[..., None])).clip(0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[..., 0] if mode == "grey" else img)


def save(img, quality, mode, restart_rows):
    out = io.BytesIO()
    kw = {"restart_marker_rows": restart_rows} if restart_rows else {}
    if img.ndim == 3:
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[mode]
    Image.fromarray(img).save(out, "JPEG", quality=quality, optimize=False, **kw)
    return out.getvalue()


@functools.lru_cache(maxsize=None)
def pillow(name):
    _, _, mode, quality, rows, _ = CASES[name]
    return save(image(name), quality, mode, rows)


@functools.lru_cache(maxsize=None)
def pillow_coefficients(name):
    """rhccq_jpeg_coefficients_host of Pillow's file"""
    st, _, _, coef = J.host_decode(pillow(name))
    assert st == J.OK
    return coef


def host_encode(img, mode, quality, restart_rows):
    """rhccq_jpeg_blocks_host and rhccq_jpeg_encode_host -> (coefficients int16[blocks, 64], the file's bytes)"""
    lib = J.lib()
    H, W = img.shape[:2]
    sizes = [C.c_int64() for _ in range(4)]
    assert lib.rhccq_jpeg_write_sizes(H, W, MODE[mode], quality, restart_rows, *[C.byref(s) for s in sizes]) == 0
    coef, out, n = np.zeros((sizes[0].value // 64, 64), np.int16), np.zeros(sizes[3].value, np.uint8), C.c_int64()
    assert lib.rhccq_jpeg_blocks_host(J._ptr(img), H, W, MODE[mode], quality, J._ptr(coef)) == 0
    assert lib.rhccq_jpeg_encode_host(J._ptr(img), H, W, MODE[mode], quality, restart_rows, J._ptr(out), out.size, C.byref(n)) == 0
    return coef, out[:n.value].tobytes()
