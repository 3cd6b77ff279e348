"""Shared cases of the error-diffusing remap tests (tests/test_palette_dither_cpu.py, tests/test_gpu_palette_dither.py): a plain helper
module, not a conftest.

`dither_reference` is the numpy statement of rhccq_palette_dither, a direct transcription of its definition: a Python loop over the
pixels in raster order, int64 throughout, the nearest row by the first minimum of the squared distances.  Every case's reference is
computed once per process and shared (do not modify what `case`, `reference` and `kodak_crop` return)."""
import ctypes as C
import functools
import os

import numpy as np

import remap_cases as RM

ROWS = (4, 8, 16, 32)                 # the values Rhccq.OPT_DITHER_ROWS takes beside 0: image rows of a band
R = max(ROWS)                         # the shapes sit at the edges of the tallest band (and so inside or at the edges of the others)
MAX_STRENGTH = 256
E_ARG, E_LIMIT = RM.E_ARG, RM.E_LIMIT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def strength_table(strength, n_classes):
    return [int(strength)] * (n_classes + 1) if np.ndim(strength) == 0 else [int(v) for v in strength]


def dither_reference(rgb, palette, strength, cls=None, n_classes=0):
    """-> (out int64[H, W], sums int64[n_classes + 1, 3]: row c = {pixels, squared error of out against the original pixel, pixels
    with out != b} over cls == c, the last row over every pixel, b int64[H, W], facts: {"low", "high": targets clamped at 0 / at 255
    per channel, "floor": terms s A + 2048 that are negative and no multiple of 4096, "ties": targets with more than one nearest
    row of different colours})"""
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    pal = np.asarray(palette, np.uint8).reshape(-1, 3).astype(np.int64)
    table = strength_table(strength, n_classes)
    assert len(table) == n_classes + 1 and min(table) >= 0 and max(table) <= MAX_STRENGTH
    c = np.full((H, W), n_classes, np.int64) if cls is None else np.minimum(np.asarray(cls).reshape(H, W).astype(np.int64), n_classes)
    b = RM.remap_reference(rgb, palette)[0].reshape(H, W)
    E = np.zeros((H + 1, W + 2, 3), np.int64)                               # E(y, x) at [y + 1, x + 1]: the terms outside stay 0
    out = np.zeros((H, W), np.int64)
    facts = {"low": np.zeros(3, np.int64), "high": np.zeros(3, np.int64), "floor": 0, "ties": 0}
    px = rgb.astype(np.int64)
    for y in range(H):
        for x in range(W):
            a = 7 * E[y + 1, x] + E[y, x] + 5 * E[y, x + 1] + 3 * E[y, x + 2]
            term = table[c[y, x]] * a + 2048
            raw = px[y, x] + (term >> 12)                                    # (numpy's >> on int64 floors toward minus infinity)
            t = np.clip(raw, 0, 255)
            d = ((pal - t) ** 2).sum(axis=1)
            k = int(d.argmin())                                              # (the first minimum: the lowest row)
            out[y, x] = k
            E[y + 1, x + 1] = t - pal[k]
            facts["low"] += raw < 0
            facts["high"] += raw > 255
            facts["floor"] += int(((term < 0) & (term % 4096 != 0)).sum())
            facts["ties"] += int(len({tuple(r) for r in pal[d == d[k]]}) > 1)
    dist = ((px - pal[out]) ** 2).sum(axis=2)
    moved = out != b
    sums = np.zeros((n_classes + 1, 3), np.int64)
    for k in range(n_classes):
        sel = c == k
        sums[k] = (sel.sum(), dist[sel].sum(), moved[sel].sum())
    sums[n_classes] = (H * W, dist.sum(), moved.sum())
    return out, sums, b, facts


_DT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def host_dither(rgb, pal, cls, n_classes, strength, elem_bytes):
    """rhccq_palette_dither_host in the element width asked for -> (return code, out int64[H, W], sums int64[n_classes + 1, 3])"""
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 3)
    cls = None if cls is None else np.ascontiguousarray(cls, np.uint8).reshape(-1)
    table = np.array(strength_table(strength, n_classes), np.uint32)
    idx = np.full(max(H * W, 1), 0xAB, _DT[elem_bytes])
    sums = np.full((n_classes + 1, 3), 0x5555, np.uint64)                  # (the call zeroes them)
    rc = lib.rhccq_palette_dither_host(_ptr(rgb if rgb.size else np.zeros(3, np.uint8)), H, W, _ptr(pal), len(pal), _ptr(cls), n_classes, _ptr(table),
                                       _ptr(idx), elem_bytes, _ptr(sums))
    return rc, idx[:H * W].astype(np.int64).reshape(H, W), sums.astype(np.int64)


def _image(rng, h, w):
    """a smooth picture with noise: gradients are what a small palette bands and error diffusion repairs"""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(3 * x + 5 * y) % 256, (255 - 2 * x + y) % 256, (7 * y + x // 2) % 256], axis=2)
    return np.clip(base + rng.integers(-9, 10, (h, w, 3)), 0, 255).astype(np.uint8)


def _build():
    """name -> (rgb uint8[H, W, 3], palette uint8[K, 3], cls uint8[H, W] or None, n_classes, strength (a number or a table), expected
    out rows or None)"""
    rng = np.random.default_rng(20261020)
    out = {}
    pal37 = RM._palette(rng, 37)
    # the smallest pictures; one image row of more than three tiles
    for h, w in ((1, 1), (1, 2), (1, 3), (2, 1), (3, 2), (1, 200)):
        out[f"shape{h}x{w}"] = (_image(rng, h, w), pal37, None, 0, 256, None)
    # narrow pictures of more than two bands: an image row starts before the row above it has two columns
    for w in (1, 2, 3):
        out[f"narrow{2 * R + 1}x{w}"] = (_image(rng, 2 * R + 1, w), pal37, None, 0, 256, None)
    # band edges: a short only band, a full one, a hand-over to a one-row band, two and three hand-overs with a short last band
    for h in (R - 1, R, R + 1, 2 * R + 1, 3 * R + 1):
        out[f"bands{h}x67"] = (_image(rng, h, 67), pal37, None, 0, 256, None)
    # palette sizes: one row, the 1-byte edge and the first 2-byte size, sizes around 1024 that no search slice divides, the device's cap
    for K in (1, 2, 3, 255, 256, 257, 1023, 1025, 4096):
        pal = RM._palette(rng, K, levels=256 if K % 2 else 6)
        out[f"K{K}"] = (_image(rng, 13, 45), pal, None, 0, 256, None)
    # a palette far inside the gamut under black and white stripes: the error piles up and the target clamps at both ends
    img = np.zeros((9, 70, 3), np.uint8)
    img[:, 35:] = 255
    img[4:] = 255 - img[4:]
    out["clamp"] = (img, np.array([[100, 100, 100], [150, 150, 150]], np.uint8), None, 0, 256, None)
    # an exact tie of a dithered target: pixel 0 (14) takes row 0 (12) and leaves 2, of which 7/16 rounds to 1: pixel 1 (10, which is row
    # 1 itself) aims at 11, one from rows 0 and 1 alike, and the lowest row wins
    out["tie"] = (np.array([[[14, 0, 0], [10, 0, 0]]], np.uint8), np.array([[12, 0, 0], [10, 0, 0], [20, 0, 0]], np.uint8), None, 0, 256, [[0, 0]])
    # strengths, on a palette with duplicate rows
    pal = RM._palette(rng, 60, levels=6)
    img = _image(rng, 21, 90)
    for s in (0, 1, 128, 256):
        out[f"strength{s}"] = (img, pal, None, 0, s, None)
    # class strengths: 2 classes, class values 2, 3 and 255 take the last entry; 16 classes
    img = _image(rng, R + 7, 93)
    cls = rng.integers(0, 4, img.shape[:2]).astype(np.uint8)
    cls[rng.random(img.shape[:2]) < 0.05] = 255
    blocks = np.repeat(rng.integers(0, 4, (img.shape[0], -(-img.shape[1] // 16))), 16, axis=1)[:, :img.shape[1]].astype(np.uint8)
    out["classes2"] = (img, pal37, cls, 2, [0, 256, 128], None)
    out["classes2_blocks"] = (img, pal37, blocks, 2, [256, 0, 0], None)
    out["classes16"] = (img, pal37, rng.integers(0, 18, img.shape[:2]).astype(np.uint8), 16, [16 * k for k in range(17)], None)
    # the hand-over's granules of 4 words, two hand-overs each: a last granule that is exactly full (4, 8, 64), that holds one word (5, 9,
    # 65), and widths at the staging tile's edge (63, 64, 65).  (Drawn last: the cases above keep their pictures.)
    for w in (4, 5, 7, 8, 9, 63, 64, 65):
        out[f"handover{2 * R + 1}x{w}"] = (_image(rng, 2 * R + 1, w), pal37, None, 0, 256, None)
    return out


_CASES = None


def names():
    global _CASES
    if _CASES is None:
        _CASES = _build()
        for rgb, pal, cls, _, _, _ in _CASES.values():
            for a in (rgb, pal, cls):
                if a is not None:
                    a.setflags(write=False)
    return list(_CASES)


def case(name):
    names()
    return _CASES[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (out int64[H, W], sums int64[n_classes + 1, 3], b int64[H, W], facts); what a case is there for is asserted here once"""
    rgb, pal, cls, nc, strength, expect = case(name)
    out, sums, b, facts = dither_reference(rgb, pal, strength, cls, nc)
    if expect is not None:
        assert out.tolist() == expect, name
    if name == "tie":
        assert b.tolist() == [[0, 1]] and facts["ties"] == 1
    if name == "clamp":
        assert (facts["low"] > 0).all() and (facts["high"] > 0).all(), facts
    if name == "strength256":
        assert facts["floor"] > 0 and sums[-1, 2] > 0
    if name == "strength0":
        assert np.array_equal(out, b) and sums[-1, 2] == 0
    for a in (out, sums, b):
        a.setflags(write=False)
    return out, sums, b, facts


def index_bytes(K):
    return RM.index_bytes(K)


# the argument errors of rhccq_palette_dither_host: (what, overrides of a valid call, return code).  A valid call: 2 x 2 pixels, K = 3, no
# class map, n_classes = 0, strength [5], 2-byte indices; "cls": True asks for a valid class map; "strength": a table or None (NULL).
ERRORS = [
    ("null rgb", {"rgb": None}, E_ARG),
    ("null palette", {"palette": None}, E_ARG),
    ("null idx_out", {"idx_out": None}, E_ARG),
    ("null sums", {"sums": None}, E_ARG),
    ("null strength", {"strength": None}, E_ARG),
    ("K = 0", {"K": 0}, E_ARG),
    ("K < 0", {"K": -5}, E_ARG),
    ("H < 0", {"H": -1}, E_ARG),
    ("W < 0", {"W": -1}, E_ARG),
    ("n_classes < 0", {"cls": True, "n_classes": -1}, E_ARG),
    ("n_classes = 17", {"cls": True, "n_classes": 17, "strength": [0] * 18}, E_ARG),
    ("n_classes without a class map", {"n_classes": 1, "strength": [0, 0]}, E_ARG),
    ("idx_elem_bytes = 0", {"idx_elem_bytes": 0}, E_ARG),
    ("idx_elem_bytes = 3", {"idx_elem_bytes": 3}, E_ARG),
    ("idx_elem_bytes = 8", {"idx_elem_bytes": 8}, E_ARG),
    ("K = 257 with 1-byte indices", {"K": 257, "idx_elem_bytes": 1}, E_ARG),
    ("strength 257", {"strength": [MAX_STRENGTH + 1]}, E_ARG),
    ("a class strength of 257", {"cls": True, "n_classes": 2, "strength": [0, MAX_STRENGTH + 1, 0]}, E_ARG),
    ("the last strength above 256", {"cls": True, "n_classes": 2, "strength": [0, 0, 1 << 31]}, E_ARG),
    ("K = 65537", {"K": 65537}, E_LIMIT),
    ("K = 65537 with a strength above 256", {"K": 65537, "strength": [MAX_STRENGTH + 1]}, E_LIMIT),     # the colours are tested before the strength
]


# ---- the value claim: what error diffusion buys at a fixed palette, from the reference alone ---------------------------------------
RAMP_MAX_BLOCK_RATIO = 0.02           # the 8 x 8 block means' error at strength 256 against the nearest-row map's, on the grey ramp
KODAK_MAX_BLOCK_RATIO = 0.75          # the same on the Kodak crop with the encoder's own palette
KODAK_MAX_PSNR_LOSS_DB = 1.0          # what strength 128 may cost on the crop


def block_mean_error(rgb, palette, idx):
    """the mean squared difference of the non-overlapping 8 x 8 block means of the picture and of its reconstruction"""
    rgb = np.asarray(rgb, np.float64)
    rec = np.asarray(palette, np.float64).reshape(-1, 3)[np.asarray(idx, np.int64)]
    h, w = rgb.shape[0] // 8 * 8, rgb.shape[1] // 8 * 8

    def means(a):
        return a[:h, :w].reshape(h // 8, 8, w // 8, 8, 3).mean(axis=(1, 3))
    return float(((means(rgb) - means(rec)) ** 2).mean())


@functools.lru_cache(maxsize=None)
def ramp():
    """-> (image uint8[64, 256, 3] with value = x in every channel, palette of the greys 0, 85, 170, 255)"""
    img = np.ascontiguousarray(np.repeat(np.tile(np.arange(256, dtype=np.uint8), (64, 1))[:, :, None], 3, axis=2))
    pal = np.array([[v, v, v] for v in (0, 85, 170, 255)], np.uint8)
    img.setflags(write=False)
    pal.setflags(write=False)
    return img, pal


@functools.lru_cache(maxsize=None)
def kodak_crop():
    """-> (kodak_22.png[128:384, 256:512] uint8[256, 256, 3], the 139 rows of compressed_22.rhccq uint8[139, 3])"""
    from PIL import Image
    from roibasedimagecompression_amd.api.uncompression import load_compressed, lossless_decompress
    img = np.asarray(Image.open(os.path.join(GOLDEN, "kodak_22.png")).convert("RGB"), dtype=np.uint8)
    img = np.ascontiguousarray(img[128:384, 256:512])
    palette, _, _ = lossless_decompress(load_compressed(os.path.join(GOLDEN, "compressed_22.rhccq")))
    pal = np.array(palette, np.uint8).reshape(-1, 3)
    assert img.shape == (256, 256, 3) and len(pal) == 139
    img.setflags(write=False)
    pal.setflags(write=False)
    return img, pal


@functools.lru_cache(maxsize=None)
def kodak_reference(strength):
    img, pal = kodak_crop()
    out, sums, b, _ = dither_reference(img, pal, strength)
    for a in (out, sums, b):
        a.setflags(write=False)
    return out, sums, b
