"""Shared cases of the pattern-dither tests (tests/test_palette_pattern_cpu.py, tests/test_gpu_palette_pattern.py): a plain helper module,
not a conftest.

`pattern_reference` is the numpy statement of rhccq_palette_pattern, a direct transcription of its definition: int64 throughout, the
nearest row by the first minimum of the squared distances, the candidates ordered by a stable sort on (luma, row), the Bayer matrices
built by their recursion.  Every case's reference is computed once per process and shared (do not modify what `case`, `reference`
and the other cached functions return)."""
import ctypes as C
import functools
import zlib

import numpy as np

import dither_cases as DC
import remap_cases as RM

SIZES = (2, 4, 8)
MAX_STRENGTH = 256
MAX_ROWS = 4096
CHUNK = {2: 1024, 4: 512, 8: 128}     # pixels a workgroup of the kernel takes at a time (csrc/palette_pattern.h: 128 lanes x 8, 4, 1 pixels)
E_ARG, E_LIMIT = RM.E_ARG, RM.E_LIMIT
strength_table = DC.strength_table


@functools.lru_cache(maxsize=None)
def bayer(n):
    """M_2 = [[0, 2], [3, 1]], M_2n = [[4 M_n, 4 M_n + 2], [4 M_n + 3, 4 M_n + 1]]"""
    if n == 2:
        m = np.array([[0, 2], [3, 1]], np.int64)
    else:
        h = bayer(n // 2)
        m = np.block([[4 * h, 4 * h + 2], [4 * h + 3, 4 * h + 1]])
    m.setflags(write=False)
    return m


def pattern_reference(rgb, palette, strength, size, cls=None, n_classes=0):
    """-> (out int64[H, W], sums int64[n_classes + 1, 3]: row c = {pixels, squared error of out against the original pixel, pixels
    with out != b} over cls == c, the last row over every pixel, b int64[H, W], facts: {"low", "high": targets clamped at 0 / at 255
    per channel, "floor": terms s e + 128 that are negative and no multiple of 256, "luma_ties": pixels with two candidates of
    different rows, different colours and equal luma, "repeats": pixels with a row more than once among their candidates, "ordered":
    the ordered candidates int64[H, W, N]})"""
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    n, N = int(size), int(size) ** 2
    assert n in SIZES
    pal = np.asarray(palette, np.uint8).reshape(-1, 3).astype(np.int64)
    table = np.asarray(strength_table(strength, n_classes), np.int64)
    assert len(table) == n_classes + 1 and table.min() >= 0 and table.max() <= MAX_STRENGTH
    c = np.full(H * W, n_classes, np.int64) if cls is None else np.minimum(np.asarray(cls).reshape(-1).astype(np.int64), n_classes)
    p = rgb.reshape(-1, 3).astype(np.int64)
    s = table[c][:, None]
    e = np.zeros_like(p)
    cand = np.zeros((H * W, N), np.int64)
    facts = {"low": np.zeros(3, np.int64), "high": np.zeros(3, np.int64), "floor": 0}
    for i in range(N):
        term = s * e + 128
        raw = p + (term >> 8)                                                # (numpy's >> on int64 floors toward minus infinity)
        t = np.clip(raw, 0, 255)
        for lo in range(0, H * W, 4096):
            d = ((pal[None, :, :] - t[lo:lo + 4096, None, :]) ** 2).sum(axis=2)
            cand[lo:lo + 4096, i] = d.argmin(axis=1)                         # (the first minimum: the lowest row)
        e = e + p - pal[cand[:, i]]
        facts["low"] += (raw < 0).sum(axis=0)
        facts["high"] += (raw > 255).sum(axis=0)
        facts["floor"] += int(((term < 0) & (term % 256 != 0)).sum())
    luma = (pal * np.array([299, 587, 114], np.int64)).sum(axis=1)
    order = np.lexsort((cand, luma[cand]), axis=1)                           # stable, by luma, then by row; duplicates kept
    ordered = np.take_along_axis(cand, order, axis=1)
    y, x = np.divmod(np.arange(H * W), max(W, 1))
    out = ordered[np.arange(H * W), bayer(n)[y % n, x % n]]
    lo_l, hi_l = luma[ordered[:, :-1]], luma[ordered[:, 1:]]
    differ = (pal[ordered[:, :-1]] != pal[ordered[:, 1:]]).any(axis=2)
    facts["luma_ties"] = int(((lo_l == hi_l) & differ).any(axis=1).sum()) if N > 1 else 0
    facts["repeats"] = int((ordered[:, :-1] == ordered[:, 1:]).any(axis=1).sum())
    facts["ordered"] = ordered.reshape(H, W, N)
    b = RM.remap_reference(rgb, palette)[0].reshape(-1)
    assert np.array_equal(cand[:, 0], b)                                     # the first target is the pixel itself
    dist = ((p - pal[out]) ** 2).sum(axis=1)
    moved = out != b
    sums = np.zeros((n_classes + 1, 3), np.int64)
    for k in range(n_classes):
        sel = c == k
        sums[k] = (sel.sum(), dist[sel].sum(), moved[sel].sum())
    sums[n_classes] = (H * W, dist.sum(), moved.sum())
    return out.reshape(H, W), sums, b.reshape(H, W), facts


_DT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def host_pattern(rgb, pal, cls, n_classes, strength, size, elem_bytes):
    """rhccq_palette_pattern_host in the element width asked for -> (return code, out int64[H, W], sums int64[n_classes + 1, 3])"""
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 3)
    cls = None if cls is None else np.ascontiguousarray(cls, np.uint8).reshape(-1)
    table = np.array(strength_table(strength, n_classes), np.uint32)
    idx = np.full(max(H * W, 1), 0xAB, _DT[elem_bytes])
    sums = np.full((n_classes + 1, 3), 0x5555, np.uint64)                  # (the call zeroes them)
    rc = lib.rhccq_palette_pattern_host(_ptr(rgb if rgb.size else np.zeros(3, np.uint8)), H, W, _ptr(pal), len(pal), _ptr(cls), n_classes, _ptr(table),
                                        int(size), _ptr(idx), elem_bytes, _ptr(sums))
    return rc, idx[:H * W].astype(np.int64).reshape(H, W), sums.astype(np.int64)


_image = DC._image

# two colours of equal luma (299 * -15 + 587 * 9 + 114 * -7 == 0), the one that sorts higher as a colour in the LOWER row
TIE_A, TIE_B = (115, 91, 107), (100, 100, 100)


def _build():
    """name -> (rgb uint8[H, W, 3], palette uint8[K, 3], cls uint8[H, W] or None, n_classes, strength (a number or a table), size,
    expected out rows or None)"""
    rng = np.random.default_rng(20261021)
    out = {}
    pal37 = RM._palette(rng, 37)
    # the smallest pictures
    for h, w in ((1, 1), (1, 2), (1, 3), (2, 1)):
        out[f"shape{h}x{w}"] = (_image(rng, h, w), pal37, None, 0, 256, 4, None)
    # the edges of the largest matrix: one short of it, exactly it, one more, two and a column / row more
    n = 8
    for h, w in ((n - 1, n - 1), (n, n), (n + 1, n + 1), (2 * n + 1, 2 * n + 1), (n - 1, 2 * n + 1), (2 * n + 1, n - 1), (n, n + 1), (n + 1, n)):
        out[f"edge{h}x{w}"] = (_image(rng, h, w), pal37, None, 0, 256, 8, None)
    # more than two chunks of every size's kernel, the width no multiple of 8 or of n: rows and columns from the linear index across chunks
    img = _image(rng, 3, 701)
    for n in SIZES:
        out[f"chunks3x701_n{n}"] = (img, pal37, None, 0, 256, n, None)
    # palette sizes: one row, the 1-byte edge and the first 2-byte size, sizes around 1024, the device's cap
    for K in (1, 2, 3, 255, 256, 257, 1023, 1025, 4096):
        pal = RM._palette(rng, K, levels=256 if K % 2 else 6)
        out[f"K{K}"] = (_image(rng, 13, 45), pal, None, 0, 256, 4, None)
    # a palette far inside the gamut under black and white stripes: the error piles up and the target clamps at both ends
    img = np.zeros((9, 70, 3), np.uint8)
    img[:, 35:] = 255
    img[4:] = 255 - img[4:]
    out["clamp"] = (img, np.array([[100, 100, 100], [150, 150, 150]], np.uint8), None, 0, 256, 4, None)
    # floor against truncation: every pixel is 11 between the rows 13 and 9.  c_0 is the tie's lowest row 0 (13) and leaves e = -2; at
    # strength 128 the term is -128: floored it moves the target to 10 and row 1 (9) wins, truncated the target stays 11 and row 0 would.
    # Then e = 0 and the two steps repeat: candidates 0, 1, 0, 1, ordered by luma 1, 1, 0, 0, picked by [[0, 2], [3, 1]]
    img = np.zeros((2, 2, 3), np.uint8)
    img[..., 0] = 11
    out["floor"] = (img, np.array([[13, 0, 0], [9, 0, 0]], np.uint8), None, 0, 128, 2, [[1, 0], [0, 1]])
    # luma ties: rows 0 and 1 have equal luma and different colours, a pixel between them takes both; row 2 repeats row 0's colour (never
    # the nearest: ties go to the lowest row) and rows 3 and 4 are far away.  Equal luma is ordered by row
    img = np.clip(np.array([108, 95, 104]) + rng.integers(-3, 4, (9, 11, 3)), 0, 255).astype(np.uint8)
    out["luma_tie"] = (img, np.array([TIE_A, TIE_B, TIE_A, [0, 0, 0], [255, 255, 255]], np.uint8), None, 0, 256, 4, None)
    # strengths, for every size, on a palette with duplicate rows
    pal = RM._palette(rng, 60, levels=6)
    img = _image(rng, 21, 90)
    for n in SIZES:
        for s in (0, 1, 128, 256):
            out[f"strength{s}_n{n}"] = (img, pal, None, 0, s, n, None)
    # class strengths: 2 classes, one of strength 0, the class values 3 and 255 take the last entry; 16 classes
    img = _image(rng, 19, 93)
    cls = rng.integers(0, 4, img.shape[:2]).astype(np.uint8)
    cls[rng.random(img.shape[:2]) < 0.05] = 255
    out["classes2"] = (img, pal37, cls, 2, [0, 256, 128], 4, None)
    out["classes16"] = (img, pal37, rng.integers(0, 18, img.shape[:2]).astype(np.uint8), 16, [16 * k for k in range(17)], 2, None)
    return out


_CASES = None


def names():
    global _CASES
    if _CASES is None:
        _CASES = _build()
        for rgb, pal, cls, _, _, _, _ in _CASES.values():
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
    rgb, pal, cls, nc, strength, size, expect = case(name)
    out, sums, b, facts = pattern_reference(rgb, pal, strength, size, cls, nc)
    if expect is not None:
        assert out.tolist() == expect, name
    if name.startswith("chunks"):
        assert rgb.shape[0] * rgb.shape[1] > 2 * CHUNK[size] and rgb.shape[1] % 8 and rgb.shape[1] % size
    if name == "clamp":
        assert (facts["low"] > 0).all() and (facts["high"] > 0).all(), facts
    if name == "floor":
        assert facts["floor"] > 0 and facts["ordered"][0, 0].tolist() == [1, 1, 0, 0]
    if name == "luma_tie":
        ordered = facts["ordered"]
        both = ((ordered == 0).any(axis=2) & (ordered == 1).any(axis=2))
        assert facts["luma_ties"] > 0 and facts["repeats"] > 0 and both.any()
        pair = np.isin(ordered, (0, 1))                                      # among the two rows of equal luma the order is by row
        assert all((np.diff(o[m]) >= 0).all() for o, m in zip(ordered.reshape(-1, ordered.shape[2]), pair.reshape(-1, ordered.shape[2])))
        assert tuple(pal[0]) > tuple(pal[1]) and not (ordered == 2).any()    # (not by colour; a repeated colour's higher row never wins)
    if name.startswith("strength256"):
        assert facts["floor"] > 0 and sums[-1, 2] > 0
    if name.startswith("strength0"):
        assert np.array_equal(out, b) and sums[-1, 2] == 0
    if name == "classes2":
        c = np.asarray(cls)
        assert (c == 3).any() and (c == 255).any() and sums[0, 2] == 0 and sums[1, 2] > 0
    for a in (out, sums, b):
        a.setflags(write=False)
    return out, sums, b, facts


def index_bytes(K):
    return RM.index_bytes(K)


# the argument errors of rhccq_palette_pattern_host: (what, overrides of a valid call, return code).  A valid call: 2 x 2 pixels, K = 3, no
# class map, n_classes = 0, strength [5], size 4, 2-byte indices; "cls": True asks for a valid class map; "strength": a table or None (NULL).
ERRORS = DC.ERRORS + [
    ("size 0", {"size": 0}, E_ARG),
    ("size 1", {"size": 1}, E_ARG),
    ("size 3", {"size": 3}, E_ARG),
    ("size 16", {"size": 16}, E_ARG),
    ("size -4", {"size": -4}, E_ARG),
    ("K = 65537 with a bad size", {"K": 65537, "size": 3}, E_LIMIT),                 # the colours are tested before the size too
]


# ---- the value claims: what the pattern buys at a fixed palette, from the references alone ---------------------------------------------
RAMP_MAX_BLOCK_RATIO = 0.02           # the 8 x 8 block means' error at n = 4, strength 256 against the nearest-row map's, on the grey ramp
RAMP_MAX_BYTES_RATIO = 0.25           # zlib-9 bytes of the ramp's index map against Floyd-Steinberg 256's
KODAK_MAX_BLOCK_RATIO = 0.75          # the block means' error at n = 4, strength 128 against the nearest-row map's, on the Kodak crop


def map_bytes(idx):
    return len(zlib.compress(np.asarray(idx).astype(np.uint8).tobytes(), 9))


@functools.lru_cache(maxsize=None)
def ramp_reference(size, strength):
    img, pal = DC.ramp()
    out, sums, b, _ = pattern_reference(img, pal, strength, size)
    for a in (out, sums, b):
        a.setflags(write=False)
    return out, sums, b


@functools.lru_cache(maxsize=None)
def kodak_reference(size, strength):
    img, pal = DC.kodak_crop()
    out, sums, b, _ = pattern_reference(img, pal, strength, size)
    for a in (out, sums, b):
        a.setflags(write=False)
    return out, sums, b


@functools.lru_cache(maxsize=None)
def stability():
    """kodak_crop()[64:192, 64:192] with its 139 rows and a copy with fixed-seed noise of -1..1 per channel -> (the share of pixels whose
    index differs between the two frames for the nearest-row map, for pattern n = 4 s = 128, for Floyd-Steinberg 256)"""
    img, pal = DC.kodak_crop()
    a = np.ascontiguousarray(img[64:192, 64:192])
    noise = np.random.default_rng(1).integers(-1, 2, a.shape)
    b = np.clip(a.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    near = [RM.remap_reference(f, pal)[0].reshape(-1) for f in (a, b)]
    pat = [pattern_reference(f, pal, 128, 4)[0] for f in (a, b)]
    fs = [DC.dither_reference(f, pal, 256)[0] for f in (a, b)]
    return tuple(float((u != v).mean()) for u, v in (near, pat, fs))
