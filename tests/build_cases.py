"""Shared cases of the palette build tests (tests/test_palette_build_cpu.py, tests/test_gpu_palette_build.py): a plain helper module, not
a conftest.

`cells_reference` and `build_reference` are the numpy / Python-integer statement of rhccq_palette_cells' and rhccq_palette_build's rule
(include/rhccq.h): the table by bincount, the gains as exact Python integers compared by cross-multiplication.  Every case's reference
is computed once per process and shared (do not modify what `pixel_case`, `chain_case`, the references and `kodak` return)."""
import functools
import math
import os

import numpy as np

import remap_cases as RM
from roibasedimagecompression_amd import ops

E_ARG, E_LIMIT = RM.E_ARG, RM.E_LIMIT
CAP = ops.palette_build_max_rows()             # the most boxes of the device form
BLOCK, CHUNK = ops.palette_cells_granules()    # pixels between two pixels of a lane; pixels of a workgroup at a time
WAVE = 64
MAX_SUM = (1 << 32) - 1
SHAPE = (4, 32, 32, 32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the references ---------------------------------------------------------------------------------------------------------------------
def pixel_weights(n, cls=None, n_classes=0, weights=None):
    w = np.ones(n_classes + 1, np.int64) if weights is None else np.asarray(weights, np.int64)
    assert len(w) == n_classes + 1 and w.min() >= 0 and w.max() <= 255 and w.any()
    c = np.full(n, n_classes, np.int64) if cls is None else np.minimum(np.asarray(cls).reshape(-1).astype(np.int64), n_classes)
    return w[c]


def cells_reference(rgb, cls=None, n_classes=0, weights=None, into=None):
    """-> int64[4, 32, 32, 32]: planes {N, Sr, Sg, Sb} over the cells (r >> 3, g >> 3, b >> 3); into: a table to add to (not modified)"""
    px = np.asarray(rgb, np.uint8).reshape(-1, 3).astype(np.int64)
    w = pixel_weights(len(px), cls, n_classes, weights)
    cell = ((px[:, 0] >> 3) * 32 + (px[:, 1] >> 3)) * 32 + (px[:, 2] >> 3)
    planes = [np.bincount(cell, weights=w, minlength=32768)] + [np.bincount(cell, weights=w * px[:, ch], minlength=32768) for ch in range(3)]
    assert max(p.max() for p in planes) < 2 ** 53                          # (bincount sums in float64: exact below 2^53)
    out = np.stack(planes).astype(np.int64).reshape(SHAPE)
    return out if into is None else out + np.asarray(into, np.int64)


def _table(cells):
    """the summed-volume table int64[4, 33, 33, 33]: T[:, x, y, z] sums the cells below (x, y, z)"""
    T = np.zeros((4, 33, 33, 33), np.int64)
    T[:, 1:, 1:, 1:] = np.asarray(cells).astype(np.int64).cumsum(1).cumsum(2).cumsum(3)
    return T


def _faces(T, lo, hi, a):
    """int64[4, hi[a] - lo[a] + 1]: the box's sums below every coordinate lo[a]..hi[a] of axis a (column 0 is zero, the last the box)"""
    rng = np.arange(lo[a], hi[a] + 1)
    u, w = (a + 1) % 3, (a + 2) % 3

    def at(cu, cw):
        ix = [None] * 3
        ix[a], ix[u], ix[w] = rng, cu, cw
        return T[:, ix[0], ix[1], ix[2]]
    f = at(hi[u], hi[w]) - at(lo[u], hi[w]) - at(hi[u], lo[w]) + at(lo[u], lo[w])
    return f - f[:, :1]


def gain(box, low):
    """(numerator, denominator) of the gain of a cut: box = [N, Sr, Sg, Sb] and low = the same of the lower half, Python integers"""
    N, N1 = box[0], low[0]
    return sum((N * low[c] - N1 * box[c]) ** 2 for c in (1, 2, 3)), N * N1 * (N - N1)


def best_cut(T, lo, hi):
    """-> (num, den, axis, t) of the valid cut of largest gain, ties to the lowest axis, then the lowest t; None: no valid cut"""
    best = None
    for a in range(3):
        if hi[a] - lo[a] < 2:
            continue
        f = _faces(T, lo, hi, a).T.tolist()                                # Python integers from here on
        box = f[-1]
        for t in range(lo[a] + 1, hi[a]):
            low = f[t - lo[a]]
            if low[0] == 0 or low[0] == box[0]:
                continue
            num, den = gain(box, low)
            if best is None or num * best[1] > best[0] * den:
                best = (num, den, a, t)
    return best


def build_reference(cells, K_target):
    """-> dict(k, palette uint8[k, 3], counts int64[k], boxes uint8[k, 6], splits int32[k - 1, 3], gains: [(num, den)] per step), or the
    error code the table itself shows (E_ARG: N all zero, E_LIMIT: its sum above 2^32 - 1)"""
    cells = np.asarray(cells)
    total = sum(int(v) for v in cells[0].reshape(-1))
    if total == 0:
        return E_ARG
    if total > MAX_SUM:
        return E_LIMIT
    T = _table(cells)
    boxes = [([0, 0, 0], [32, 32, 32])]
    cuts = [best_cut(T, *boxes[0])]
    splits, gains = [], []
    while len(boxes) < K_target:
        pick = None
        for j, c in enumerate(cuts):
            if c is not None and (pick is None or c[0] * cuts[pick][1] > cuts[pick][0] * c[1]):
                pick = j
        if pick is None:
            break
        num, den, a, t = cuts[pick]
        lo, hi = boxes[pick]
        up_lo = list(lo)
        up_lo[a] = t
        low_hi = list(hi)
        low_hi[a] = t
        boxes[pick] = (lo, low_hi)
        boxes.append((up_lo, list(hi)))
        cuts[pick] = best_cut(T, *boxes[pick])
        cuts.append(best_cut(T, *boxes[-1]))
        splits.append((pick, a, t))
        gains.append((num, den))
    pal, counts = [], []
    for lo, hi in boxes:
        s = _faces(T, lo, hi, 0)[:, -1].tolist()
        pal.append([(2 * s[c] + s[0]) // (2 * s[0]) for c in (1, 2, 3)])
        counts.append(s[0])
    return {"k": len(boxes), "palette": np.array(pal, np.uint8), "counts": np.array(counts, np.int64),
            "boxes": np.array([lo + hi for lo, hi in boxes], np.uint8), "splits": np.array(splits, np.int32).reshape(-1, 3), "gains": gains}


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pixel_cases():
    """name -> (rgb uint8[n, 3], cls uint8[n] or None, n_classes, weights or None)"""
    rng = np.random.default_rng(20261019)
    out = {}

    def rand(n):
        return rng.integers(0, 256, (n, 3)).astype(np.uint8)
    out["1x1"] = (np.array([[200, 7, 99]], np.uint8), None, 0, None)
    out["3x5"] = (rand(15), None, 0, None)
    for g, what in ((WAVE, "wave"), (BLOCK, "block"), (CHUNK, "chunk")):
        for d in (-1, 0, 1):
            out[f"{what}{d:+d}"] = (RM._near(rng, RM._palette(rng, 9), g + d, spread=20), None, 0, None)
    out["three_chunks_less_one"] = (RM._near(rng, RM._palette(rng, 5), 3 * CHUNK - 1, spread=4), None, 0, None)
    out["one_colour_64x64"] = (np.tile(np.array([[13, 250, 77]], np.uint8), (64 * 64, 1)), None, 0, None)
    corners = np.zeros((300, 3), np.uint8)
    corners[rng.random(300) < 0.4] = 255
    out["corner_cells"] = (corners, None, 0, None)
    out["random_181x181"] = (rand(181 * 181), None, 0, None)
    n = 700
    out["classes_1_7"] = (RM._near(rng, RM._palette(rng, 12), n, spread=30), rng.integers(0, 2, n).astype(np.uint8), 1, [1, 7])
    # a zero-weight class and class values >= n_classes (3, 200: they weigh weights[2])
    out["classes_0_3_2"] = (RM._near(rng, RM._palette(rng, 12), n, spread=30), rng.choice(np.array([0, 1, 2, 3, 200], np.uint8), n), 2, [0, 3, 2])
    out["uniform_weight_255"] = (rand(333), None, 0, [255])
    # more chunks than the kernel starts workgroups (four a CU), so that a workgroup walks a stretch of several chunks
    out["stretches"] = (RM._near(rng, RM._palette(rng, 40), (4 * 256 + 2) * CHUNK + 5, spread=12), None, 0, None)
    return out


def _photo():
    import roimask_cases as RC
    return RC.case("photo96")[1]


def big_table():
    """N summing to 2^32 - 1 over four cells of the r axis, sums at the ends of the 8-bit range.  The first split parts cells {0, 1} (box
    0) from {30, 31} (box 1); the second step compares their cuts, whose gains differ by about 2^-65 of their size: box 1's is the larger
    one, a float64 comparison sees them equal (and would take box 0), and their cross products need more than 128 bits"""
    a1, a2, b1 = (1 << 30) + 12345, (1 << 30) - 54321, (1 << 30) + 777
    b2 = MAX_SUM - a1 - a2 - b1
    while math.gcd(b1, b2) != 1:
        b1, b2 = b1 + 1, b2 - 1
    sa1, sa2 = 1 * a1 + 98765, 14 * a2 + 4321                              # cell 0: r in 0..7, cell 1: r in 8..15
    num_a, den_a = gain([a1 + a2, sa1 + sa2, 0, 0], [a1, sa1, 0, 0])
    # box 1's cut has the gain X^2 / (b1 b2 (b1 + b2)) with X = b1 S2 - b2 S1: the smallest X whose gain is above box 0's
    den_b = b1 * b2 * (b1 + b2)
    X = math.isqrt(num_a * den_b // den_a) + 1
    assert X * X * den_a > num_a * den_b
    # b1 S2 - b2 S1 = X with cell 31's mean near 254: S2 = X / b1 (mod b2)
    r = X * pow(b1, -1, b2) % b2
    sb2 = r + (254 * b2 - r) // b2 * b2
    assert (b1 * sb2 - X) % b2 == 0
    sb1 = (b1 * sb2 - X) // b2
    assert 240 * b1 <= sb1 <= 247 * b1 and 248 * b2 <= sb2 <= 255 * b2
    num_b, den_b2 = gain([b1 + b2, sb1 + sb2, 0, 0], [b1, sb1, 0, 0])
    assert den_b2 == den_b and num_b == X * X
    assert num_b * den_a > num_a * den_b                                   # exactly: box 1 first
    assert not float(num_b) / float(den_b) > float(num_a) / float(den_a)   # in float64: not larger, so box 0 (the lower index) first
    assert (num_b * den_a).bit_length() > 128 and (num_b * den_a).bit_length() <= 242
    cells = np.zeros(SHAPE, np.uint64)
    for cell, n, s in ((0, a1, sa1), (1, a2, sa2), (30, b1, sb1), (31, b2, sb2)):
        cells[0, cell, 0, 0], cells[1, cell, 0, 0] = n, s
    assert int(cells[0].sum()) == MAX_SUM
    return cells


def _chain_cases():
    """name -> (cells [4, 32, 32, 32], K_target, the expected k or None)"""
    rng = np.random.default_rng(20261020)
    px = _pixel_cases()
    out = {}

    def cells_of(rgb):
        return cells_reference(np.asarray(rgb, np.uint8))
    out["K1"] = (cells_of(px["random_181x181"][0]), 1, 1)
    out["two_colours_one_cell"] = (cells_of([[16, 16, 16], [23, 23, 23], [23, 23, 23]]), 4, 1)
    out["three_cells_ask_8"] = (cells_of([[0, 0, 0], [0, 0, 0], [100, 7, 7], [250, 250, 1]]), 8, 3)
    out["channel_symmetric"] = (cells_of(np.repeat(np.array([[8, 0, 0], [0, 8, 0], [0, 0, 8], [0, 0, 0]], np.uint8), 5, axis=0)), 4, 4)
    cluster = rng.integers(0, 40, (400, 3))
    out["translated_copies"] = (cells_of(np.concatenate([cluster, cluster + 128])), 7, 7)
    out["equal_gains_two_positions"] = (cells_of([[4, 0, 0]] * 5 + [[12, 0, 0]] * 3 + [[20, 0, 0]] * 5), 3, 3)
    grid = np.stack(np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij"), axis=-1).reshape(-1, 3)
    out["full_cube_cap"] = (cells_of(grid * 8 + rng.integers(0, 8, grid.shape)), CAP, CAP)
    out["photo96_k64"] = (cells_of(_photo()), 64, 64)
    out["random_181x181_k200"] = (cells_of(px["random_181x181"][0]), 200, 200)
    out["weighted_classes"] = (cells_reference(*px["classes_0_3_2"]), 16, None)
    out["big_entries"] = (big_table(), 3, 3)
    return out


_PIXELS = _CHAINS = None


def pixel_names():
    global _PIXELS
    if _PIXELS is None:
        _PIXELS = _pixel_cases()
        for c in _PIXELS.values():
            for a in c[:2]:
                if a is not None:
                    a.setflags(write=False)
    return list(_PIXELS)


def pixel_case(name):
    pixel_names()
    return _PIXELS[name]


@functools.lru_cache(maxsize=None)
def pixel_reference(name):
    out = cells_reference(*pixel_case(name))
    out.setflags(write=False)
    return out


def chain_names():
    global _CHAINS
    if _CHAINS is None:
        _CHAINS = _chain_cases()
        for c in _CHAINS.values():
            c[0].setflags(write=False)
    return list(_CHAINS)


def chain_case(name):
    chain_names()
    return _CHAINS[name]


@functools.lru_cache(maxsize=None)
def chain_reference(name):
    cells, K, expect_k = chain_case(name)
    ref = build_reference(cells, K)
    assert expect_k is None or ref["k"] == expect_k, name
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    if name == "channel_symmetric":
        assert ref["splits"][0, 1] == 0                                    # the axis tie goes to r
    if name == "equal_gains_two_positions":
        assert ref["splits"][0].tolist() == [0, 0, 1] and ref["gains"][0] == gain([13, 156, 0, 0], [8, 56, 0, 0])     # (the cut at t = 2 has the same gain)
    if name == "translated_copies":
        g = ref["gains"]
        assert ref["splits"][1, 0] == 0 and ref["splits"][2, 0] == 1 and g[1][0] * g[2][1] == g[2][0] * g[1][1]       # equal gains: box 0 first
    if name == "big_entries":
        assert ref["splits"].tolist() == [[0, 0, 2], [1, 0, 31]]
    return ref


def limit_table():
    """big_table() plus one pixel: the sum is 2^32"""
    cells = big_table()
    cells[0, 31, 0, 0] += 1
    cells[1, 31, 0, 0] += 250
    return cells


def same(got, ref, K_target):
    """(k_out, palette [K_target, 3], counts [K_target], boxes [K_target, 6], splits [K_target - 1, 3]) as an entry point wrote them
    against the reference: every byte, the zero rows from k_out on and the -1 behind the last step included"""
    k, pal, counts, boxes, splits = got
    rk = ref["k"]
    assert k == rk
    assert np.array_equal(pal[:rk], ref["palette"]) and not pal[rk:].any()
    assert np.array_equal(np.asarray(counts[:rk]).astype(np.int64), ref["counts"]) and not counts[rk:].any()
    assert np.array_equal(boxes[:rk], ref["boxes"]) and not boxes[rk:].any()
    assert splits.shape == (K_target - 1, 3)
    assert np.array_equal(splits[:rk - 1], ref["splits"]) and (splits[rk - 1:] == -1).all()
    return True


# the argument errors of rhccq_palette_cells: (what, overrides of a valid call, return code).  A valid call: 4 pixels, no class map,
# n_classes = 0, weights NULL, accumulate 0; "cls": True asks for a valid class map; "cells": None = NULL, "odd" = off its alignment
CELLS_ERRORS = [
    ("null rgb", {"rgb": None}, E_ARG),
    ("null cells", {"cells": None}, E_ARG),
    ("misaligned cells", {"cells": "odd"}, E_ARG),
    ("n_pixels < 0", {"n_pixels": -1}, E_ARG),
    ("n_classes < 0", {"cls": True, "n_classes": -1}, E_ARG),
    ("n_classes = 17", {"cls": True, "n_classes": 17, "weights": [1] * 18}, E_ARG),
    ("n_classes without a class map", {"n_classes": 1, "weights": [1, 1]}, E_ARG),
    ("a weight of 256", {"weights": [256]}, E_ARG),
    ("a negative weight", {"cls": True, "n_classes": 1, "weights": [-1, 2]}, E_ARG),
    ("all weights zero", {"cls": True, "n_classes": 1, "weights": [0, 0]}, E_ARG),
    ("2^32 pixels", {"n_pixels": 1 << 32}, E_LIMIT),
    ("2^24 + 65794 pixels of weight 255", {"n_pixels": (1 << 24) + 65794, "weights": [255]}, E_LIMIT),      # 255 n = 2^32 + 254
    ("a weight of 256 on 2^32 pixels", {"n_pixels": 1 << 32, "weights": [256]}, E_ARG),                   # the weights are tested before the limit
]
# of rhccq_palette_build.  A valid call: K_target = 4 on a table of three pixels; "splits": None and "boxes": None are valid (optional)
BUILD_ERRORS = [
    ("null cells", {"cells": None}, E_ARG),
    ("null palette_out", {"palette_out": None}, E_ARG),
    ("null counts_out", {"counts_out": None}, E_ARG),
    ("null k_out", {"k_out": None}, E_ARG),
    ("misaligned cells", {"cells": "odd"}, E_ARG),
    ("misaligned counts_out", {"counts_out": "odd"}, E_ARG),
    ("misaligned splits", {"splits": "odd"}, E_ARG),
    ("misaligned k_out", {"k_out": "odd"}, E_ARG),
    ("K_target = 0", {"K_target": 0}, E_ARG),
    ("K_target < 0", {"K_target": -3}, E_ARG),
    ("K_target = 32769", {"K_target": 32769}, E_LIMIT),
]
# the device form's own: the workspace ("work": None = NULL, "odd" = off its alignment, "short" = one byte too few) and its cap
BUILD_DEVICE_ERRORS = [
    ("null workspace", {"work": None}, E_ARG),
    ("misaligned workspace", {"work": "odd"}, E_ARG),
    ("short workspace", {"work": "short"}, E_ARG),
    ("K_target = cap + 1", {"K_target": CAP + 1}, E_LIMIT),
]


# ---- the value claim: kodak_22 and the palette of its shipped container ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kodak():
    """-> (image uint8[512, 768, 3], the artefact's palette uint8[139, 3], its nearest-row SSE, the built palette of as many rows, its
    nearest-row SSE, the built reference)"""
    from PIL import Image
    from roibasedimagecompression_amd.api.uncompression import load_compressed, lossless_decompress
    img = np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, "kodak_22.png")).convert("RGB"), dtype=np.uint8))
    palette, _, _ = lossless_decompress(load_compressed(os.path.join(GOLDEN, "compressed_22.rhccq")))
    pal = np.array(palette, np.uint8).reshape(-1, 3)
    ref = build_reference(cells_reference(img), len(pal))
    sse_art = int(RM.remap_reference(img, pal)[1][-1, 1])
    sse_built = int(RM.remap_reference(img, ref["palette"])[1][-1, 1])
    img.setflags(write=False)
    return img, pal, sse_art, ref["palette"], sse_built, ref
