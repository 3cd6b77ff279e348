"""Shared cases of the run-carrying remap tests (tests/test_palette_runs_cpu.py, tests/test_gpu_palette_runs.py): a plain helper
module, not a conftest.

`runs_reference` is the numpy statement of rhccq_palette_runs: b from remap_cases.remap_reference, then a loop over the columns
vectorised over the image rows, int64 squared distances.  Every case's reference is computed once per process and shared (do not
modify what `case`, `reference` and `grid_case` return)."""
import functools
import os
import zlib

import numpy as np

import remap_cases as RM
from roibasedimagecompression_amd import ops

ROWS, COLS = ops.palette_runs_tile()  # image rows a workgroup walks, columns of the tile it stages: the cases sit at their edges
T = RM.T
MAX_SLACK = 3 * 255 ** 2
E_ARG, E_LIMIT = RM.E_ARG, RM.E_LIMIT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def slack_table(slack, n_classes):
    return [int(slack)] * (n_classes + 1) if np.ndim(slack) == 0 else [int(v) for v in slack]


def runs_reference(rgb, palette, slack, cls=None, n_classes=0, b=None):
    """-> (out int64[H, W], sums int64[n_classes + 1, 3]: row c = {pixels, squared error of out, pixels with out != b} over cls == c,
    the last row over every pixel, b int64[H, W]).  `b`: the nearest-row map when the caller has it already."""
    rgb = np.asarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    px = rgb.astype(np.int64)
    pal = np.asarray(palette, np.uint8).reshape(-1, 3).astype(np.int64)
    table = np.asarray(slack_table(slack, n_classes), np.int64)
    assert len(table) == n_classes + 1 and table.min() >= 0 and table.max() <= MAX_SLACK
    if b is None:
        b = RM.remap_reference(rgb, palette)[0]
    b = np.asarray(b, np.int64).reshape(H, W)
    db = ((px - pal[b]) ** 2).sum(axis=2)
    c = np.full((H, W), n_classes, np.int64) if cls is None else np.minimum(np.asarray(cls).reshape(H, W).astype(np.int64), n_classes)
    limit = db + table[c]
    out = b.copy()
    for x in range(1, W):
        carried = out[:, x - 1]
        keep = ((px[:, x] - pal[carried]) ** 2).sum(axis=1) <= limit[:, x]
        out[:, x] = np.where(keep, carried, b[:, x])
    dist = ((px - pal[out]) ** 2).sum(axis=2)
    moved = out != b
    sums = np.zeros((n_classes + 1, 3), np.int64)
    for k in range(n_classes):
        sel = c == k
        sums[k] = (sel.sum(), dist[sel].sum(), moved[sel].sum())
    sums[n_classes] = (H * W, dist.sum(), moved.sum())
    return out, sums, b


def _image(rng, pal, h, w, spread=6):
    """a picture of horizontal stretches around palette rows, so that runs start, hold and break"""
    pal = np.asarray(pal, np.int64)
    rows = rng.integers(0, len(pal), (h, -(-w // 5)))
    base = np.repeat(pal[rows], 5, axis=1)[:, :w]
    return np.clip(base + rng.integers(-spread, spread + 1, (h, w, 3)), 0, 255).astype(np.uint8)


def _build():
    """name -> (rgb uint8[H, W, 3], palette uint8[K, 3], cls uint8[H, W] or None, n_classes, slack (a number or a table),
    expected out rows or None)"""
    rng = np.random.default_rng(20261019)
    out = {}
    pal37 = RM._palette(rng, 37)
    # shape edges: one column, one row, the lanes of a wave, the staging tile's width, the rows of a workgroup
    shapes = [(5, 1), (1, 70), (63, 7), (64, 7), (65, 7), (3, COLS - 1), (3, COLS), (3, COLS + 1), (ROWS + 1, COLS + 3), (2 * ROWS, 2 * COLS),
              (1, 1)]
    for h, w in shapes:
        out[f"shape{h}x{w}"] = (_image(rng, pal37, h, w), pal37, None, 0, 900, None)
    # a run that survives two staging-tile boundaries: rows 0 and 1 of the palette are 3 apart, the noise moves b between them, and
    # every pixel is within the slack of either, so each image row stays at its first index
    pal = np.array([[100, 100, 100], [103, 100, 100], [250, 10, 10]], np.uint8)
    w = 2 * COLS + 5
    img = np.clip(np.array([101, 100, 100]) + rng.integers(-2, 3, (ROWS + 3, w, 3)), 0, 255).astype(np.uint8)
    out["run_across_tiles"] = (img, pal, None, 0, 64, "constant")
    # a break exactly at the boundary: columns from COLS on sit on the far row, at any slack below the distance
    img = img.copy()
    img[:, COLS:] = (250, 10, 10)
    out["break_at_tile"] = (img, pal, None, 0, 64, "break")
    # the tie: [11, 0, 0] is 1 from both rows; b is row 0 (the lowest), the carried row 1 wins at slack 0
    out["tie"] = (np.array([[[12, 0, 0], [11, 0, 0], [11, 0, 0]]], np.uint8), np.array([[10, 0, 0], [12, 0, 0]], np.uint8), None, 0, 0, [[1, 1, 1]])
    # exactly at db + slack and at db + slack + 1 (slack 1): [1, 0, 0] is 1 from the carried row 0 and 0 from b = 1 (kept);
    # [1, 1, 0] is 2 from row 0 and 0 from b = 2 (broken)
    pal = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0]], np.uint8)
    img = np.array([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [1, 0, 0]]], np.uint8)
    out["at_the_limit"] = (img, pal, None, 0, 1, [[0, 0, 2], [0, 2, 2]])
    out["at_the_limit_slack0"] = (img, pal, None, 0, 0, [[0, 1, 2], [0, 2, 1]])
    out["at_the_limit_slack2"] = (img, pal, None, 0, 2, [[0, 0, 0], [0, 0, 0]])
    # slack 0 on a palette with duplicate rows (ties), and the largest slack: whole image rows are constant
    pal = RM._palette(rng, 60, levels=6)
    img = _image(rng, pal, 21, 150, spread=30)
    out["slack0"] = (img, pal, None, 0, 0, None)
    out["slack_max"] = (img, pal, None, 0, MAX_SLACK, "constant")
    # palette sizes: one row, two, the 1-byte edge, the first 2-byte size, two remap tiles
    for K in (1, 2, 256, 257, T + 1):
        pal = RM._palette(rng, K, levels=256 if K % 2 else 6)
        out[f"K{K}"] = (_image(rng, pal, 9, 83, spread=12), pal, None, 0, 300, None)
    # class slacks: 2 classes, class values 2 and 3 (and 255) take the last entry
    pal = RM._palette(rng, 300)
    img = _image(rng, pal, ROWS + 7, COLS + 29, spread=20)
    cls = rng.integers(0, 4, img.shape[:2]).astype(np.uint8)
    cls[rng.random(img.shape[:2]) < 0.05] = 255
    out["classes2"] = (img, pal, cls, 2, [0, 2500, 400], None)
    out["classes2_blocks"] = (img, pal, np.repeat(rng.integers(0, 4, (img.shape[0], -(-img.shape[1] // 16))), 16, axis=1)[:, :img.shape[1]].astype(np.uint8),
                              2, [MAX_SLACK, 0, 77], None)
    out["classes16"] = (img, pal, rng.integers(0, 18, img.shape[:2]).astype(np.uint8), 16, [37 * k for k in range(17)], None)
    out["classes_none"] = (img, pal, None, 0, 400, None)
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
    """-> (out int64[H, W], sums int64[n_classes + 1, 3], b int64[H, W]); the properties the rule implies are asserted here once"""
    rgb, pal, cls, nc, slack, expect = case(name)
    out, sums, b = runs_reference(rgb, pal, slack, cls, nc)
    if expect == "constant":
        assert (out == out[:, :1]).all() and (out[:, 0] == b[:, 0]).all(), name
    elif expect == "break":
        assert (out[:, :COLS] == out[:, :1]).all() and (out[:, COLS:] == 2).all() and (b[:, 0] != 2).all(), name
    elif expect is not None:
        assert out.tolist() == expect, name
    if name == "run_across_tiles":
        assert len(np.unique(b)) == 2 and sums[-1, 2] > 0, name                    # (the run is a carried one, not b's own)
    if name == "tie":
        assert b.tolist() == [[1, 0, 0]] and sums[-1, 1] == RM.remap_reference(rgb, pal)[1][-1, 1]
    for a in (out, sums, b):
        a.setflags(write=False)
    return out, sums, b


def index_bytes(K):
    return RM.index_bytes(K)


# ---- many workgroups, ragged last tiles in both directions ---------------------------------------------------------------------------
GRID_CASES = RM.GRID_CASES
GRID_SLACK = [30, 3000, 400]


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """remap_cases.grid_case (2200 x 2049, 2 classes with the values 2 and 3 outside) -> (rgb, palette, cls, n_classes, slack table,
    reference out, reference sums); b is the grid case's own reference"""
    rgb, pal, cls, nc, b, _ = RM.grid_case(name)
    out, sums, _ = runs_reference(rgb, pal, GRID_SLACK, cls, nc, b=b)
    out.setflags(write=False)
    sums.setflags(write=False)
    return rgb, pal, cls, nc, GRID_SLACK, out, sums


# the argument errors of rhccq_palette_runs: (what, overrides of a valid call, return code).  A valid call: 2 x 2 pixels, K = 3, no
# class map, n_classes = 0, slack [5], 2-byte indices; "cls": True asks for a valid class map; "slack": a table or None (NULL).
ERRORS = [
    ("null rgb", {"rgb": None}, E_ARG),
    ("null palette", {"palette": None}, E_ARG),
    ("null idx_out", {"idx_out": None}, E_ARG),
    ("null sums", {"sums": None}, E_ARG),
    ("null slack", {"slack": None}, E_ARG),
    ("K = 0", {"K": 0}, E_ARG),
    ("K < 0", {"K": -5}, E_ARG),
    ("H < 0", {"H": -1}, E_ARG),
    ("W < 0", {"W": -1}, E_ARG),
    ("n_classes < 0", {"cls": True, "n_classes": -1}, E_ARG),
    ("n_classes = 17", {"cls": True, "n_classes": 17, "slack": [0] * 18}, E_ARG),
    ("n_classes without a class map", {"n_classes": 1, "slack": [0, 0]}, E_ARG),
    ("idx_elem_bytes = 0", {"idx_elem_bytes": 0}, E_ARG),
    ("idx_elem_bytes = 3", {"idx_elem_bytes": 3}, E_ARG),
    ("idx_elem_bytes = 8", {"idx_elem_bytes": 8}, E_ARG),
    ("K = 257 with 1-byte indices", {"K": 257, "idx_elem_bytes": 1}, E_ARG),
    ("slack above 3 * 255^2", {"slack": [MAX_SLACK + 1]}, E_ARG),
    ("a class slack above 3 * 255^2", {"cls": True, "n_classes": 2, "slack": [0, MAX_SLACK + 1, 0]}, E_ARG),
    ("the last slack above 3 * 255^2", {"cls": True, "n_classes": 2, "slack": [0, 0, 1 << 31]}, E_ARG),
    ("K = 65537", {"K": 65537}, E_LIMIT),
    ("K = 65537 with a slack above 3 * 255^2", {"K": 65537, "slack": [MAX_SLACK + 1]}, E_LIMIT),      # the colours are tested before the slack
]


# ---- the value claim: kodak_22 and the palette of its shipped container ----------------------------------------------------------------
KODAK_SLACK = 128
KODAK_MAX_BYTES_RATIO = 0.80          # the run-carrying map's zlib-9 bytes against the nearest-row map's
KODAK_MAX_PSNR_LOSS_DB = 1.2


@functools.lru_cache(maxsize=None)
def kodak():
    """-> (image uint8[512, 768, 3], palette uint8[139, 3], b, out at KODAK_SLACK, sums of out)"""
    from PIL import Image
    from roibasedimagecompression_amd.api.uncompression import load_compressed, lossless_decompress
    img = np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, "kodak_22.png")).convert("RGB"), dtype=np.uint8))
    palette, _, _ = lossless_decompress(load_compressed(os.path.join(GOLDEN, "compressed_22.rhccq")))
    pal = np.array(palette, np.uint8).reshape(-1, 3)
    assert len(pal) <= 256
    out, sums, b = runs_reference(img, pal, KODAK_SLACK)
    for a in (img, pal, out, sums, b):
        a.setflags(write=False)
    return img, pal, b, out, sums


def index_bytes_zlib9(idx):
    return len(zlib.compress(np.asarray(idx).astype(np.uint8).tobytes(), 9))
