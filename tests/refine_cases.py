"""Shared cases of the palette refinement tests (tests/test_palette_refine_cpu.py, tests/test_gpu_palette_refine.py): a plain helper
module, not a conftest.

`refine_reference` is the numpy statement of rhccq_palette_refine (include/rhccq.h): per iteration the assignment of
remap_cases.remap_reference, the sums N, S, E with np.add.at on int64, the update (2 S + N) // (2 N) for rows with N > 0, and the stop
after the first iteration that changes no row.  Every case's reference is computed once per process and shared (do not modify what
`case` and `reference` return)."""
import functools

import numpy as np

import remap_cases as RM
from roibasedimagecompression_amd import ops, synth

T = RM.T                              # the remap's palette tile
L = ops.palette_refine_lds_rows()     # the largest palette whose accumulators live in LDS
E_ARG, E_LIMIT = RM.E_ARG, RM.E_LIMIT
CHUNK = 256 * 8                       # pixels a workgroup takes at a time


def pixel_weights(cls, weights, n):
    """int64[n]: weights[cls] where cls < n_classes, weights[n_classes] elsewhere and everywhere without a class map"""
    if weights is None:
        return np.ones(n, np.int64)
    w = np.asarray(weights, np.int64)
    nc = len(w) - 1
    if cls is None or nc == 0:
        return np.full(n, w[nc], np.int64)
    c = np.asarray(cls).reshape(-1).astype(np.int64)
    return w[np.where(c < nc, c, nc)]


def refine_reference(rgb, palette, cls=None, weights=None, max_iter=8, mult=None, trace=None):
    """-> (palette uint8[K, 3], history int64[max_iter, 2], n_iter).  mult: an int64 multiplicity per pixel (a histogram's counts:
    a pixel that stands for mult equal pixels of its class), multiplied into the weights.  trace: a list that receives
    (assignment, palette) after every iteration."""
    px8 = np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1, 3))
    px = px8.astype(np.int64)
    pal = np.array(np.asarray(palette, np.uint8).reshape(-1, 3))
    n, K = len(px), len(pal)
    w = pixel_weights(cls, weights, n)
    if mult is not None:
        w = w * np.asarray(mult, np.int64)
    history = np.zeros((max_iter, 2), np.int64)
    n_iter = 0
    if n == 0:
        return pal, history, 0
    for i in range(max_iter):
        idx, _ = RM.remap_reference(px8, pal)
        dist = ((px - pal.astype(np.int64)[idx]) ** 2).sum(axis=1)
        N = np.zeros(K, np.int64)
        S = np.zeros((K, 3), np.int64)
        np.add.at(N, idx, w)
        np.add.at(S, idx, w[:, None] * px)
        new = pal.copy()
        m = N > 0
        new[m] = ((2 * S[m] + N[m, None]) // (2 * N[m, None])).astype(np.uint8)
        changed = int((new != pal).any(axis=1).sum())
        history[i] = (int((w * dist).sum()), changed)
        pal = new
        n_iter = i + 1
        if trace is not None:
            trace.append((idx, pal.copy()))
        if changed == 0:
            break
    return pal, history, n_iter


def _case(rgb, pal, cls=None, weights=None, max_iter=4, expect=None, first=None):
    """expect: the final palette rows {row: [r, g, b]}; first: the row pixel 0 goes to in the first iteration"""
    return {"rgb": np.asarray(rgb, np.uint8), "pal": np.asarray(pal, np.uint8), "cls": cls, "weights": weights, "max_iter": max_iter,
            "expect": expect, "first": first}


def _build():
    rng = np.random.default_rng(20261018)
    out = {}
    pool = synth.photo(64, 128, 11).reshape(-1, 3)
    pal37 = pool[rng.choice(len(pool), 37, replace=False)]
    for n in (0, 1, 63, 64, 65, 257, CHUNK + 301, 3 * CHUNK):
        out[f"px{n}"] = _case(pool[rng.permutation(len(pool))[:n]], pal37)
    for h, w in ((1, 1), (1, 67), (37, 53)):
        out[f"shape{h}x{w}"] = _case(RM._near(rng, pal37, h * w, spread=9).reshape(h, w, 3), pal37)
    for K in sorted({1, 2, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, L - 1, L, L + 1}):
        pal = RM._palette(rng, K, levels=256 if K % 2 else 6)           # even K: duplicate rows in several tiles
        px = np.concatenate([RM._near(rng, pal, 300, spread=9), rng.integers(0, 256, (89, 3)).astype(np.uint8)])
        out[f"K{K}"] = _case(px, pal, max_iter=3)
    pal = RM._palette(rng, 65536)
    out["K65536"] = _case(RM._near(rng, pal, 64 * 64, spread=3).reshape(64, 64, 3), pal, max_iter=2)
    # rounding to nearest, halves up (K = 1)
    out["round_half_up"] = _case([[10, 0, 0], [11, 0, 0]], [[0, 0, 0]], expect={0: [11, 0, 0]})
    out["round_down"] = _case([[10, 0, 0], [10, 0, 0], [11, 0, 0]], [[0, 0, 0]], expect={0: [10, 0, 0]})
    out["round_weighted"] = _case([[10, 4, 0], [12, 9, 0]], [[0, 0, 0]], np.array([0, 1], np.uint8), [3, 1, 1],   # 42 / 4 = 10.5, 21 / 4 = 5.25
                                  expect={0: [11, 5, 0]})
    # ties decide which row moves: remap_cases' constructions (equal distances inside a tile and across rows T-1 and T) with a
    # second pixel next to the filler rows
    for name in ("tie", "tie_reversed", "boundary_tie", "boundary_tie_reversed", "boundary_duplicate", "boundary_nearer_looking",
                 "boundary_three_tiles", "boundary_later_strictly_nearer"):
        px, pal, _, _, want = RM.case(name)
        out[name] = _case(np.concatenate([px, np.array([[201, 200, 199]], np.uint8)]), pal, max_iter=3, first=want[0])
    # 64-bit sums: S = 262144 * 255 * 255 > 2^32
    out["white_on_black"] = _case(np.full((512, 512, 3), 255, np.uint8), np.zeros((1, 3), np.uint8), None, [255], max_iter=2,
                                  expect={0: [255, 255, 255]})
    # class maps and weights
    wts = {1: [1, 0], 2: [0, 255, 1], 16: [int(v) for v in rng.integers(0, 256, 17)]}
    wts[16][:3] = [0, 1, 255]
    for nc in (1, 2, 16):
        img, pal, cls, _, _ = RM.case(f"classes{nc}")
        out[f"classes{nc}"] = _case(img, pal, cls, wts[nc], max_iter=3)
    img, pal, cls, _, _ = RM.case("classes_all_255")
    out["classes_all_255"] = _case(img, pal, cls, [0, 0, 7], max_iter=3)
    # early stop
    photo = synth.photo(64, 64, 3)
    flat = photo.reshape(-1, 3)
    out["early_stop"] = _case(photo, flat[np.random.default_rng(1).choice(len(flat), 1025, replace=False)], max_iter=16)
    return out


_CASES = None


def names():
    global _CASES
    if _CASES is None:
        _CASES = _build()
        for c in _CASES.values():
            for a in (c["rgb"], c["pal"], c["cls"]):
                if a is not None:
                    a.setflags(write=False)
    return list(_CASES)


def case(name):
    names()
    return _CASES[name]


def later_duplicates(pal):
    """rows equal to an earlier row"""
    keys = (pal[:, 0].astype(np.int64) << 16) | (pal[:, 1].astype(np.int64) << 8) | pal[:, 2]
    _, first = np.unique(keys, return_index=True)
    later = np.ones(len(pal), bool)
    later[first] = False
    return np.nonzero(later)[0]


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    trace = []
    pal, history, n_iter = refine_reference(c["rgb"], c["pal"], c["cls"], c["weights"], c["max_iter"], trace=trace)
    idx, one = trace[0] if trace else (np.zeros(0, np.int64), pal)           # the first iteration's assignment and result
    if c["expect"]:
        for row, want in c["expect"].items():
            assert pal[row].tolist() == want, name
    if c["first"] is not None:
        # the tie decides which row moves: pixel 0 goes to the expected row, and only rows that took a pixel moved
        assert idx[0] == c["first"], name
        idle = np.setdiff1d(np.arange(len(c["pal"])), idx)
        assert np.array_equal(one[idle], c["pal"][idle]), name
        if idx[1] != idx[0]:                                                  # alone in its row: the row becomes the pixel
            assert np.array_equal(one[c["first"]], c["rgb"][0]), name
    dup = later_duplicates(c["pal"])
    if name.startswith("K") and len(c["pal"]) % 2 == 0 and len(c["pal"]) > 216:
        assert len(dup) > 0, name
    # a later duplicate never receives a pixel while its earlier twin stands where it stood: it is unchanged by the first iteration
    # (once the twin has moved, the row is no duplicate any more and may take pixels like any other)
    assert np.array_equal(one[dup], c["pal"][dup]), name
    if name == "white_on_black":
        assert history[0].tolist() == [255 * 262144 * 195075, 1] and 262144 * 255 * 255 > 2 ** 32 and n_iter == 2
    if name == "early_stop":
        assert 2 < n_iter < c["max_iter"], n_iter
    assert (history[n_iter:] == 0).all() and (np.diff(history[:n_iter, 0]) <= 0).all(), name
    pal.setflags(write=False)
    history.setflags(write=False)
    return pal, history, n_iter


# ---- one workgroup, many chunks (device only) ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_workgroup_case():
    """40 chunks of white at weight 255 against (black, mid-grey): with OPT_REFINE_MAX_BLOCKS = 1 one workgroup's own sums pass 2^32
    (40 * 2048 * 255 * 255 = 5.3e9) -> (case, reference)"""
    c = _case(np.full((40, CHUNK, 3), 255, np.uint8), [[0, 0, 0], [128, 128, 128]], None, [255], max_iter=3)
    pal, history, n_iter = refine_reference(c["rgb"], c["pal"], None, c["weights"], c["max_iter"])
    assert 40 * CHUNK * 255 * 255 > 2 ** 32 and pal.tolist() == [[0, 0, 0], [255, 255, 255]] and n_iter == 2
    return c, (pal, history, n_iter)


# ---- more chunks than workgroups (device only) --------------------------------------------------------------------------------------
GRID_CASES = RM.GRID_CASES            # remap_cases.grid_case: 2200 x 2049 pixels of 512 colours, 4 class values, K = 5 and K = T + 1
GRID_WEIGHTS = [3, 255, 1]            # classes 0 and 1; the values 2 and 3 are outside and take the last weight
GRID_MAX_ITER = 3


@functools.lru_cache(maxsize=None)
def grid_case(name):
    """-> (case, reference).  The reference is computed from the (colour, class) histogram: every distinct pair once, its count
    as a multiplicity.  The sums of the definition are sums over pixels of a function of (colour, class), so this is exact."""
    rgb, pal, cls, _, _, _ = RM.grid_case(name)
    flat = rgb.reshape(-1, 3).astype(np.int64)
    keys = (((flat[:, 0] << 16) | (flat[:, 1] << 8) | flat[:, 2]) << 8) | cls.reshape(-1)
    u, counts = np.unique(keys, return_counts=True)
    colours = np.stack([(u >> 24) & 255, (u >> 16) & 255, (u >> 8) & 255], axis=1).astype(np.uint8)
    ref = refine_reference(colours, pal, (u & 255).astype(np.uint8), GRID_WEIGHTS, GRID_MAX_ITER, mult=counts)
    assert int(counts.sum()) == flat.shape[0] and len(u) <= 512 * 4
    return _case(rgb, pal, cls, GRID_WEIGHTS, GRID_MAX_ITER), ref


# the argument errors of rhccq_palette_refine: (what, overrides of a valid call, return code, device only).  A valid call: 4 pixels,
# K = 3, no class map, weights NULL, max_iter = 2; "cls": True asks for a valid 4-element class map; "misalign": the named buffer
# is passed one byte (history, work) or two bytes (n_iter) off; "work_short": work_bytes is one less than asked for.
ERRORS = [
    ("null rgb", {"rgb": None}, E_ARG, False),
    ("null palette", {"palette": None}, E_ARG, False),
    ("null history", {"history": None}, E_ARG, False),
    ("null n_iter", {"n_iter": None}, E_ARG, False),
    ("null work", {"work": None}, E_ARG, True),
    ("K = 0", {"K": 0}, E_ARG, False),
    ("K < 0", {"K": -5}, E_ARG, False),
    ("n_pixels < 0", {"n_pixels": -1}, E_ARG, False),
    ("n_classes < 0", {"cls": True, "n_classes": -1}, E_ARG, False),
    ("n_classes = 17", {"cls": True, "n_classes": 17, "weights": [1] * 18}, E_ARG, False),
    ("n_classes without a class map", {"n_classes": 1, "weights": [1, 1]}, E_ARG, False),
    ("max_iter = 0", {"max_iter": 0}, E_ARG, False),
    ("max_iter = 65", {"max_iter": 65}, E_ARG, False),
    ("weight < 0", {"weights": [-1]}, E_ARG, False),
    ("weight = 256", {"cls": True, "n_classes": 1, "weights": [256, 1]}, E_ARG, False),
    ("all weights zero", {"cls": True, "n_classes": 2, "weights": [0, 0, 0]}, E_ARG, False),
    ("misaligned history", {"misalign": "history"}, E_ARG, False),
    ("misaligned n_iter", {"misalign": "n_iter"}, E_ARG, False),
    ("misaligned work", {"misalign": "work"}, E_ARG, True),
    ("short workspace", {"work_short": True}, E_ARG, True),
    ("K = 65537", {"K": 65537}, E_LIMIT, False),
    ("max_iter = 0 with a weight of 256", {"max_iter": 0, "cls": True, "n_classes": 1, "weights": [256, 1]}, E_ARG, False),
]
# max_iter is tested before the weights: both give E_ARG, so the device test tells them apart by the case's message
ERROR_MESSAGES = {"max_iter = 0 with a weight of 256": "palette_refine: max_iter must be 1..64"}


# ---- the frames of the encode_sequence test -------------------------------------------------------------------------------------------
SEQ_SHIFT = 20


@functools.lru_cache(maxsize=None)
def drift_frames(shift=SEQ_SHIFT):
    """[A, A', B]: A is remap_cases' red-only frame with its red channel compressed into 1..191, A' is A plus `shift` in red (a
    brightness drift every palette row is off by, with headroom below 255 for shifts up to 40), B the green / blue frame.
    (Compressed into 1..151 the frame cannot be a key frame: its grey range is then 45 and no Canny threshold pair of
    find_best_edges_by_quality finds an edge, which the reference answers with an exception, and so does encode.  1..171 is the
    first of 151, 171, 191 that has edges; 191 keeps a margin.)"""
    a0, _, b, _ = RM.sequence_frames()
    a = a0.copy()
    a[..., 0] = (1 + (a0[..., 0].astype(np.int64) - 1) * 190 // 254).astype(np.uint8)
    a2 = a.copy()
    a2[..., 0] = a[..., 0] + shift
    assert a[..., 0].min() >= 1 and a[..., 0].max() <= 191
    frames = [a, a2, b]
    for f in frames:
        f.setflags(write=False)
    return frames
