"""Shared cases of the palette ladder tests (tests/test_palette_ladder_cpu.py, tests/test_gpu_palette_ladder.py): a plain helper
module, not a conftest.

A case is a picture, a palette, an optional class map and the weight of every class table; the counts a chain runs with are
sum over tables of weight x N, as ImageEncoder.ladder forms them.  The yardsticks are the numpy references of the remap
(remap_cases.remap_reference) and of the reduction (reduce_cases.reduce_reference); nothing here replays a log.  Every case and every
reference is computed once per process and shared (do not modify what they return)."""
import ctypes as C
import functools

import numpy as np

import reduce_cases as RD
import remap_cases as RM
from roibasedimagecompression_amd import ops

E_ARG, E_LIMIT = RM.E_ARG, RM.E_LIMIT
CAP = RD.CAP
CHUNK = 256 * 8                       # pixels a workgroup takes at a time
LDS0, LDS2 = ops.palette_moments_lds_rows(0), ops.palette_moments_lds_rows(2)
EVERY_STEP_MAX_LIVE = 128             # every case here has fewer rows in use (at most 99), so the curve is checked at every step


def _sparse(rng, K, used, n, spread=4):
    """a palette of K rows and n pixels near `used` of them: a large palette (the kernel's LDS threshold) with a short chain"""
    pal = RM._palette(rng, K)
    rows = rng.choice(K, min(used, K), replace=False)
    p = pal[rows[rng.integers(0, len(rows), n)]].astype(np.int64) + rng.integers(-spread, spread + 1, (n, 3))
    return np.clip(p, 0, 255).astype(np.uint8), pal


def _build():
    """name -> {"rgb", "pal", "cls", "n_classes", "weights" (one per table that enters the counts: n_classes + 1 of them)}"""
    rng = np.random.default_rng(20261020)
    out = {}

    def add(name, rgb, pal, cls=None, n_classes=0, weights=None):
        out[name] = {"rgb": rgb, "pal": pal, "cls": cls, "n_classes": n_classes, "weights": weights or [1] * (n_classes + 1)}

    pal3 = np.array([[0, 0, 0], [200, 10, 30], [200, 10, 30]], np.uint8)               # a black row and a duplicate no pixel reaches
    add("1x1_K1", np.array([[[7, 8, 9]]], np.uint8), np.array([[1, 2, 3]], np.uint8))
    add("1x1_K3", np.array([[[190, 20, 30]]], np.uint8), pal3)
    pal2 = np.array([[10, 20, 30], [220, 210, 200]], np.uint8)
    add("1x2049_K2", RM._near(rng, pal2, CHUNK + 1, spread=9).reshape(1, CHUNK + 1, 3), pal2)        # one pixel past a chunk
    pal64 = RM._palette(rng, 64, levels=6)                                             # duplicates; some rows unused
    pal64[5] = 0
    h, w = 3, 2731                                                                     # four chunks, a ragged tail
    cls = (rng.random((h, w)) < 0.4).astype(np.uint8)
    add("3x2731_K64_roi7", RM._near(rng, pal64, h * w, spread=12).reshape(h, w, 3), pal64, cls, 2, [1, 7, 1])
    add("3x2731_K64_roi1", out["3x2731_K64_roi7"]["rgb"], pal64, cls, 2, [1, 1, 1])
    pal257 = RM._palette(rng, 257)                                                     # two-byte indices
    img = RM._near(rng, pal257[:60], 37 * 53, spread=10).reshape(37, 53, 3)
    add("37x53_K257", img, pal257)
    pal300 = RM._palette(rng, 300)
    pal300[17] = pal300[3]
    pal300[0] = 0
    img = RM._near(rng, pal300[:66], 37 * 53, spread=10).reshape(37, 53, 3)
    cls16 = rng.integers(0, 18, (37, 53)).astype(np.uint8)                              # 16 and 17 are outside the 16 classes
    cls16[rng.random((37, 53)) < 0.1] = 255
    add("37x53_K300_c16", img, pal300, cls16, 16, [int(v) for v in rng.integers(1, 5, 17)])
    add("37x53_K300_roi7", img, pal300, (cls16 < 6).astype(np.uint8), 2, [1, 7, 1])
    flat = np.full((33, 67, 3), (90, 140, 200), np.uint8)                               # one winner throughout: the wave-uniform path
    add("flat_K3", flat, np.array([[0, 0, 0], [91, 139, 201], [250, 250, 250]], np.uint8))
    halves = np.zeros((33, 67), np.uint8)
    halves[:, 40:] = 1                                                                  # waves of one winner and two classes
    add("flat_K3_roi7", flat, out["flat_K3"]["pal"], halves, 2, [1, 7, 1])
    for K in (LDS0, LDS0 + 1):                                                          # both sides of the LDS threshold, one table
        rgb, pal = _sparse(rng, K, 48, 37 * 53)
        add(f"37x53_K{K}", rgb.reshape(37, 53, 3), pal)
    for K in (LDS2, LDS2 + 1):                                                          # and with three tables
        rgb, pal = _sparse(rng, K, 48, 37 * 53)
        add(f"37x53_K{K}_roi7", rgb.reshape(37, 53, 3), pal, (rng.random((37, 53)) < 0.3).astype(np.uint8), 2, [1, 7, 1])
    big = RM._palette(rng, LDS0 + 1)                                                    # the wave-uniform path with accumulators in global memory
    big[700] = (91, 139, 201)
    add(f"flat_K{LDS0 + 1}", flat, big)
    add(f"flat_K{LDS2 + 1}_roi7", flat, big[:LDS2 + 1].copy(), halves, 2, [1, 7, 1])
    add("0px_K3", np.zeros((0, 5, 3), np.uint8), pal3)
    add("0px_K3_roi7", np.zeros((0, 5, 3), np.uint8), pal3, np.zeros((0, 5), np.uint8), 2, [1, 7, 1])
    return out


# The nearest-colour search's constructed ties (remap_cases), for the moments pass alone: equal distances inside a tile and across a
# tile boundary, where the lowest row must win.  "expect" holds the indices.  Kept out of names(): no chain runs on them.
TIE_NAMES = ["tie", "tie_reversed", "tie_duplicates", "boundary_tie", "boundary_tie_reversed", "boundary_duplicate", "boundary_nearer_looking",
             "boundary_three_tiles", "boundary_later_strictly_nearer"]


def _build_ties():
    out = {}
    for name in TIE_NAMES:
        rgb, pal, cls, n_classes, expect = RM.case(name)
        assert cls is None and n_classes == 0 and expect is not None and 1 <= len(rgb) <= 3 and len(pal) <= 2 * RM.T + 1
        out[name] = {"rgb": rgb, "pal": pal, "cls": None, "n_classes": 0, "weights": [1], "expect": list(expect)}
    return out


_CASES = None
_TIES = None


def names(pixels=True):
    """pixels: only the cases that have any (a chain needs weight)"""
    global _CASES, _TIES
    if _CASES is None:
        _CASES, _TIES = _build(), _build_ties()
        assert not set(_CASES) & set(_TIES)
        for c in _CASES.values():
            for a in (c["rgb"], c["pal"], c["cls"]):
                if a is not None:
                    a.setflags(write=False)
    return [k for k, c in _CASES.items() if not pixels or c["rgb"].size]


def case(name):
    """a case of names() or of TIE_NAMES"""
    names()
    return _CASES[name] if name in _CASES else _TIES[name]


def table_masks(c):
    """bool[n_classes + 1, n]: the pixels of every table (the last: all)"""
    n = c["rgb"].size // 3
    m = np.ones((c["n_classes"] + 1, n), bool)
    if c["n_classes"]:
        cl = c["cls"].reshape(-1)
        for t in range(c["n_classes"]):
            m[t] = cl == t
    return m


def combine_counts(moments, weights):
    """sum over the tables of weight x N, the "every pixel" table standing for the pixels of no class: with classes, its N minus
    the class tables' N"""
    N = np.asarray(moments)[:, :, 0].astype(np.int64)
    T = len(N)
    rest = N[-1] - N[:-1].sum(axis=0)
    return (np.tensordot(np.asarray(weights[:T - 1], np.int64), N[:-1], axes=1) + weights[T - 1] * rest).astype(np.int64)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (indices int64[n], moments int64[T, K, 5], counts int64[K]) from remap_reference and np.bincount"""
    c = case(name)
    px = c["rgb"].reshape(-1, 3).astype(np.int64)
    K = len(c["pal"])
    idx, _ = RM.remap_reference(c["rgb"], c["pal"]) if len(px) else (np.zeros(0, np.int64), None)
    assert "expect" not in c or idx.tolist() == c["expect"], name
    fields = np.concatenate([np.ones((len(px), 1), np.int64), px, (px * px).sum(axis=1, keepdims=True)], axis=1)
    masks = table_masks(c)
    mom = np.zeros((len(masks), K, 5), np.int64)
    for t, m in enumerate(masks):
        for f in range(5):                                # float64 weights: every partial sum is an integer far below 2^53
            mom[t, :, f] = np.bincount(idx[m], weights=fields[m, f], minlength=K).astype(np.int64)
    counts = combine_counts(mom, c["weights"])
    for a in (idx, mom, counts):
        a.setflags(write=False)
    return idx, mom, counts


def decode_sse(c, idx, map_, palette):
    """int64[T]: per table, the squared error of the pixels shown through palette[map_[idx]], straight from the pixels"""
    px = c["rgb"].reshape(-1, 3).astype(np.int64)
    d = ((px - np.asarray(palette, np.int64)[map_[idx]]) ** 2).sum(axis=1)
    return np.array([int(d[m].sum()) for m in table_masks(c)], np.int64)


def steps_to_check(live):
    if live <= EVERY_STEP_MAX_LIVE:
        return list(range(live))
    return sorted({0, 1, 2, live // 2, live - 2, live - 1})


# ---- the host forms through ctypes ----------------------------------------------------------------------------------------------------
def ptr(a, off=0):
    return C.c_void_p(a.ctypes.data + off) if a is not None else C.c_void_p(0)


def _lib():
    from roibasedimagecompression_amd import _lib as L
    return L.load()


def host_moments(rgb, pal, cls=None, n_classes=0, idx_bytes=None):
    """-> (rc, indices or None, moments int64[T, K, 5]); idx_bytes None: idx_out == NULL"""
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 3)
    cls = None if cls is None else np.ascontiguousarray(cls, np.uint8).reshape(-1)
    n, K = len(rgb), len(pal)
    idx = None if idx_bytes is None else np.full(max(n, 1), 0x55, {1: np.uint8, 2: np.uint16, 4: np.uint32}[idx_bytes])
    mom = np.full((n_classes + 1, K, 5), 0x5555, np.uint64)
    if n == 0:                                            # (an empty array need not have an address)
        rgb, cls = np.zeros((1, 3), np.uint8), None if cls is None else np.zeros(1, np.uint8)
    rc = _lib().rhccq_palette_moments_host(ptr(rgb), n, ptr(pal), K, ptr(cls), n_classes, ptr(idx), idx_bytes or 0, ptr(mom))
    return rc, None if idx is None else idx[:n].astype(np.int64), mom.astype(np.int64)


def host_reduce(pal, counts, target):
    """-> (rc, palette, counts, map, merges int32[max(K - 1, 1), 2], k_out)"""
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 3)
    counts = np.ascontiguousarray(counts).astype(np.uint64)
    K = len(pal)
    pal_out, cnt_out = np.full((target, 3), 0x55, np.uint8), np.full(target, 0x5555, np.uint64)
    map_, merges, k_out = np.full(K, -7, np.int32), np.full((max(K - 1, 1), 2), -1, np.int32), np.full(1, -7, np.int32)
    rc = _lib().rhccq_palette_reduce_host(ptr(pal), ptr(counts), K, target, ptr(pal_out), ptr(cnt_out), ptr(map_), ptr(merges), ptr(k_out))
    return rc, pal_out, cnt_out.astype(np.int64), map_, merges, int(k_out[0])


def host_rung(pal, counts, merges, target):
    """-> (rc, palette, counts, map, k_out)"""
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 3)
    counts = np.ascontiguousarray(counts).astype(np.uint64)
    merges = np.ascontiguousarray(merges, np.int32)
    K = len(pal)
    pal_out, cnt_out = np.full((target, 3), 0x55, np.uint8), np.full(target, 0x5555, np.uint64)
    map_, k_out = np.full(K, -7, np.int32), np.full(1, -7, np.int32)
    rc = _lib().rhccq_palette_rung_host(ptr(pal), ptr(counts), K, ptr(merges), target, ptr(pal_out), ptr(cnt_out), ptr(map_), ptr(k_out))
    return rc, pal_out, cnt_out.astype(np.int64), map_, int(k_out[0])


def host_curve(pal, counts, merges, moments):
    """-> (rc, curve int64[T, K])"""
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 3)
    counts = np.ascontiguousarray(counts).astype(np.uint64)
    merges = np.ascontiguousarray(merges, np.int32)
    mom = np.ascontiguousarray(moments).astype(np.uint64)
    K, T = len(pal), len(mom)
    curve = np.full((T, K), 0x5555, np.uint64)
    rc = _lib().rhccq_palette_curve_host(ptr(pal), ptr(counts), K, ptr(merges), ptr(mom), T, ptr(curve))
    return rc, curve.astype(np.int64)


@functools.lru_cache(maxsize=None)
def host_ladder(name):
    """the host forms end to end -> (counts, merges, curve, live): the chain runs to one row"""
    c = case(name)
    rc, _, mom = host_moments(c["rgb"], c["pal"], c["cls"], c["n_classes"])
    assert rc == 0
    counts = combine_counts(mom, c["weights"])
    rc, _, _, _, merges, k = host_reduce(c["pal"], counts, 1)
    assert rc == 0 and k == 1
    rc, curve = host_curve(c["pal"], counts, merges, mom)
    assert rc == 0
    for a in (counts, merges, curve):
        a.setflags(write=False)
    return counts, merges, curve, int((counts > 0).sum())


# ---- argument errors: (what, overrides of the valid call, return code, where: "both" or "device") -------------------------------------
# moments: the valid call is 4 pixels, K = 3, no class map, 2-byte indices.  "cls": True asks for a valid class map.
MOMENTS_ERRORS = [
    ("null rgb", {"rgb": None}, E_ARG),
    ("null palette", {"palette": None}, E_ARG),
    ("null moments", {"moments": None}, E_ARG),
    ("K = 0", {"K": 0}, E_ARG),
    ("n_pixels < 0", {"n_pixels": -1}, E_ARG),
    ("n_classes < 0", {"cls": True, "n_classes": -1}, E_ARG),
    ("n_classes = 17", {"cls": True, "n_classes": 17}, E_ARG),
    ("n_classes without a class map", {"n_classes": 1}, E_ARG),
    ("idx_elem_bytes = 3", {"idx_elem_bytes": 3}, E_ARG),
    ("K = 257 with 1-byte indices", {"K": 257, "idx_elem_bytes": 1}, E_ARG),
    ("misaligned indices", {"misalign": "idx_out"}, E_ARG),
    ("misaligned moments", {"misalign": "moments"}, E_ARG),
    ("K = 65537", {"K": 65537}, E_LIMIT),
]
MOMENTS_ACCEPTED = [("the valid call", {}), ("null idx_out", {"idx_out": None}), ("null idx_out, any width", {"idx_out": None, "idx_elem_bytes": 3})]
# curve and rung: the valid call is K = 3, counts (1, 2, 3), the log [(0, 1), (-1, -1)], one table (curve), K_target = 2 (rung)
CURVE_ERRORS = [
    ("null palette", {"palette": None}, E_ARG, "both"),
    ("null counts", {"counts": None}, E_ARG, "both"),
    ("null merges", {"merges": None}, E_ARG, "both"),
    ("null moments", {"moments": None}, E_ARG, "both"),
    ("null curve", {"curve": None}, E_ARG, "both"),
    ("null work", {"work": None}, E_ARG, "device"),
    ("K = 0", {"K": 0}, E_ARG, "both"),
    ("n_tables = 0", {"n_tables": 0}, E_ARG, "both"),
    ("n_tables = 18", {"n_tables": 18}, E_ARG, "both"),
    ("misaligned counts", {"misalign": "counts"}, E_ARG, "both"),
    ("misaligned merges", {"misalign": "merges"}, E_ARG, "both"),
    ("misaligned moments", {"misalign": "moments"}, E_ARG, "both"),
    ("misaligned curve", {"misalign": "curve"}, E_ARG, "both"),
    ("misaligned work", {"misalign": "work"}, E_ARG, "device"),
    ("short workspace", {"work_short": True}, E_ARG, "device"),
    ("K = 65537", {"K": 65537}, E_LIMIT, "both"),
    ("K = cap + 1", {"K": CAP + 1}, E_LIMIT, "device"),
]
RUNG_ERRORS = [
    ("null palette", {"palette": None}, E_ARG, "both"),
    ("null counts", {"counts": None}, E_ARG, "both"),
    ("null merges", {"merges": None}, E_ARG, "both"),
    ("null palette_out", {"palette_out": None}, E_ARG, "both"),
    ("null counts_out", {"counts_out": None}, E_ARG, "both"),
    ("null map", {"map": None}, E_ARG, "both"),
    ("null k_out", {"k_out": None}, E_ARG, "both"),
    ("K = 0", {"K": 0}, E_ARG, "both"),
    ("K_target = 0", {"K_target": 0}, E_ARG, "both"),
    ("K_target = K + 1", {"K_target": 4}, E_ARG, "both"),
    ("misaligned counts", {"misalign": "counts"}, E_ARG, "both"),
    ("misaligned counts_out", {"misalign": "counts_out"}, E_ARG, "both"),
    ("misaligned map", {"misalign": "map"}, E_ARG, "both"),
    ("misaligned merges", {"misalign": "merges"}, E_ARG, "both"),
    ("misaligned k_out", {"misalign": "k_out"}, E_ARG, "both"),
    ("K = 65537", {"K": 65537, "K_target": 2}, E_LIMIT, "both"),
    ("K = cap + 1", {"K": CAP + 1, "K_target": 2}, E_LIMIT, "device"),
]
RUNG_DATA_ERRORS = [("every count zero", [0, 0, 0], E_ARG), ("counts add up to 2^32", [1, RD.MAX_SUM - 1, 1], E_LIMIT)]
