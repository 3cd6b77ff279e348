"""Shared cases of the candidate-grid search tests (tests/test_palette_grid_cpu.py, tests/test_gpu_palette_grid.py): a plain helper
module, not a conftest.  The reference of every remap is remap_cases.remap_reference; `lists_reference` is the numpy statement of the
grid's definition (include/rhccq.h).  A case: (rgb, palette, class map or None, n_classes, entries or None = room for every list)."""
import ctypes as C
import functools

import numpy as np

import remap_cases as RM
from roibasedimagecompression_amd import _lib, ops

CELLS, CELL, CAP, CHUNK = 32768, ops.palette_grid_cell(), ops.palette_grid_max_list(), ops.palette_grid_chunk()


def _cases():
    rng = np.random.default_rng(20261126)
    rand = lambda n: rng.integers(0, 256, (n, 3)).astype(np.uint8)
    pal37 = rand(37)
    out = {"K1": (rand(65), rand(1), None, 0, None),
           # (8, 0, 0) is 3 from (5, 0, 0) in cell 0 and from (11, 0, 0) in cell 1: the lower row wins, whichever it is
           "tie_two_cells": (np.array([[8, 0, 0]], np.uint8), np.array([[11, 0, 0], [5, 0, 0]], np.uint8), None, 0, None),
           "duplicates": (RM._near(rng, pal37, 200), np.concatenate([pal37, pal37[::-1], pal37]), None, 0, None),
           "cell_edges": (np.stack(np.meshgrid(*[[0, 7, 8, 255]] * 3), -1).reshape(-1, 3).astype(np.uint8), pal37, None, 0, None)}
    far = np.full((1100, 3), 200, np.uint8)                    # the tied rows 3 and 1030 lie in different tiles of the search
    far[3], far[1030] = (11, 0, 0), (5, 0, 0)
    out["tie_two_tiles"] = (np.array([[8, 0, 0], [200, 200, 201]], np.uint8), far, None, 0, None)
    for n in (1, 63, 65, CHUNK + 1, 3 * CHUNK + 5):
        out[f"px{n}"] = (np.concatenate([RM._near(rng, pal37, n - n // 2, 40), rand(n // 2)]), pal37, None, 0, None)
    for K in (1023, 1025, 4097):
        pal = rand(K)
        out[f"K{K}"] = (np.concatenate([RM._near(rng, pal, 300), rand(89)]), pal, None, 0, None)
    # 1500 rows in [0, 16)^3, drawn from its upper octant [8, 16)^3: for the white cell [248, 255]^3 every row then has dmin <= 3 * 240^2
    # <= U, so the cell's list has all 1500 rows and is above the cap (rows drawn from all of [0, 16)^3 leave it at about 750)
    # 30 more rows in the cell [24, 32) x [0, 8)^2 (from the white cell farther than U, so they change nothing there) with pixels of
    # that cell, whose own list is short: the walk and the queue both get pixels
    dense = np.concatenate([rng.integers(8, 16, (1500, 3)), rng.integers(0, 8, (30, 3)) + (24, 0, 0)]).astype(np.uint8)
    out["over_cap"] = (np.concatenate([255 - rng.integers(0, 8, (700, 3)), rng.integers(0, 8, (500, 3)) + (24, 0, 0)]).astype(np.uint8), dense, None, 0, None)
    out["capacity"] = (rand(3000), pal37, None, 0, 6000)       # the lists of the first cells fill the capacity, the rest is flagged
    out["all_flagged"] = (rand(CHUNK + 77), pal37, None, 0, 0)
    pal300 = rand(300)
    cls = rng.integers(0, 4, 41 * 59).astype(np.uint8)          # 2 and 3 are outside the 2 classes
    out["classes2"] = (RM._near(rng, pal300, 41 * 59, 20), pal300, cls, 2, None)
    out["classes2_capacity"] = (rand(41 * 59), pal300, cls, 2, 40000)
    return out


CASES = _cases()
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    rgb, pal, cls, nc, _ = CASES[name]
    return RM.remap_reference(rgb, pal, cls, nc)


def room(K):
    """entries that hold every list of any K-row palette"""
    return CELLS * min((K + 1) & ~1, CAP)


def ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def pieces(work, entries):
    """the workspace of a grid (uint8 array) as include/rhccq.h lays it out -> cells [32768, 2], U, counts, entries [E, 2], rows [E]"""
    E = max(entries & ~1, 2)
    rows_at = 524288 + (E * 8 + 255) // 256 * 256
    w = np.ascontiguousarray(work)
    return (w[:262144].view(np.uint32).reshape(CELLS, 2), w[262144:393216].view(np.uint32), w[393216:524288].view(np.uint32),
            w[524288:524288 + E * 8].view(np.uint32).reshape(E, 2), w[rows_at:rows_at + E * 2].view(np.uint16))


@functools.lru_cache(maxsize=None)
def host_grid(name):
    """rhccq_palette_grid_host of the case's palette -> (workspace uint8, entries, stats uint64[4])"""
    _, pal, _, _, entries = CASES[name]
    lib = _lib.load()
    entries = room(len(pal)) if entries is None else entries
    work, stats = np.zeros(lib.rhccq_palette_grid_bytes(len(pal), entries), np.uint8), np.zeros(4, np.uint64)
    assert lib.rhccq_palette_grid_host(ptr(pal), len(pal), entries, ptr(work), work.size, ptr(stats)) == 0
    return work, entries, stats


def lists_reference(pal):
    """the definition: member[cell, j] = dmin_j(cell) <= U(cell), and U"""
    cell = np.arange(CELLS)
    dmin, dmax = np.zeros((CELLS, len(pal)), np.int32), np.zeros((CELLS, len(pal)), np.int32)
    for ch, shift in enumerate((10, 5, 0)):
        lo = (((cell >> shift) & 31) * CELL)[:, None]
        c = pal[:, ch].astype(np.int32)[None, :]
        dmin += np.maximum(np.maximum(lo - c, c - (lo + CELL - 1)), 0) ** 2
        dmax += np.maximum(np.abs(c - lo), np.abs(c - (lo + CELL - 1))) ** 2
    U = dmax.min(axis=1)
    return dmin <= U[:, None], U
