"""The candidate-grid search on the host (rhccq_palette_grid_host, rhccq_palette_remap_grid_host: the device kernels' functions run
serially, csrc/palette_grid.hip) against the brute-force reference of tests/remap_cases.py and the numpy statement of the grid's
definition, and the messages of the new Python arguments.  No GPU."""
import numpy as np
import pytest

import grid_cases as G
import remap_cases as RM

_DT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


@pytest.mark.parametrize("name", G.NAMES)
def test_host_remap_through_the_grid_equals_reference(name):
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    rgb, pal, cls, nc, _ = G.CASES[name]
    want_idx, want_sums = G.reference(name)
    work, entries, stats = G.host_grid(name)
    cells = G.pieces(work, entries)[0]
    px = rgb.astype(np.int64)
    flagged = int((cells[(px[:, 0] >> 3) << 10 | (px[:, 1] >> 3) << 5 | px[:, 2] >> 3, 1] == 0).sum())
    for eb in RM.index_bytes(len(pal)):
        idx, sums, over = np.full(len(rgb), 0xAB, _DT[eb]), np.full((nc + 1, 2), 0x55, np.uint64), np.full(1, 0x55, np.uint64)
        rc = lib.rhccq_palette_remap_grid_host(G.ptr(rgb), len(rgb), G.ptr(pal), len(pal), G.ptr(cls), nc, G.ptr(work), entries, G.ptr(idx), eb,
                                               G.ptr(sums), G.ptr(over))
        assert rc == 0, (name, eb)
        assert np.array_equal(idx.astype(np.int64), want_idx) and np.array_equal(sums.astype(np.int64), want_sums), (name, eb)
        assert int(over[0]) == flagged, (name, eb)
    # what the case is there for
    if name == "over_cap":
        assert G.pieces(work, entries)[2][G.CELLS - 1] > G.CAP and 0 < flagged < len(rgb)
    if name in ("capacity", "classes2_capacity"):
        assert 0 < flagged < len(rgb) and stats[0] > 0 and stats[1] > 0 and G.pieces(work, entries)[2].max() <= G.CAP
    if name == "all_flagged":
        assert flagged == len(rgb) and stats.tolist() == [0, G.CELLS, 0, 0]
    if G.CASES[name][4] is None and name not in ("over_cap", "tie_two_tiles"):
        assert flagged == 0 and stats[1] == 0
    if name.startswith("tie"):
        assert want_idx[0] == {"tie_two_cells": 0, "tie_two_tiles": 3}[name]


@pytest.mark.parametrize("name", [n for n in G.NAMES if len(G.CASES[n][1]) <= 300])
def test_host_grid_equals_the_definition(name):
    pal, cap = G.CASES[name][1], G.CASES[name][4]
    work, entries, stats = G.host_grid(name)
    cells, U, counts, ent, rows = G.pieces(work, entries)
    member, want_U = G.lists_reference(pal)
    n = member.sum(axis=1)
    assert np.array_equal(U, want_U) and np.array_equal(counts, n) and n.min() >= 1
    len2 = np.where(n > G.CAP, 0, (n + 1) & ~1)
    off = np.cumsum(len2) - len2
    listed = (n <= G.CAP) & (off + len2 <= (entries & ~1))
    assert np.array_equal(cells[:, 0], np.where(listed, off, 0)) and np.array_equal(cells[:, 1], np.where(listed, n, 0))
    assert stats.tolist() == [listed.sum(), (~listed).sum(), (off + len2)[listed].max(initial=0), n[listed].max(initial=0)]
    assert (cap is None) == bool(listed.all())
    # every listed cell's rows in ascending order, each entry the search's packed row under its position; odd lists padded
    cell, j = np.nonzero(member & listed[:, None])
    pos = np.arange(len(j)) - (np.cumsum(n * listed) - n * listed)[cell]
    at = off[cell] + pos
    p = pal.astype(np.int64)
    assert np.array_equal(rows[at], j)
    assert np.array_equal(ent[at, 0], 0xFFFFFF - (p[j, 0] << 16 | p[j, 1] << 8 | p[j, 2]))
    assert np.array_equal(ent[at, 1], (p[j] ** 2).sum(axis=1) << 12 | pos)
    odd = np.nonzero(listed & (n % 2 == 1))[0]
    last = off[odd] + n[odd]
    assert np.array_equal(rows[last], rows[last - 1]) and np.array_equal(ent[last, 0], ent[last - 1, 0])
    assert np.array_equal(ent[last, 1], ent[last - 1, 1] + 1)


def test_constants_and_sizes():
    from roibasedimagecompression_amd import _lib, ops
    lib = _lib.load()
    assert (ops.palette_grid_cell(), ops.palette_grid_max_list()) == (8, 1024) and G.CHUNK % 256 == 0
    assert lib.rhccq_palette_grid_bytes(5, 0) == lib.rhccq_palette_grid_bytes(5, 3) == 524288 + 256 + 256
    assert lib.rhccq_palette_grid_bytes(5, 1000) == 524288 + 8192 + 2048
    assert [lib.rhccq_palette_grid_bytes(*a) for a in ((0, 4), (65537, 4), (5, -1), (5, G.CELLS * G.CAP + 1))] == [-1] * 4
    assert lib.rhccq_palette_remap_grid_bytes(100) == 512 + 512 and lib.rhccq_palette_remap_grid_bytes(-1) == -1


@pytest.mark.parametrize("over,code", [({"palette": None}, RM.E_ARG), ({"K": 0}, RM.E_ARG), ({"entries": -1}, RM.E_ARG), ({"work_bytes": 1000}, RM.E_ARG),
                                       ({"stats": None}, RM.E_ARG), ({"K": 65537}, RM.E_LIMIT), ({"entries": G.CELLS * G.CAP + 2}, RM.E_LIMIT)],
                         ids=lambda v: str(v))
def test_host_grid_argument_errors(over, code):
    from roibasedimagecompression_amd import _lib
    a = {"palette": np.zeros((3, 3), np.uint8), "K": 3, "entries": 100, "work": np.zeros(600000, np.uint8), "work_bytes": 600000,
         "stats": np.zeros(4, np.uint64)}
    a.update(over)
    rc = _lib.load().rhccq_palette_grid_host(G.ptr(a["palette"]), a["K"], a["entries"], G.ptr(a["work"]), a["work_bytes"], G.ptr(a["stats"]))
    assert rc == code


def test_python_argument_messages():
    """the argument layer needs no device: entries, grid= and search= are tested before anything is launched"""
    import torch
    from roibasedimagecompression_amd import _palette_args as A
    assert A.grid_entries(None, "f") is None and A.grid_entries(np.int64(6), "f") == 6 and A.grid_entries(0, "f") == 0
    with pytest.raises(TypeError, match="palette_grid: entries must be an integer or None, got float"):
        A.grid_entries(6.0, "palette_grid")
    with pytest.raises(TypeError, match="got bool"):
        A.grid_entries(True, "palette_grid")
    for bad in (-1, G.CELLS * G.CAP + 1):
        with pytest.raises(ValueError, match="palette_grid: entries must be 0..33554432"):
            A.grid_entries(bad, "palette_grid")
    pal = torch.zeros((5, 3), dtype=torch.uint8)
    grid = A.PaletteGrid(pal, 10, None, {})
    assert A.grid_arg(None, pal, "f") is None and A.grid_arg(grid, pal, "f") is grid and grid.K == 5 and grid.overflow is None
    with pytest.raises(TypeError, match="palette_remap: grid must be what palette_grid returned, got dict"):
        A.grid_arg({}, pal, "palette_remap")
    with pytest.raises(ValueError, match="palette_remap: the grid was built for a palette of 5 rows on cpu"):
        A.grid_arg(grid, pal[:4], "palette_remap")
    assert A.search_kind("full", "f") == "full" and A.search_kind("grid", "f") == "grid" and A.search_kind(grid, "f") is grid
    for bad in ("Grid", None, 1):
        with pytest.raises(ValueError, match='encode_with_palette: search must be "full", "grid" or a grid from Rhccq.palette_grid'):
            A.search_kind(bad, "encode_with_palette")
