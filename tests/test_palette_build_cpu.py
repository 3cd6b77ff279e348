"""rhccq_palette_cells_host and rhccq_palette_build_host (the device kernels' functions run serially: csrc/palette_build.h,
csrc/palette_build.hip) against the numpy / Python-integer reference of tests/build_cases.py, bit for bit: the table, palette, counts,
boxes, splits and k_out; the properties the rule implies; argument errors; the value claim on a shipped artefact.  No GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import build_cases as BC


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _lib():
    from roibasedimagecompression_amd import _lib
    return _lib.load()


def host_cells(rgb, cls=None, n_classes=0, weights=None, into=None):
    """-> (rc, table int64[4, 32, 32, 32]); into: a table to accumulate into (copied), else the call starts from garbage and zeroes it"""
    rgb = np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1, 3))
    cls = None if cls is None else np.ascontiguousarray(cls, np.uint8).reshape(-1)
    w = None if weights is None else np.array(weights, np.int32)
    cells = np.full(BC.SHAPE, 0x5555555555, np.uint64) if into is None else np.array(into, np.uint64)
    rc = _lib().rhccq_palette_cells_host(_ptr(rgb if rgb.size else np.zeros(3, np.uint8)), len(rgb), _ptr(cls), n_classes, _ptr(w),
                                         0 if into is None else 1, _ptr(cells))
    return rc, cells.astype(np.int64)


def host_build(cells, K_target, want_boxes=True, want_splits=True):
    """-> (rc, (k_out, palette, counts, boxes, splits) with the outputs pre-filled, so that unwritten elements show)"""
    cells = np.ascontiguousarray(np.asarray(cells).astype(np.uint64))
    pal = np.full((K_target, 3), 0xAB, np.uint8)
    counts = np.full(K_target, 0x5555, np.uint64)
    boxes = np.full((K_target, 6), 0xCD, np.uint8) if want_boxes else None
    splits = np.full((max(K_target - 1, 1), 3), 0x2B2B, np.int32) if want_splits else None
    k = np.full(1, 0x77, np.int32)
    rc = _lib().rhccq_palette_build_host(_ptr(cells), K_target, _ptr(pal), _ptr(counts), _ptr(boxes), _ptr(splits), _ptr(k))
    return rc, (int(k[0]), pal, counts, boxes, None if splits is None else splits[:K_target - 1])


def test_caps_and_granules_are_exported():
    lib = _lib()
    assert BC.CAP >= 1024 and lib.rhccq_palette_build_bytes() == 33 ** 3 * 4 * 8
    assert BC.CHUNK % BC.BLOCK == 0 and BC.BLOCK % BC.WAVE == 0 and BC.CHUNK > BC.BLOCK > BC.WAVE


@pytest.mark.parametrize("name", BC.pixel_names())
def test_host_cells_equal_reference(name):
    rc, cells = host_cells(*BC.pixel_case(name))
    assert rc == 0 and np.array_equal(cells, BC.pixel_reference(name)), name


def test_host_cells_rgb_at_an_odd_offset():
    rgb = BC.pixel_case("chunk+1")[0]
    buf = np.zeros(rgb.size + 1, np.uint8)
    buf[1:] = rgb.reshape(-1)
    assert buf[1:].ctypes.data % 2 == 1
    cells = np.zeros(BC.SHAPE, np.uint64)
    rc = _lib().rhccq_palette_cells_host(C.c_void_p(buf.ctypes.data + 1), len(rgb), C.c_void_p(0), 0, C.c_void_p(0), 0, _ptr(cells))
    assert rc == 0 and np.array_equal(cells.astype(np.int64), BC.pixel_reference("chunk+1"))


def test_host_cells_accumulate_equals_the_concatenation():
    a, b = BC.pixel_case("classes_1_7"), BC.pixel_case("random_181x181")
    rc, first = host_cells(*a)
    rc2, both = host_cells(*b, into=first)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(both, BC.pixel_reference("classes_1_7") + BC.pixel_reference("random_181x181"))
    # with one weight table the sum is the table of the concatenated pictures
    rgb = np.concatenate([a[0], b[0]])
    rc, first = host_cells(a[0])
    rc2, both = host_cells(b[0], into=first)
    assert rc == 0 and rc2 == 0 and np.array_equal(both, BC.cells_reference(rgb))


def test_host_cells_no_pixels():
    rc, cells = host_cells(np.zeros((0, 3), np.uint8))
    assert rc == 0 and not cells.any()
    rc, cells = host_cells(np.zeros((0, 3), np.uint8), into=BC.pixel_reference("3x5"))
    assert rc == 0 and np.array_equal(cells, BC.pixel_reference("3x5"))


@pytest.mark.parametrize("name", BC.chain_names())
def test_host_build_equals_reference(name):
    cells, K, _ = BC.chain_case(name)
    rc, got = host_build(cells, K)
    assert rc == 0 and BC.same(got, BC.chain_reference(name), K), name
    rc, (k, pal, counts, boxes, splits) = host_build(cells, K, want_boxes=False, want_splits=False)         # the optional outputs
    assert rc == 0 and k == got[0] and np.array_equal(pal, got[1]) and np.array_equal(counts, got[2])


def test_host_build_takes_more_rows_than_the_device_cap():
    cells, _, _ = BC.chain_case("full_cube_cap")
    K = BC.CAP + 40
    rc, got = host_build(cells, K)
    ref = BC.build_reference(cells, K)
    assert rc == 0 and ref["k"] == K and BC.same(got, ref, K)
    assert np.array_equal(ref["splits"][:BC.CAP - 1], BC.chain_reference("full_cube_cap")["splits"])


def test_table_errors_are_returned_by_the_host_form():
    rc, _ = host_build(np.zeros(BC.SHAPE, np.uint64), 4)
    assert rc == BC.E_ARG
    zero_n = np.zeros(BC.SHAPE, np.uint64)
    zero_n[1:] = 7                                                          # sums without weight: still empty
    assert host_build(zero_n, 4)[0] == BC.E_ARG
    assert host_build(BC.limit_table(), 3)[0] == BC.E_LIMIT and BC.build_reference(BC.limit_table(), 3) == BC.E_LIMIT
    assert host_build(BC.big_table(), 3)[0] == 0


# ---- properties ---------------------------------------------------------------------------------------------------------------------------
def _members(cells, boxes):
    """the box of every occupied cell: int64[n_occupied], and the cells' indices; every occupied cell must lie in exactly one box"""
    occ = np.argwhere(np.asarray(cells)[0] != 0)
    inside = np.stack([((occ >= b[:3]) & (occ < b[3:])).all(axis=1) for b in boxes.astype(np.int64)])
    assert (inside.sum(axis=0) == 1).all()
    return inside.argmax(axis=0), occ


@pytest.mark.parametrize("name", ["photo96_k64", "translated_copies", "weighted_classes", "three_cells_ask_8", "full_cube_cap"])
def test_boxes_partition_the_cells_and_counts_add_up(name):
    cells, K, _ = BC.chain_case(name)
    rc, (k, pal, counts, boxes, splits) = host_build(cells, K)
    assert rc == 0
    member, occ = _members(cells, boxes[:k])
    n = np.asarray(cells)[0][tuple(occ.T)].astype(np.int64)
    assert np.array_equal(np.bincount(member, weights=n, minlength=k).astype(np.int64), counts[:k].astype(np.int64))
    assert int(counts.astype(np.int64).sum()) == int(np.asarray(cells)[0].astype(np.int64).sum())
    b = boxes[:k].astype(np.int64)
    assert (b[:, :3] < b[:, 3:]).all() and ((b[:, 3:] - b[:, :3]).prod(axis=1)).sum() == 32 ** 3        # the boxes tile the cube


@pytest.mark.parametrize("name", ["3x5", "classes_0_3_2", "random_181x181"])
def test_error_through_the_boxes_is_the_one_box_error_minus_the_gains(name):
    """exact, in Python integers: sum w |p - mean of p's box|^2 = sum w |p|^2 - sum over boxes |S|^2 / N, and every split lowers it by its gain"""
    rgb, cls, nc, weights = BC.pixel_case(name)
    cells = BC.pixel_reference(name)
    K = 24
    rc, (k, pal, counts, boxes, splits) = host_build(cells, K)
    assert rc == 0 and k > 1
    ref = BC.build_reference(cells, K)
    w = BC.pixel_weights(len(rgb), cls, nc, weights)
    px = rgb.astype(np.int64)
    q = int((w * (px ** 2).sum(axis=1)).sum())
    cell_of = px >> 3
    b = boxes[:k].astype(np.int64)
    inside = np.stack([((cell_of >= bb[:3]) & (cell_of < bb[3:])).all(axis=1) for bb in b])
    assert (inside.sum(axis=0) == 1).all()
    member = inside.argmax(axis=0)
    through = Fraction(q)
    for j in range(k):
        n = int(w[member == j].sum())
        s = [int((w[member == j] * px[member == j, c]).sum()) for c in range(3)]
        if n:
            through -= Fraction(sum(v * v for v in s), n)
    n_all, s_all = int(w.sum()), [int((w * px[:, c]).sum()) for c in range(3)]
    one_box = Fraction(q) - Fraction(sum(v * v for v in s_all), n_all)
    assert through == one_box - sum(Fraction(num, den) for num, den in ref["gains"])
    assert through >= 0 and all(num >= 0 and den > 0 for num, den in ref["gains"])


@pytest.mark.parametrize("name", ["photo96_k64", "translated_copies"])
def test_the_chain_to_one_more_colour_shares_every_earlier_split(name):
    cells, K, _ = BC.chain_case(name)
    _, (k, _, _, _, splits) = host_build(cells, K)
    _, (k1, _, _, _, splits1) = host_build(cells, K + 1)
    assert k == K and k1 == K + 1 and np.array_equal(splits1[:K - 1], splits)


def test_hand_written_chains():
    """the ties of the rule: lowest axis, lowest position, lowest box"""
    rc, (k, pal, counts, boxes, splits) = host_build(BC.chain_case("channel_symmetric")[0], 4)
    assert rc == 0 and k == 4 and splits[0].tolist() == [0, 0, 1] and sorted(pal.tolist()) == [[0, 0, 0], [0, 0, 8], [0, 8, 0], [8, 0, 0]]
    rc, (k, pal, counts, boxes, splits) = host_build(BC.chain_case("equal_gains_two_positions")[0], 3)
    assert rc == 0 and splits.tolist() == [[0, 0, 1], [1, 0, 2]] and pal.tolist() == [[4, 0, 0], [12, 0, 0], [20, 0, 0]] and counts.tolist() == [5, 3, 5]
    rc, (k, pal, counts, boxes, splits) = host_build(BC.chain_case("two_colours_one_cell")[0], 4)
    assert rc == 0 and k == 1 and pal.tolist() == [[21, 21, 21], [0, 0, 0], [0, 0, 0], [0, 0, 0]] and (splits == -1).all()       # (16 + 23 + 23) / 3 = 20.67
    assert boxes[0].tolist() == [0, 0, 0, 32, 32, 32]
    rc, (k, pal, counts, boxes, splits) = host_build(BC.big_table(), 3)
    assert rc == 0 and splits.tolist() == [[0, 0, 2], [1, 0, 31]]          # a float64 or 128-bit comparison splits box 0 second


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def _odd(a):
    return C.c_void_p(a.ctypes.data + 1)


@pytest.mark.parametrize("what,over,code", BC.CELLS_ERRORS, ids=[e[0] for e in BC.CELLS_ERRORS])
def test_host_cells_argument_errors(what, over, code):
    rgb, cells = np.zeros((4, 3), np.uint8), np.zeros(BC.SHAPE[0] * 32 ** 3 + 1, np.uint64)
    cls = np.zeros(4, np.uint8) if over.get("cls") else None
    w = None if over.get("weights") is None else np.array(over["weights"], np.int32)
    p_rgb = _ptr(None if "rgb" in over else rgb)
    p_cells = {"ok": _ptr(cells), None: C.c_void_p(0), "odd": _odd(cells)}[over.get("cells", "ok")]
    rc = _lib().rhccq_palette_cells_host(p_rgb, over.get("n_pixels", 4), _ptr(cls), over.get("n_classes", 0), _ptr(w), 0, p_cells)
    assert rc == code, what


@pytest.mark.parametrize("what,over,code", BC.BUILD_ERRORS, ids=[e[0] for e in BC.BUILD_ERRORS])
def test_host_build_argument_errors(what, over, code):
    a = {"cells": np.zeros(4 * 32 ** 3 + 1, np.uint64), "palette_out": np.zeros((4, 3), np.uint8), "counts_out": np.zeros(5, np.uint64),
         "splits": np.zeros((4, 3), np.int32), "k_out": np.zeros(2, np.int32)}
    a["cells"][:4 * 32 ** 3] = BC.cells_reference(np.array([[0, 0, 0], [100, 7, 7], [250, 250, 1]], np.uint8)).reshape(-1)
    p = {k: {"ok": _ptr(v), None: C.c_void_p(0), "odd": _odd(v)}[over.get(k, "ok")] for k, v in a.items()}
    rc = _lib().rhccq_palette_build_host(p["cells"], over.get("K_target", 4), p["palette_out"], p["counts_out"], C.c_void_p(0), p["splits"], p["k_out"])
    assert rc == code, what


def test_host_accepts_the_valid_calls_the_errors_vary():
    rc, cells = host_cells(np.zeros((4, 3), np.uint8))
    assert rc == 0 and cells[0, 0, 0, 0] == 4 and cells.sum() == 4
    rc, cells = host_cells(np.zeros((4, 3), np.uint8), np.array([0, 1, 1, 9], np.uint8), 1, [0, 2])
    assert rc == 0 and cells[0, 0, 0, 0] == 6
    rc, (k, pal, counts, boxes, splits) = host_build(BC.cells_reference(np.array([[0, 0, 0], [100, 7, 7], [250, 250, 1]], np.uint8)), 4)
    assert rc == 0 and k == 3 and counts.tolist() == [1, 1, 1, 0]


def test_device_entry_points_raise_without_a_gpu():
    """no CPU fallback: Rhccq.palette_cells and ImageEncoder.quantize need the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError
    from roibasedimagecompression_amd.image import ImageEncoder
    from roibasedimagecompression_amd.ops import default_context
    img = np.zeros((4, 4, 3), np.uint8)
    if torch.cuda.is_available():
        assert int(default_context().palette_cells(img)[0, 0, 0, 0]) == 16
        assert ImageEncoder().quantize(img, colours=4)["stats"]["build"] == {"asked": 4, "rows": 1, "cells": 1, "steps": 0}
    else:
        with pytest.raises(RhccqError):
            default_context().palette_cells(img)
        with pytest.raises(RhccqError):
            ImageEncoder().quantize(img, colours=4)


# ---- the value claim ------------------------------------------------------------------------------------------------------------------------
def test_value_claim_on_kodak_22():
    """the reference alone: on kodak_22 at the 139 rows of compressed_22.rhccq the built palette's nearest-row squared error is no larger
    than the artefact palette's (19 483 383 against 24 547 032, 35.95 dB against 34.95 dB, in the numpy trial that proposed the rule)"""
    img, pal, sse_art, built, sse_built, ref = BC.kodak()
    print(f"kodak_22 at {len(pal)} rows: artefact palette SSE {sse_art}, built palette ({ref['k']} rows) SSE {sse_built}")
    assert ref["k"] == len(pal) == 139
    assert sse_built <= sse_art


def test_host_equals_reference_on_kodak_22():
    img, pal, _, built, _, ref = BC.kodak()
    rc, cells = host_cells(img)
    assert rc == 0 and np.array_equal(cells, BC.cells_reference(img))
    rc, got = host_build(cells, len(pal))
    assert rc == 0 and BC.same(got, ref, len(pal))
