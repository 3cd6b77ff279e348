"""The host forms of the batched palette build path (csrc/palette_batch.hip: rhccq_palette_cells_batch_host, _build_batch_host,
_remap_batch_host, _refine_batch_host) against the per-image references of tests/build_cases.py, remap_cases.py and refine_cases.py, bit
for bit, and the argument errors of all eight entries (the device forms up to where they need a context).  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import build_cases as BC
import refine_cases as RF
import remap_cases as RM

E_ARG, E_LIMIT = BC.E_ARG, BC.E_LIMIT
K_TARGET = 16
WEIGHTS = [0, 3, 2]                    # classes 0 and 1; every other class value weighs the last entry
MAX_ITER = 3
CELLS = 4 * 32 ** 3


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _odd(a):
    return C.c_void_p(a.ctypes.data + 1)


def _lib():
    from roibasedimagecompression_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def batch():
    """four images back to back, an empty one in the middle; image 0 has 15 pixels, so image 1 starts at an odd byte -> (images,
    class maps, px_off, per-image references: cells, build (or the error code), remap on the built palette, refine of it)"""
    rng = np.random.default_rng(20261101)
    images = [BC.pixel_case("3x5")[0], BC.pixel_case("classes_0_3_2")[0], np.zeros((0, 3), np.uint8), BC.pixel_case("chunk+1")[0]]
    maps = [rng.choice(np.array([0, 1, 2, 200], np.uint8), 15), BC.pixel_case("classes_0_3_2")[1], np.zeros(0, np.uint8),
            rng.integers(0, 4, len(images[3])).astype(np.uint8)]
    off = np.concatenate([[0], np.cumsum([len(i) for i in images])]).astype(np.int64)
    assert (off[1] * 3) % 2 == 1 and off[2] == off[3]
    cells = [BC.cells_reference(i, m, 2, WEIGHTS) for i, m in zip(images, maps)]
    built = [BC.build_reference(c, K_TARGET) for c in cells]
    assert built[2] == E_ARG and all(b["k"] >= 2 for b in built if b != E_ARG)
    remap = [None if b == E_ARG else RM.remap_reference(i, b["palette"], m, 2) for i, m, b in zip(images, maps, built)]
    refine = [None if b == E_ARG else RF.refine_reference(i, b["palette"], m, WEIGHTS, MAX_ITER) for i, m, b in zip(images, maps, built)]
    return images, maps, off, cells, built, remap, refine


def _concat(images, maps, lead=0):
    """the concatenated pixels `lead` bytes into their allocation, and the class maps"""
    flat = np.concatenate([i.reshape(-1) for i in images])
    buf = np.zeros(flat.size + lead + 3, np.uint8)
    buf[lead:lead + flat.size] = flat
    return buf, np.ascontiguousarray(np.concatenate(maps))


def _palettes(built, stride, fill=0xAB):
    pal = np.full((len(built), stride, 3), fill, np.uint8)
    k = np.zeros(len(built), np.int32)
    for b, ref in enumerate(built):
        if ref == E_ARG:
            k[b] = E_ARG
        else:
            k[b] = ref["k"]
            pal[b, :ref["k"]] = ref["palette"]
    return pal, k


# ---- the four host forms against the per-image references ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1])
def test_host_cells_batch_equals_the_per_image_reference(lead):
    images, maps, off, cells_ref, _, _, _ = batch()
    buf, cls = _concat(images, maps, lead)
    cells = np.full((4, CELLS), 0x5555555555, np.uint64)
    w = np.array(WEIGHTS, np.int32)
    rc = _lib().rhccq_palette_cells_batch_host(C.c_void_p(buf.ctypes.data + lead), _ptr(off), 4, _ptr(cls), 2, _ptr(w), _ptr(cells))
    assert rc == 0
    for b in range(4):
        assert np.array_equal(cells[b].astype(np.int64).reshape(BC.SHAPE), cells_ref[b]), b
    assert not cells[2].any()


def test_host_cells_batch_without_classes_and_one_image():
    images, _, off, _, _, _, _ = batch()
    buf, _ = _concat(images, [np.zeros(0, np.uint8)])
    cells = np.full((4, CELLS), 0x5555555555, np.uint64)
    assert _lib().rhccq_palette_cells_batch_host(_ptr(buf), _ptr(off), 4, None, 0, None, _ptr(cells)) == 0
    for b in range(4):
        assert np.array_equal(cells[b].astype(np.int64).reshape(BC.SHAPE), BC.cells_reference(images[b])), b
    one = np.full(CELLS, 0x77, np.uint64)
    o1 = np.array([0, len(images[3])], np.int64)
    assert _lib().rhccq_palette_cells_batch_host(_ptr(np.ascontiguousarray(images[3])), _ptr(o1), 1, None, 0, None, _ptr(one)) == 0
    assert np.array_equal(one.astype(np.int64).reshape(BC.SHAPE), BC.pixel_reference("chunk+1"))


@pytest.mark.parametrize("optional", [True, False])
def test_host_build_batch_equals_the_per_image_reference(optional):
    _, _, _, cells_ref, built, _, _ = batch()
    cells = np.ascontiguousarray(np.stack(cells_ref).astype(np.uint64))
    pal = np.full((4, K_TARGET, 3), 0xAB, np.uint8)
    counts = np.full((4, K_TARGET), 0x5555, np.uint64)
    boxes = np.full((4, K_TARGET, 6), 0xCD, np.uint8) if optional else None
    splits = np.full((4, K_TARGET - 1, 3), 0x2B2B, np.int32) if optional else None
    k = np.full(4, 0x77, np.int32)
    rc = _lib().rhccq_palette_build_batch_host(_ptr(cells), 4, K_TARGET, _ptr(pal), _ptr(counts), _ptr(boxes), _ptr(splits), _ptr(k))
    assert rc == 0
    for b, ref in enumerate(built):
        if ref == E_ARG:                                                    # the empty table: its code, zero rows, its neighbours exact
            assert k[b] == E_ARG and not pal[b].any() and not counts[b].any()
            assert not optional or (not boxes[b].any() and (splits[b] == -1).all())
        elif optional:
            assert BC.same((int(k[b]), pal[b], counts[b], boxes[b], splits[b]), ref, K_TARGET), b
        else:
            assert k[b] == ref["k"] and np.array_equal(pal[b, :ref["k"]], ref["palette"]) and not pal[b, ref["k"]:].any(), b
            assert np.array_equal(counts[b, :ref["k"]].astype(np.int64), ref["counts"]) and not counts[b, ref["k"]:].any(), b
    assert any(ref != E_ARG and ref["k"] < K_TARGET for ref in built)       # a table that cannot reach K_target is among them


@pytest.mark.parametrize("elem", [1, 2, 4])
@pytest.mark.parametrize("with_cls", [True, False])
def test_host_remap_batch_equals_the_per_image_reference(elem, with_cls):
    images, maps, off, _, built, remap, _ = batch()
    buf, cls = _concat(images, maps, 1)
    stride = K_TARGET + 3
    pal, k = _palettes(built, stride)
    for b, ref in enumerate(built):                                         # padding rows hold colours of the image: reading them would show
        if ref != E_ARG:
            pal[b, ref["k"]:] = np.resize(images[b], (stride - ref["k"], 3))
    nc = 2 if with_cls else 0
    idx = np.full(int(off[-1]), 0x7B, {1: np.uint8, 2: np.uint16, 4: np.uint32}[elem])
    sums = np.full((4, nc + 1, 2), 0x5555, np.uint64)
    rc = _lib().rhccq_palette_remap_batch_host(C.c_void_p(buf.ctypes.data + 1), _ptr(off), 4, _ptr(pal), stride, _ptr(k), _ptr(cls) if with_cls else None,
                                               nc, _ptr(idx), elem, _ptr(sums))
    assert rc == 0
    for b, ref in enumerate(built):
        got = idx[off[b]:off[b + 1]]
        if ref == E_ARG:
            assert not got.any() and not sums[b].any()
            continue
        want_idx, want_sums = remap[b] if with_cls else RM.remap_reference(images[b], ref["palette"])
        assert np.array_equal(got.astype(np.int64), want_idx) and np.array_equal(sums[b].astype(np.int64), want_sums), b


def test_host_remap_batch_skips_images_without_rows():
    images, maps, off, _, built, _, _ = batch()
    buf, _ = _concat(images, maps)
    pal, _ = _palettes(built, K_TARGET)
    k = np.array([0, -3, 5, 1], np.int32)
    idx = np.full(int(off[-1]), 0x7B, np.uint8)
    sums = np.full((4, 1, 2), 0x5555, np.uint64)
    assert _lib().rhccq_palette_remap_batch_host(_ptr(buf), _ptr(off), 4, _ptr(pal), K_TARGET, _ptr(k), None, 0, _ptr(idx), 1, _ptr(sums)) == 0
    assert not idx[:off[2]].any() and not sums[:3].any()                      # k_rows 0, a negative code, and the empty image
    assert not idx[off[3]:].any() and sums[3, 0, 0] == len(images[3])         # one row: index 0, but counted
    assert sums[3, 0, 1] == RM.remap_reference(images[3], pal[3, :1])[1][-1, 1]


def test_host_refine_batch_equals_the_per_image_reference():
    images, maps, off, _, built, _, refine = batch()
    buf, cls = _concat(images, maps, 1)
    stride = K_TARGET + 2
    pal, k = _palettes(built, stride)
    before = pal.copy()
    hist = np.full((4, MAX_ITER, 2), 0x5555, np.uint64)
    nit = np.full(4, 0x77, np.int32)
    w = np.array(WEIGHTS, np.int32)
    rc = _lib().rhccq_palette_refine_batch_host(C.c_void_p(buf.ctypes.data + 1), _ptr(off), 4, _ptr(pal), stride, _ptr(k), _ptr(cls), 2, _ptr(w), MAX_ITER,
                                                _ptr(hist), _ptr(nit))
    assert rc == 0
    for b, ref in enumerate(built):
        if ref == E_ARG:
            assert nit[b] == 0 and not hist[b].any() and np.array_equal(pal[b], before[b])
            continue
        want_pal, want_hist, want_n = refine[b]
        assert nit[b] == want_n and np.array_equal(hist[b].astype(np.int64), want_hist), b
        assert np.array_equal(pal[b, :ref["k"]], want_pal) and np.array_equal(pal[b, ref["k"]:], before[b, ref["k"]:]), b
        assert (np.diff(hist[b, :want_n, 0].astype(np.int64)) <= 0).all()


# ---- arguments ----------------------------------------------------------------------------------------------------------------------------
def test_bytes_helpers():
    lib = _lib()
    one = lib.rhccq_palette_build_bytes()
    assert [lib.rhccq_palette_build_batch_bytes(b) for b in (-1, 0, 1, 7, 300)] == [0, 0, one, 7 * one, 300 * one]
    assert lib.rhccq_palette_refine_batch_bytes(5, 300) == 5 * lib.rhccq_palette_refine_bytes(300) == 5 * 300 * 32
    assert lib.rhccq_palette_refine_batch_bytes(0, 300) == 0 and lib.rhccq_palette_refine_batch_bytes(5, 0) == 0


def _valid():
    """a valid two-image call of every host form: 3 + 1 pixels, K_stride = 3, no class map"""
    a = {"rgb": np.zeros((4, 3), np.uint8), "off": np.array([0, 3, 4], np.int64), "cls": np.zeros(4, np.uint8), "cells": np.zeros(2 * CELLS + 1, np.uint64),
         "pal": np.zeros((2, 3, 3), np.uint8), "counts": np.zeros(7, np.uint64), "splits": np.zeros((2, 2, 3), np.int32), "k": np.array([3, 2, 0], np.int32),
         "idx": np.zeros(5, np.uint16), "sums": np.zeros(2 * 17 * 2 + 1, np.uint64), "hist": np.zeros(2 * 64 * 2 + 1, np.uint64), "nit": np.zeros(3, np.int32)}
    a["rgb"][:] = [[0, 0, 0], [100, 7, 7], [250, 250, 1], [9, 9, 9]]
    return a


def _arg(a, over, name):
    v = over.get(name, "ok")
    if v is None:
        return C.c_void_p(0)
    if isinstance(v, np.ndarray):
        return _ptr(v)
    if v == "odd":
        return C.c_void_p(a[name].ctypes.data + (2 if a[name].dtype.itemsize == 4 else 1))
    return _ptr(a[name])


LAYOUT_ERRORS = [
    ("B = 0", {"B": 0}, E_ARG),
    ("B < 0", {"B": -2}, E_ARG),
    ("null px_off", {"off": None}, E_ARG),
    ("px_off[0] != 0", {"off": np.array([1, 3, 4], np.int64)}, E_ARG),
    ("px_off decreases", {"off": np.array([0, 3, 2], np.int64)}, E_ARG),
    ("B = 65536", {"B": 65536, "off": np.zeros(65537, np.int64)}, E_LIMIT),
    ("null rgb", {"rgb": None}, E_ARG),
    ("n_classes < 0", {"cls": "ok", "n_classes": -1}, E_ARG),
    ("n_classes = 17", {"cls": "ok", "n_classes": 17, "weights": [1] * 18}, E_ARG),
    ("n_classes without a class map", {"n_classes": 1, "weights": [1, 1]}, E_ARG),
]
CELLS_ERRORS = LAYOUT_ERRORS + [
    ("null cells", {"cells": None}, E_ARG),
    ("misaligned cells", {"cells": "odd"}, E_ARG),
    ("a weight of 256", {"weights": [256]}, E_ARG),
    ("all weights zero", {"cls": "ok", "n_classes": 1, "weights": [0, 0]}, E_ARG),
    ("one image of 2^32 pixels", {"off": np.array([0, 3, 3 + (1 << 32)], np.int64)}, E_LIMIT),
    ("one image above 2^32 / 255 at weight 255", {"off": np.array([0, (1 << 24) + 65794, (1 << 24) + 65795], np.int64), "weights": [255]}, E_LIMIT),
]
REMAP_ERRORS = LAYOUT_ERRORS + [
    ("null palettes", {"pal": None}, E_ARG),
    ("null k_rows", {"k": None}, E_ARG),
    ("misaligned k_rows", {"k": "odd"}, E_ARG),
    ("null idx_out", {"idx": None}, E_ARG),
    ("misaligned idx_out", {"idx": "odd"}, E_ARG),
    ("null sums", {"sums": None}, E_ARG),
    ("misaligned sums", {"sums": "odd"}, E_ARG),
    ("K_stride = 0", {"K_stride": 0}, E_ARG),
    ("K_stride < 0", {"K_stride": -4}, E_ARG),
    ("idx_elem_bytes = 3", {"elem": 3}, E_ARG),
    ("K_stride = 257 with 1-byte indices", {"K_stride": 257, "elem": 1}, E_ARG),
    ("K_stride = 65537", {"K_stride": 65537}, E_LIMIT),
]
REFINE_ERRORS = LAYOUT_ERRORS + [
    ("null palettes", {"pal": None}, E_ARG),
    ("null k_rows", {"k": None}, E_ARG),
    ("misaligned k_rows", {"k": "odd"}, E_ARG),
    ("null history", {"hist": None}, E_ARG),
    ("misaligned history", {"hist": "odd"}, E_ARG),
    ("null n_iter", {"nit": None}, E_ARG),
    ("misaligned n_iter", {"nit": "odd"}, E_ARG),
    ("K_stride = 0", {"K_stride": 0}, E_ARG),
    ("max_iter = 0", {"max_iter": 0}, E_ARG),
    ("max_iter = 65", {"max_iter": 65}, E_ARG),
    ("weight < 0", {"weights": [-1]}, E_ARG),
    ("all weights zero", {"cls": "ok", "n_classes": 2, "weights": [0, 0, 0]}, E_ARG),
    ("K_stride = 65537", {"K_stride": 65537}, E_LIMIT),
]
BUILD_ERRORS = [
    ("B = 0", {"B": 0}, E_ARG),
    ("B < 0", {"B": -1}, E_ARG),
    ("B = 65536", {"B": 65536}, E_LIMIT),
    ("null cells", {"cells": None}, E_ARG),
    ("misaligned cells", {"cells": "odd"}, E_ARG),
    ("null palette_out", {"pal": None}, E_ARG),
    ("null counts_out", {"counts": None}, E_ARG),
    ("misaligned counts_out", {"counts": "odd"}, E_ARG),
    ("misaligned splits", {"splits": "odd"}, E_ARG),
    ("null k_out", {"k": None}, E_ARG),
    ("misaligned k_out", {"k": "odd"}, E_ARG),
    ("K_target = 0", {"K_target": 0}, E_ARG),
    ("K_target = 32769", {"K_target": 32769}, E_LIMIT),
]


def _weights(over):
    w = over.get("weights")
    return None if w is None else np.array(w, np.int32)


def _cls(a, over):
    return _ptr(a["cls"]) if over.get("cls") == "ok" else C.c_void_p(0)


def _call_cells(a, over):
    w = _weights(over)                                                      # (kept alive over the call)
    return _lib().rhccq_palette_cells_batch_host(_arg(a, over, "rgb"), _arg(a, over, "off"), over.get("B", 2), _cls(a, over), over.get("n_classes", 0),
                                                 _ptr(w), _arg(a, over, "cells"))


def _call_build(a, over):
    return _lib().rhccq_palette_build_batch_host(_arg(a, over, "cells"), over.get("B", 2), over.get("K_target", 3), _arg(a, over, "pal"),
                                                 _arg(a, over, "counts"), C.c_void_p(0), _arg(a, over, "splits"), _arg(a, over, "k"))


def _call_remap(a, over):
    return _lib().rhccq_palette_remap_batch_host(_arg(a, over, "rgb"), _arg(a, over, "off"), over.get("B", 2), _arg(a, over, "pal"), over.get("K_stride", 3),
                                                 _arg(a, over, "k"), _cls(a, over), over.get("n_classes", 0), _arg(a, over, "idx"), over.get("elem", 2),
                                                 _arg(a, over, "sums"))


def _call_refine(a, over):
    w = _weights(over)
    return _lib().rhccq_palette_refine_batch_host(_arg(a, over, "rgb"), _arg(a, over, "off"), over.get("B", 2), _arg(a, over, "pal"),
                                                  over.get("K_stride", 3), _arg(a, over, "k"), _cls(a, over), over.get("n_classes", 0), _ptr(w),
                                                  over.get("max_iter", 2), _arg(a, over, "hist"), _arg(a, over, "nit"))


@pytest.mark.parametrize("what,over,code", CELLS_ERRORS, ids=[e[0] for e in CELLS_ERRORS])
def test_host_cells_batch_argument_errors(what, over, code):
    assert _call_cells(_valid(), over) == code, what


@pytest.mark.parametrize("what,over,code", BUILD_ERRORS, ids=[e[0] for e in BUILD_ERRORS])
def test_host_build_batch_argument_errors(what, over, code):
    assert _call_build(_valid(), over) == code, what


@pytest.mark.parametrize("what,over,code", REMAP_ERRORS, ids=[e[0] for e in REMAP_ERRORS])
def test_host_remap_batch_argument_errors(what, over, code):
    assert _call_remap(_valid(), over) == code, what


@pytest.mark.parametrize("what,over,code", REFINE_ERRORS, ids=[e[0] for e in REFINE_ERRORS])
def test_host_refine_batch_argument_errors(what, over, code):
    assert _call_refine(_valid(), over) == code, what


def test_host_forms_accept_the_valid_calls_the_errors_vary():
    a = _valid()
    a["cells"][:2 * CELLS] = np.concatenate([BC.cells_reference(a["rgb"][:3]).reshape(-1), BC.cells_reference(a["rgb"][3:]).reshape(-1)])
    want = a["cells"].copy()
    assert _call_build(a, {}) == 0 and a["k"][:2].tolist() == [3, 1] and a["counts"][:6].tolist() == [1, 1, 1, 1, 0, 0]
    assert _call_cells(a, {}) == 0 and np.array_equal(a["cells"], want)
    assert _call_remap(a, {}) == 0 and sorted(a["idx"][:3].tolist()) == [0, 1, 2] and a["idx"][3] == 0
    assert a["sums"][:4].tolist() == [3, 0, 1, 0]
    assert _call_refine(a, {}) == 0 and a["nit"][:2].tolist() == [1, 1]


def test_device_forms_need_a_context():
    """the device forms return RHCCQ_E_ARG for a null context before anything else"""
    lib, z = _lib(), C.c_void_p(0)
    assert lib.rhccq_palette_cells_batch(z, z, z, z, 1, z, 0, z, z) == E_ARG
    assert lib.rhccq_palette_build_batch(z, z, 1, 4, z, 0, z, z, z, z, z) == E_ARG
    assert lib.rhccq_palette_remap_batch(z, z, z, z, 1, z, 3, z, z, 0, z, 2, z) == E_ARG
    assert lib.rhccq_palette_refine_batch(z, z, z, z, 1, z, 3, z, z, 0, z, 2, z, 0, z, z) == E_ARG


def test_batch_entry_points_raise_without_a_gpu():
    """no CPU fallback: the Python surface needs the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError
    from roibasedimagecompression_amd.image import ImageEncoder
    from roibasedimagecompression_amd.ops import default_context
    imgs = [np.zeros((4, 4, 3), np.uint8), np.full((1, 3, 3), 200, np.uint8)]
    if torch.cuda.is_available():
        res = ImageEncoder().quantize_batch(imgs, colours=4)
        assert [r["stats"]["build"] for r in res] == [{"asked": 4, "rows": 1, "cells": 1, "steps": 0}] * 2
    else:
        with pytest.raises(RhccqError):
            default_context().palette_cells_batch(np.zeros((4, 3), np.uint8), [0, 4])
        with pytest.raises(RhccqError):
            ImageEncoder().quantize_batch(imgs, colours=4)
