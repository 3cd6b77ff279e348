"""The argument layer of the Rhccq.palette_* wrappers (roibasedimagecompression_amd/_palette_args.py) on device="cpu": every accepted
input kind of every helper and every refusal with its exception class and its message, and ImageEncoder._run_arg with both of its
nouns.  The message literals are the texts the wrappers raised before the helpers were shared; they pin them.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from roibasedimagecompression_amd import RhccqError
from roibasedimagecompression_amd import _palette_args as A

DEV = "cpu"


def raises(cls, literal):
    return pytest.raises(cls, match="^" + re.escape(literal) + "$")


def _kinds(a):
    """an array as the wrappers take it: numpy, CPU tensor, non-contiguous numpy and tensor views with the same values"""
    wide = np.repeat(a, 2, axis=-1)
    return [a, torch.from_numpy(a.copy()), wide[..., ::2], torch.from_numpy(wide.copy())[..., ::2]]


# ---- the uint8 conversion -----------------------------------------------------------------------------------------------------------------
def test_as_uint8_takes_numpy_tensor_bool_and_strided_input():
    a = np.arange(24, dtype=np.uint8).reshape(2, 4, 3)
    for given in _kinds(a):
        got = A.as_uint8(given, DEV, "op", "rgb")
        assert got.dtype == torch.uint8 and got.is_contiguous() and got.device.type == "cpu" and np.array_equal(got.numpy(), a)
    m = a[..., 0] % 2 == 1
    for given in _kinds(m):
        got = A.as_uint8(given, DEV, "op", "class_map")
        assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.numpy(), m.astype(np.uint8))


def test_as_uint8_refuses_other_types():
    with raises(TypeError, "palette_remap: rgb must be uint8, got torch.int32"):
        A.as_uint8(np.zeros((2, 3), np.int32), DEV, "palette_remap", "rgb")
    with raises(TypeError, "palette_cells: cls must be uint8, got torch.float32"):
        A.as_uint8(torch.zeros(4), DEV, "palette_cells", "cls")


# ---- the integer-to-int64 / exact-dtype conversion ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32, np.int64, np.uint64])
def test_as_dtype_widens_integers_to_int64(dtype):
    a = np.array([0, 1, 77, 255], dtype)
    for given in _kinds(a) if dtype != np.uint64 else [a, np.repeat(a, 2)[::2]]:                     # (torch has no uint64 arithmetic)
        got = A.as_dtype(given, torch.int64, DEV, "op", "counts")
        assert got.dtype == torch.int64 and got.is_contiguous() and got.tolist() == [0, 1, 77, 255]


def test_as_dtype_keeps_the_bits_of_uint64():
    got = A.as_dtype(np.array([2 ** 64 - 1, 2 ** 63], np.uint64), torch.int64, DEV, "op", "counts")
    assert got.tolist() == [-1, -2 ** 63]


def test_as_dtype_exact_types():
    pal = np.arange(12, dtype=np.uint8).reshape(4, 3)
    for given in _kinds(pal):
        got = A.as_dtype(given, torch.uint8, DEV, "op", "palette")
        assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.numpy(), pal)
    merges = np.array([[0, 1], [0, 2]], np.int32)
    for given in _kinds(merges):
        assert np.array_equal(A.as_dtype(given, torch.int32, DEV, "op", "merges").numpy(), merges)


def test_as_dtype_refusals():
    with raises(TypeError, "palette_reduce: counts must be integers, got float64"):
        A.as_dtype(np.zeros(3), torch.int64, DEV, "palette_reduce", "counts")
    with raises(TypeError, "palette_curve: moments must be torch.int64, got torch.float32"):
        A.as_dtype(torch.zeros(3), torch.int64, DEV, "palette_curve", "moments")
    with raises(TypeError, "palette_rung: palette must be torch.uint8, got torch.bool"):
        A.as_dtype(np.zeros((2, 3), bool), torch.uint8, DEV, "palette_rung", "palette")
    with raises(TypeError, "palette_rung: merges must be torch.int32, got torch.int64"):
        A.as_dtype(np.zeros((1, 2), np.int64), torch.int32, DEV, "palette_rung", "merges")


def test_cells_table():
    a = np.arange(8, dtype=np.int32).reshape(4, 2)
    for given in (a, a.astype(np.uint8), a.astype(np.int16), a.astype(np.uint64), a.astype(np.int64), np.repeat(a, 2, axis=1)[:, ::2],
                  torch.from_numpy(a.astype(np.int64))):
        got = A.cells_table(given, "palette_build")
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), a)
    with raises(TypeError, "palette_build: cells must be integers, got float32"):
        A.cells_table(a.astype(np.float32), "palette_build")
    with raises(TypeError, "palette_build_batch: cells must be int64, got torch.int32"):                # a tensor is not widened
        A.cells_table(torch.from_numpy(a), "palette_build_batch")


# ---- pixels + palette ---------------------------------------------------------------------------------------------------------------------
def test_pixels_shapes():
    rgb, pal = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3), np.arange(9, dtype=np.uint8).reshape(3, 3)
    for given in _kinds(rgb):
        for rows in (False, True):
            r, p = A.pixels(given, torch.from_numpy(pal), DEV, "op", rows=rows)
            assert np.array_equal(r.numpy(), rgb) and np.array_equal(p.numpy(), pal) and r.is_contiguous()
    r, p = A.pixels(rgb.reshape(-1, 3), None, DEV, "op")
    assert p is None and tuple(r.shape) == (35, 3)
    assert tuple(A.pixels(np.zeros((0, 7, 3), np.uint8), pal, DEV, "op", rows=True)[0].shape) == (0, 7, 3)


def test_pixels_refusals():
    rgb, pal = np.zeros((5, 7, 3), np.uint8), np.zeros((3, 3), np.uint8)
    for bad_rgb, bad_pal in ((rgb[..., :2], pal), (np.uint8(3), pal), (rgb, pal[:, :2]), (rgb, pal.reshape(-1))):
        with raises(ValueError, "palette_remap: rgb [..., 3] and palette [K, 3] are expected"):
            A.pixels(bad_rgb, bad_pal, DEV, "palette_remap")
    for bad_rgb, bad_pal in ((rgb.reshape(-1, 3), pal), (rgb[None], pal), (rgb, pal[None])):
        with raises(ValueError, "palette_runs: rgb [H, W, 3] and palette [K, 3] are expected"):
            A.pixels(bad_rgb, bad_pal, DEV, "palette_runs", rows=True)
    with raises(ValueError, "palette_cells: rgb [..., 3] is expected"):
        A.pixels(rgb.reshape(-1), None, DEV, "palette_cells")
    with raises(TypeError, "palette_segment: rgb must be uint8, got torch.int32"):                      # rgb before the palette
        A.pixels(rgb.astype(np.int32), pal.astype(np.int16), DEV, "palette_segment", rows=True)
    with raises(TypeError, "palette_segment: palette must be uint8, got torch.int16"):                  # the types before the shapes
        A.pixels(rgb.reshape(-1, 3), pal.astype(np.int16), DEV, "palette_segment", rows=True)


# ---- class map ----------------------------------------------------------------------------------------------------------------------------
def test_class_map():
    m = (np.arange(35).reshape(5, 7) % 3 == 0)
    for given in _kinds(m) + _kinds(m.astype(np.uint8)):
        got = A.class_map(given, 35, 2, DEV, "op")
        assert got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(got.numpy(), m.astype(np.uint8))
    assert A.class_map(None, 35, 0, DEV, "op") is None
    again = A.class_map(got, 35, 2, DEV, "op")                                                           # a converted map passes as it is
    assert again.data_ptr() == got.data_ptr()


def test_class_map_refusals():
    m = np.zeros((5, 7), np.uint8)
    with raises(ValueError, "palette_remap: the class map must have one element per pixel"):
        A.class_map(m[:-1], 35, 2, DEV, "palette_remap")
    with raises(ValueError, "palette_moments: n_classes without a class map"):
        A.class_map(None, 35, 2, DEV, "palette_moments")
    with raises(ValueError, "palette_refine: class weights without a class map"):
        A.class_map(None, 35, 2, DEV, "palette_refine", without="class weights")
    with raises(TypeError, "palette_runs: class_map must be uint8, got torch.int64"):
        A.class_map(m.astype(np.int64), 35, 2, DEV, "palette_runs")
    with raises(TypeError, "palette_cells: cls must be uint8, got torch.int64"):
        A.class_map(m.astype(np.int64), 35, 2, DEV, "palette_cells", what="cls")


# ---- per-class table ----------------------------------------------------------------------------------------------------------------------
def _u32(arg, n):
    return list(C.cast(arg, C.POINTER(C.c_uint32))[:n])


def test_class_table():
    table, arg = A.class_table(7, 2, 195075, "palette_runs", "slack")
    assert table == [7, 7, 7] and _u32(arg, 3) == table
    table, arg = A.class_table(np.int64(195075), 0, 195075, "palette_runs", "slack")
    assert table == [195075] and _u32(arg, 1) == table
    for given in ([0, 16777215, 5], (0, 16777215, 5), np.array([0, 16777215, 5])):
        table, arg = A.class_table(given, 2, 16777215, "palette_segment", "penalty")
        assert table == [0, 16777215, 5] and _u32(arg, 3) == table and isinstance(arg, C.c_void_p)


def test_class_table_refusals():
    for given, nc in (([1, 2], 2), ([1, 2, 3], 0), (1, -1)):
        with raises(ValueError, "palette_runs: slack is one integer or n_classes + 1 of them"):
            A.class_table(given, nc, 195075, "palette_runs", "slack")
    for given in (-1, 195076, [0, 195076, 0], [0, 0, -1]):
        with raises(ValueError, "palette_runs: a slack must be 0..195075"):
            A.class_table(given, 0 if np.ndim(given) == 0 else 2, 195075, "palette_runs", "slack")
    with raises(ValueError, "palette_segment: penalty is one integer or n_classes + 1 of them"):
        A.class_table([1, 2], 2, 16777215, "palette_segment", "penalty")
    with raises(ValueError, "palette_segment: a penalty must be 0..16777215"):
        A.class_table(16777216, 0, 16777215, "palette_segment", "penalty")
    with raises(ValueError, "palette_runs: slack is one integer or n_classes + 1 of them"):             # the length before the values
        A.class_table([1, -2], 2, 195075, "palette_runs", "slack")


# ---- weights ------------------------------------------------------------------------------------------------------------------------------
def test_class_weights():
    w, arg = A.class_weights(None, 0, "palette_cells")
    assert w is None and isinstance(arg, C.c_void_p) and not arg.value
    assert A.class_weights(None, None, "palette_refine")[0] is None
    for given in ([1, 0, 255], (1, 0, 255), np.array([1, 0, 255], np.uint8)):
        for nc in (2, None):
            w, arg = A.class_weights(given, nc, "op")
            assert w == [1, 0, 255] and list(C.cast(arg, C.POINTER(C.c_int32))[:3]) == w
    w, arg = A.class_weights([-1, 256], 1, "op")                                                         # the values are the wrappers' to test
    assert w == [-1, 256] and list(C.cast(arg, C.POINTER(C.c_int32))[:2]) == w
    assert A.bad_weights([-1, 2]) and A.bad_weights([256]) and A.bad_weights([0, 0]) and not A.bad_weights(None) and not A.bad_weights([0, 255])


def test_class_weights_refusals():
    with raises(ValueError, "palette_cells: weights must have n_classes + 1 entries"):
        A.class_weights([1, 2], 2, "palette_cells")
    with raises(ValueError, "palette_cells_batch: weights must have n_classes + 1 entries"):
        A.class_weights([], 0, "palette_cells_batch")
    with raises(ValueError, "palette_refine: weights must have n_classes + 1 entries"):
        A.class_weights([], None, "palette_refine")


# ---- palette + counts + cap, index dtype, k_out ---------------------------------------------------------------------------------------------
def test_counted_rows_and_cap():
    pal, counts = torch.zeros((5, 3), dtype=torch.uint8), torch.ones(5, dtype=torch.int64)
    assert A.counted_rows(pal, counts, "op") == 5 and A.counted_rows(pal[:0], counts[:0], "op") == 0
    for bad_pal, bad_counts in ((pal[:, :2], counts), (pal.reshape(-1), counts), (pal, counts[:4]), (pal, counts.reshape(5, 1))):
        with raises(ValueError, "palette_reduce: palette [K, 3] and counts [K] are expected"):
            A.counted_rows(bad_pal, bad_counts, "palette_reduce")
    assert A.rows_cap(4096, 4096, "op") is None
    with raises(RhccqError, "palette_curve: 4097 rows, the device form takes at most 4096 (palette_reduce_max_rows())"):
        A.rows_cap(4097, 4096, "palette_curve")


def test_index_dtype_switches_at_257_rows():
    assert [A.index_dtype(K) for K in (1, 256, 257, 65536)] == [torch.uint8, torch.uint8, torch.int16, torch.int16]


def test_k_out_rows():
    assert A.k_out_rows(0, "op") == 0 and A.k_out_rows(17, "op") == 17
    with raises(RhccqError, "palette_reduce failed (-1): every count is zero"):
        A.k_out_rows(-1, "palette_reduce")
    with raises(RhccqError, "palette_rung failed (-3): the counts add up to more than 2^32 - 1"):
        A.k_out_rows(-3, "palette_rung")
    with raises(RhccqError, "palette_build failed (-1): the table is empty"):
        A.k_out_rows(-1, "palette_build", "the table is empty", "the table's N adds up to more than 2^32 - 1")
    with raises(RhccqError, "palette_build failed (-3): the table's N adds up to more than 2^32 - 1"):
        A.k_out_rows(-3, "palette_build", "the table is empty", "the table's N adds up to more than 2^32 - 1")


# ---- ImageEncoder's run_slack / run_penalty keyword -----------------------------------------------------------------------------------------
RUN_ARGS = [("run_slack", "slack", 195075), ("run_penalty", "penalty", 16777215)]


@pytest.mark.parametrize("name,key,most", RUN_ARGS, ids=[a[0] for a in RUN_ARGS])
def test_run_arg(name, key, most):
    from roibasedimagecompression_amd import ops
    from roibasedimagecompression_amd.image import ImageEncoder
    assert most == {"slack": ops.RUN_SLACK_MAX, "penalty": ops.RUN_PENALTY_MAX}[key]
    run = ImageEncoder._run_arg
    assert run("encode", name, key, most, None, True) is None
    assert run("encode", name, key, most, most, False) == {key: most, "nonroi": most, "roi": most}
    assert run("encode", name, key, most, np.int64(0), True) == {key: 0, "nonroi": 0, "roi": 0}
    assert run("encode", name, key, most, {"roi": 3, "nonroi": 9}, True) == {key: {"roi": 3, "nonroi": 9}, "nonroi": 9, "roi": 3}
    with raises(ValueError, f'encode: {name} is a number or a dict over "roi" and "nonroi"'):
        run("encode", name, key, most, {"roi": 3}, True)
    with raises(ValueError, f"encode: a roi / nonroi {name} needs roi_mask"):
        run("encode", name, key, most, {"roi": 3, "nonroi": 9}, False)
    for bad in (-1, most + 1, {"roi": 3, "nonroi": most + 1}, {"roi": -1, "nonroi": 0}):
        with raises(ValueError, f"encode: a {name} must be 0..{most}"):
            run("encode", name, key, most, bad, True)
    # _runs_args hands each keyword to it with its own noun and bound
    assert ImageEncoder._runs_args("quantize", 5, None, False) == {"slack": 5, "nonroi": 5, "roi": 5}
    assert ImageEncoder._runs_args("quantize", None, 5, False) == {"penalty": 5, "nonroi": 5, "roi": 5}
    assert ImageEncoder._runs_args("quantize", None, None, False) is None
    with raises(ValueError, "quantize: a run_slack must be 0..195075"):
        ImageEncoder._runs_args("quantize", 195076, None, False)
    with raises(ValueError, "quantize: a run_penalty must be 0..16777215"):
        ImageEncoder._runs_args("quantize", None, 16777216, False)
