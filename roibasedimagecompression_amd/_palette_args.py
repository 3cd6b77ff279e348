"""The argument layer of the Rhccq.palette_* wrappers (ops.py): every conversion and shape test they share, once.  Plain functions over
the target `device` and the calling operation's name `fn` (the prefix of every message); none needs a context or a GPU.  The limit
tests (K, n_classes, max_iter, weights' values) are NOT here: each wrapper keeps its own where it stands, some before allocating and
some only on the empty-image path, because that decides which message a caller sees."""
import ctypes as C

import numpy as np
import torch

from ._lib import RhccqError


def as_uint8(a, device, fn, what):
    """numpy or tensor, uint8 or bool -> a contiguous uint8 tensor on the device"""
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if a.dtype == torch.bool:
        a = a.view(torch.uint8)
    if a.dtype != torch.uint8:
        raise TypeError(f"{fn}: {what} must be uint8, got {a.dtype}")
    return a.to(device).contiguous()


def _integers(a, fn, what):
    """a numpy array of any integers as an int64 tensor (uint64 keeps its bits); a tensor as it is"""
    if torch.is_tensor(a):
        return a
    a = np.ascontiguousarray(a)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{fn}: {what} must be integers, got {a.dtype}")
    return torch.from_numpy(a.astype(np.uint64).view(np.int64))


def as_dtype(a, dtype, device, fn, what):
    """numpy or tensor -> a contiguous tensor of exactly `dtype` on the device; int64 takes any numpy integers and uint8 / int16 / int32
    tensors (counts, as palette_reduce takes them)"""
    if not torch.is_tensor(a):
        a = _integers(a, fn, what) if dtype is torch.int64 else torch.from_numpy(np.ascontiguousarray(a))
    if a.dtype != dtype and not (dtype is torch.int64 and a.dtype in (torch.int32, torch.uint8, torch.int16)):
        raise TypeError(f"{fn}: {what} must be {dtype}, got {a.dtype}")
    return a.to(device).to(dtype).contiguous()


def cells_table(cells, fn):
    """palette_cells' table(s): numpy integers or an int64 tensor -> an int64 tensor where it lies (the caller tests the shape, then moves it)"""
    cells = _integers(cells, fn, "cells")
    if cells.dtype != torch.int64:
        raise TypeError(f"{fn}: cells must be int64, got {cells.dtype}")
    return cells


def pixels(rgb, palette, device, fn, rows=False):
    """rgb uint8[..., 3] (rows: [H, W, 3]) and palette uint8[K, 3] or None -> both on the device"""
    rgb = as_uint8(rgb, device, fn, "rgb")
    form = "[H, W, 3]" if rows else "[..., 3]"
    bad = (rgb.ndim != 3 if rows else rgb.ndim < 1) or rgb.shape[-1] != 3
    if palette is None:
        if bad:
            raise ValueError(f"{fn}: rgb {form} is expected")
        return rgb, None
    palette = as_uint8(palette, device, fn, "palette")
    if bad or palette.ndim != 2 or palette.shape[1] != 3:
        raise ValueError(f"{fn}: rgb {form} and palette [K, 3] are expected")
    return rgb, palette


def class_map(cls, n, n_classes, device, fn, what="class_map", without="n_classes"):
    """the class map (uint8 / bool, one element per pixel) on the device, or None; without one n_classes is 0"""
    if cls is None:
        if n_classes:
            raise ValueError(f"{fn}: {without} without a class map")
        return None
    cls = as_uint8(cls, device, fn, what)
    if cls.numel() != n:
        raise ValueError(f"{fn}: the class map must have one element per pixel")
    return cls


def class_table(value, n_classes, most, fn, noun):
    """a slack / penalty: one integer 0..most, or n_classes + 1 of them -> (the list of n_classes + 1, the const uint32_t* argument)"""
    table = [int(value)] * (max(n_classes, 0) + 1) if np.ndim(value) == 0 else [int(v) for v in value]
    if len(table) != n_classes + 1:
        raise ValueError(f"{fn}: {noun} is one integer or n_classes + 1 of them")
    if min(table) < 0 or max(table) > most:
        raise ValueError(f"{fn}: a {noun} must be 0..{most}")
    return table, C.cast((C.c_uint32 * len(table))(*table), C.c_void_p)


def class_weights(weights, n_classes, fn):
    """weights: n_classes + 1 integers (n_classes None: their number tells it) or None -> (the list or None, the const int32_t* argument,
    null for None).  The pointer keeps its array alive."""
    if weights is None:
        return None, C.c_void_p(0)
    w = [int(v) for v in weights]
    if len(w) < 1 if n_classes is None else len(w) != n_classes + 1:
        raise ValueError(f"{fn}: weights must have n_classes + 1 entries")
    return w, C.cast((C.c_int32 * len(w))(*w), C.c_void_p)


def bad_weights(w):
    """what every wrapper's limit test asks of the list: 0..255, one > 0"""
    return w is not None and (min(w) < 0 or max(w) > 255 or not any(w))


def counted_rows(palette, counts, fn):
    """palette [K, 3] with counts [K] (converted) -> K"""
    if palette.ndim != 2 or palette.shape[1] != 3 or counts.ndim != 1 or counts.shape[0] != palette.shape[0]:
        raise ValueError(f"{fn}: palette [K, 3] and counts [K] are expected")
    return int(palette.shape[0])


def rows_cap(K, cap, fn):
    """the reduction's row cap (ops.palette_reduce_max_rows()), which the ladder's device forms share"""
    if K > cap:
        raise RhccqError(f"{fn}: {K} rows, the device form takes at most {cap} (palette_reduce_max_rows())")


def index_dtype(K):
    """the index buffer of a K-row palette: uint8, or int16 holding uint16"""
    return torch.uint8 if K <= 256 else torch.int16


def index_map(indices, H, W, device, fn):
    """an index map of H x W elements in the dtypes container._index_tensor accepts -> a flat contiguous device tensor: uint8, int16
    holding uint16, or int32 (from int32 / int64; numpy uint16 becomes the int16 storage, any other numpy integers int32)"""
    if not torch.is_tensor(indices):
        a = np.ascontiguousarray(indices)
        if a.dtype.kind not in "iu":
            raise TypeError(f"{fn}: indices must be integers, got {a.dtype}")
        a = a if a.dtype == np.uint8 else a.view(np.int16) if a.dtype == np.uint16 else a.astype(np.int32)
        indices = torch.from_numpy(a)
    if indices.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64):
        raise TypeError(f"{fn}: indices must be uint8, int16 (uint16 storage), int32 or int64, got {indices.dtype}")
    if indices.numel() != H * W:
        raise ValueError(f"{fn}: indices must have H * W elements")
    t = indices.to(device).reshape(-1)
    return (t.to(torch.int32) if t.dtype == torch.int64 else t).contiguous()


def k_out_rows(k, fn, empty="every count is zero", over="the counts add up to more than 2^32 - 1"):
    """the k_out a chain wrote: the rows it made, or the negative code of an error only the counts (the table) show"""
    if k < 0:
        raise RhccqError(f"{fn} failed ({k}): " + (empty if k == -1 else over))
    return k
