"""The .rhccq container written on the device: the same package and framing as api/compression.py's
lossless_compress_optimized + save_compressed (compression.py:119-142,151-220), with every zlib layer compressed by
the device encoder (csrc/zlib_deflate.hip) instead of zlib.compress(level=9) on one host core.

The files are format-compatible, not byte-identical: load_compressed / lossless_decompress read them unchanged, but
the zlib streams differ from zlib's own.  The host path (api.compression) is the one for byte-identical files.  There
is no CPU fallback: without a GPU these functions raise like Rhccq(0) does."""
import pickle
import struct

import numpy as np
import torch

from .ops import RhccqError, default_context
from .segment import IndexList, as_index_array


def _index_tensor(indices, rh):
    """indices -> (flat contiguous device tensor, element bytes): uint8, int16 holding uint16 (FrameEncoder's storage),
    int32, or a host array / list that is uploaded"""
    if isinstance(indices, torch.Tensor):
        if not indices.is_cuda:
            indices = indices.to(rh.device)
        t = indices.reshape(-1).contiguous()
        if t.dtype == torch.uint8:
            return t, 1
        if t.dtype == torch.int16:
            return t, 2
        if t.dtype in (torch.int32, torch.int64):
            return t.to(torch.int32), 4
        raise TypeError(f"indices tensor of dtype {t.dtype}: uint8, int16 (uint16 storage), int32 or int64 expected")
    if not isinstance(indices, (list, np.ndarray, IndexList)):
        raise TypeError(f"indices must be a device tensor, list or numpy array, got {type(indices)}")
    arr = as_index_array(indices)
    if arr.dtype == np.uint8:
        return rh.dev(arr), 1
    return rh.dev(arr.astype(np.int32, copy=False)), 4


def narrow_indices(indices, rh=None):
    """-> (contiguous uint8 device tensor holding the index map in its container dtype, dtype name).  The dtype follows
    compression.py's rule on the largest index (< 256 uint8, < 65 536 uint16, else uint32), found on the device; the
    bytes equal numpy's astype(dtype).tobytes() of the same indices."""
    rh = rh or default_context()
    t, eb = _index_tensor(indices, rh)
    if t.numel() == 0:
        return torch.empty((0,), dtype=torch.uint8, device=rh.device), "uint8"
    wide = t.to(torch.int32) & 0xFFFF if eb == 2 else t.to(torch.int32)
    mx = int(wide.max().item())
    if mx < 256:
        return (t if eb == 1 else wide.to(torch.uint8)), "uint8"
    if mx < 65536:
        if eb == 2:
            return t.view(torch.uint8), "uint16"
        return torch.stack([(wide & 0xFF).to(torch.uint8), (wide >> 8).to(torch.uint8)], dim=1).reshape(-1), "uint16"
    return t.view(torch.uint8), "uint32"


def lossless_compress_device(palette, indices, shape, rh=None):
    """lossless_compress_optimized with the device encoder: the same dict (s, l, p, i, d); "i" and "p" decompress to
    exactly the bytes the host function compresses"""
    rh = rh or default_context()
    pal = np.array(palette, dtype=np.uint8)
    idx, name = narrow_indices(indices, rh)
    return {"s": shape, "l": len(palette), "p": rh.zlib_compress(rh.dev(pal.reshape(-1))), "i": rh.zlib_compress(idx), "d": name}


def save_compressed_device(compressed_data, filename, rh=None):
    """save_compressed with the outer zlib layer on the device: b"RHCCQ", <I length, zlib of the protocol-5 pickle;
    returns what save_compressed returns (the body's length + 8)"""
    rh = rh or default_context()
    raw = np.frombuffer(pickle.dumps(compressed_data, protocol=5), dtype=np.uint8).copy()
    body = rh.zlib_compress(rh.dev(raw))
    with open(filename, "wb") as f:
        f.write(b"RHCCQ")
        f.write(struct.pack("<I", len(body)))
        f.write(body)
    return len(body) + 8


def write_frame(result, filename, rh=None):
    """the result dict of FrameEncoder.encode / encode_native straight to a .rhccq file; returns save_compressed's value"""
    if "palette" not in result or "indices" not in result or "shape" not in result:
        raise RhccqError("write_frame: a FrameEncoder result (palette, indices, shape) is required")
    pkg = lossless_compress_device(result["palette"], result["indices"], result["shape"], rh)
    return save_compressed_device(pkg, filename, rh)
