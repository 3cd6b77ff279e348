"""The .rhccq container written on the device: the same package and framing as api/compression.py's
lossless_compress_optimized + save_compressed (compression.py:119-142,151-220), with every zlib layer compressed by
the device encoder (csrc/zlib_deflate.hip) instead of zlib.compress(level=9) on one host core.

The files are format-compatible, not byte-identical: load_compressed / lossless_decompress read them unchanged, but
the zlib streams differ from zlib's own.  With exact=True every layer goes through the level-9 encoder of
csrc/zlib_deflate9.hip instead, and the file is byte-identical to the host path's (api.compression).  The read
side (load_compressed_device, lossless_decompress_device, read_frame) inflates every layer with the device decoder
(csrc/zlib_inflate.hip) and leaves the index map on the device.  There is no CPU fallback: without a GPU these functions
raise like Rhccq(0) does."""
import io
import os
import pickle
import struct
import time

import numpy as np
import torch

from .api.uncompression import _SafeUnpickler
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


def lossless_compress_device(palette, indices, shape, rh=None, exact=False):
    """lossless_compress_optimized with the device encoder: the same dict (s, l, p, i, d); "i" and "p" decompress to
    exactly the bytes the host function compresses.  exact=True: "p" and "i" are also byte-identical to the host's
    (the level-9 encoder of csrc/zlib_deflate9.hip); the shape is kept as given, as the host function keeps it"""
    rh = rh or default_context()
    pal = np.array(palette, dtype=np.uint8)
    idx, name = narrow_indices(indices, rh)
    return {"s": shape, "l": len(palette), "p": rh.zlib_compress(rh.dev(pal.reshape(-1)), exact=exact),
            "i": rh.zlib_compress(idx, exact=exact), "d": name}


def package_bytes(compressed_data, rh=None, exact=False):
    """the .rhccq file of a package (lossless_compress_device's dict) as bytes: b"RHCCQ", <I length, zlib of the protocol-5 pickle,
    the outer zlib layer on the device.  exact=True: the bytes of save_compressed's file"""
    rh = rh or default_context()
    raw = np.frombuffer(pickle.dumps(compressed_data, protocol=5), dtype=np.uint8).copy()
    body = rh.zlib_compress(rh.dev(raw), exact=exact)
    return b"RHCCQ" + struct.pack("<I", len(body)) + body


def save_compressed_device(compressed_data, filename, rh=None, exact=False):
    """save_compressed with the outer zlib layer on the device (package_bytes written to `filename`); returns what save_compressed
    returns (the body's length + 8).  exact=True: the file is byte-identical to save_compressed's"""
    data = package_bytes(compressed_data, rh, exact=exact)
    with open(filename, "wb") as f:
        f.write(data)
    return len(data) - 1                                   # (save_compressed counts the body and 8 of the 9 framing bytes)


def frame_bytes(result, rh=None, exact=False):
    """the .rhccq file of a FrameEncoder result (palette, indices, shape) as bytes, built in memory: what write_frame writes.
    exact=True: every layer through the level-9 encoder, so the bytes are those of the host path's file"""
    if "palette" not in result or "indices" not in result or "shape" not in result:
        raise RhccqError("write_frame: a FrameEncoder result (palette, indices, shape) is required")
    pkg = lossless_compress_device(result["palette"], result["indices"], result["shape"], rh, exact=exact)
    return package_bytes(pkg, rh, exact=exact)


def write_frame(result, filename, rh=None, exact=False):
    """the result dict of FrameEncoder.encode / encode_native straight to a .rhccq file; returns save_compressed's value.
    exact=True: every layer through the level-9 encoder, so the file is byte-identical to
    save_compressed(lossless_compress_optimized(palette, indices, shape), filename)"""
    if "palette" not in result or "indices" not in result or "shape" not in result:
        raise RhccqError("write_frame: a FrameEncoder result (palette, indices, shape) is required")
    pkg = lossless_compress_device(result["palette"], result["indices"], result["shape"], rh, exact=exact)
    return save_compressed_device(pkg, filename, rh, exact=exact)


def _png_frame(result, rh, fn):
    """a result (palette, indices, shape) -> (rh, flat device indices, H, W, uint8 palette array)"""
    if not isinstance(result, dict) or "palette" not in result or "indices" not in result or "shape" not in result:
        raise RhccqError(f"{fn}: a FrameEncoder result (palette, indices, shape) is required")
    rh = rh or default_context()
    pal = result["palette"]
    if not isinstance(pal, torch.Tensor):
        pal = np.array(pal, dtype=np.uint8).reshape(-1, 3)
    h, w = (int(v) for v in result["shape"][:2])
    return rh, _index_tensor(result["indices"], rh)[0], h, w, pal


def png_bytes(result, rh=None, exact=False, depth8=False, filter=True):
    """the PNG file of a result (palette, indices, shape: what write_frame takes) as bytes, built on the device: palette PNG
    (colour type 3, 1 / 2 / 4 / 8 bits) up to 256 rows, truecolour with adaptive row filters above (include/rhccq.h).  An index past
    the palette shows row 0, as read_frame's image does.  exact=True: IDAT through the level-9 encoder, the file a function of the
    result alone"""
    return png_file(result, rh, exact=exact, depth8=depth8, filter=filter)[0]


def png_file(result, rh=None, exact=False, depth8=False, filter=True):
    """png_bytes with what the file is: -> (bytes, {"bytes": their number, "colour_type": 3 or 2, "depth": bits a sample,
    "filter_rows": [rows of filter type 0, 1, 2, 3, 4]}); the file and the five counts come down in one copy each, together"""
    rh, idx, h, w, pal = _png_frame(result, rh, "write_png")
    out, length, rows = rh._png_encode(idx, h, w, pal, exact, depth8, filter)
    n = int(length.item())
    data, rows = rh.to_host(out[:n], rows)
    K = len(pal)
    depth = 8 if (K > 16 or depth8) else 1 if K <= 2 else 2 if K <= 4 else 4
    return data.tobytes(), {"bytes": n, "colour_type": 3 if K <= 256 else 2, "depth": depth, "filter_rows": [int(v) for v in rows]}


def write_png(result, filename, rh=None, exact=False, depth8=False, filter=True):
    """png_bytes written to `filename`; returns the file's length in bytes"""
    data = png_bytes(result, rh, exact=exact, depth8=depth8, filter=filter)
    with open(filename, "wb") as f:
        f.write(data)
    return len(data)


def _gif_frames(results, rh, delta):
    """one result or a list of them -> (rh, flat device indices of all frames, n, H, W, palettes as Rhccq.gif_encode_async takes them,
    rows per local table or None)"""
    if isinstance(results, dict):
        results = [results]
    if not isinstance(results, (list, tuple)) or not results:
        raise RhccqError("write_gif: a result (palette, indices, shape) or a list of them is required")
    for r in results:
        if not isinstance(r, dict) or "palette" not in r or "indices" not in r or "shape" not in r:
            raise RhccqError("write_gif: a FrameEncoder result (palette, indices, shape) is required")
    # what the definition refuses is decided on the host, before any device work
    h, w = (int(v) for v in results[0]["shape"][:2])
    if any(tuple(int(v) for v in r["shape"][:2]) != (h, w) for r in results):
        raise ValueError("write_gif: every frame must have the same shape")
    if h > 65535 or w > 65535:
        raise ValueError("write_gif: a GIF frame is at most 65535 x 65535")
    pals = [r["palette"].cpu().numpy() if isinstance(r["palette"], torch.Tensor) else r["palette"] for r in results]
    pals = [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1, 3) for p in pals]
    if max(len(p) for p in pals) > 256:
        raise ValueError("write_gif: a GIF colour table has at most 256 rows")
    same = all(np.array_equal(p, pals[0]) for p in pals[1:])
    if delta and not same:
        raise ValueError("write_gif: delta needs one palette for all frames (a global colour table)")
    if delta and len(pals[0]) > 255:
        raise ValueError("write_gif: delta needs a palette of at most 255 rows (the transparent index is one more entry)")
    frames = [_png_frame(r, rh, "write_gif") for r in results]
    rh = frames[0][0]
    idx = [f[1] for f in frames]
    if len({t.dtype for t in idx}) > 1:
        idx = [t.to(torch.int32) & 0xFFFF if t.dtype == torch.int16 else t.to(torch.int32) for t in idx]
    idx = idx[0] if len(idx) == 1 else torch.cat(idx)
    if same:
        return rh, idx, len(frames), h, w, pals[0], None
    block = np.zeros((len(pals), max(len(p) for p in pals), 3), np.uint8)
    for f, p in enumerate(pals):
        block[f, :len(p)] = p
    return rh, idx, len(frames), h, w, block, [len(p) for p in pals]


def gif_file(results, rh=None, delay=4, loop=0, delta=False):
    """gif_bytes with what the file is: -> (bytes, {"bytes": their number, "frames", "table": "global" | "local", "colours": rows of the
    largest table, "delta", "stream_bytes": [bytes of every frame's code stream]}); the file and the stream lengths come down together"""
    rh, idx, n, h, w, pals, rows = _gif_frames(results, rh, delta)
    out, length, lens = rh.gif_encode_async(idx, n, h, w, pals, rows, delay, loop, delta)
    size = int(length.item())
    data, lens = rh.to_host(out[:size], lens)
    return data.tobytes(), {"bytes": size, "frames": n, "table": "global" if rows is None else "local", "colours": int(pals.shape[-2]),
                            "delta": bool(delta), "stream_bytes": [int(v) for v in lens]}


def gif_bytes(results, rh=None, delay=4, loop=0, delta=False):
    """the GIF89a file of one result (palette, indices, shape: what write_png takes) or of a list of them of one shape as bytes, built
    on the device (include/rhccq.h "GIF files written on the device").  One global colour table when every result carries the same
    palette (the same object, or equal rows), else a local table a frame.  delay: centiseconds, one number or one a frame; loop: the
    animation's repeat count, 0 for ever.  delta=True (global table, at most 255 rows): a pixel that equals the frame in front is
    written as the transparent index.  An index past the palette shows row 0, as in write_png."""
    return gif_file(results, rh, delay, loop, delta)[0]


def write_gif(results, filename, rh=None, delay=4, loop=0, delta=False):
    """gif_bytes written to `filename`; returns the file's length in bytes"""
    data = gif_bytes(results, rh, delay, loop, delta)
    with open(filename, "wb") as f:
        f.write(data)
    return len(data)


def load_compressed_device(path, rh=None):
    """load_compressed with the outer zlib layer inflated on the device: the framing is read on the host, the pickle comes
    back through page-locked memory and is parsed by the same allow-list unpickler.  Returns the same dict."""
    rh = rh or default_context()
    with open(path, "rb") as f:
        if f.read(5) != b"RHCCQ":
            raise ValueError("Invalid file format")
        size = struct.unpack("<I", f.read(4))[0]
        body = f.read(size)
    raw = rh.to_host(rh.zlib_decompress(body)).tobytes()
    return _SafeUnpickler(io.BytesIO(raw)).load()


_DTYPES = {"uint8": (1, torch.uint8), "uint16": (2, torch.int16), "uint32": (4, torch.int32)}


def lossless_decompress_device(pkg, rh=None):
    """lossless_decompress with "p" and "i" inflated on the device -> (palette uint8[l, 3] device, indices device tensor in
    the map's dtype -- uint8, int16 holding uint16, int32 holding uint32 -- flat, shape)"""
    rh = rh or default_context()
    h, w = pkg["s"]
    n_pal = int(pkg["l"])
    pal = rh.zlib_decompress(pkg["p"])
    if pal.numel() < 3 * n_pal:
        raise RhccqError(f"palette stream of {pal.numel()} bytes, {3 * n_pal} needed for {n_pal} colours")
    raw = rh.zlib_decompress(pkg["i"])
    name = pkg.get("d", "uint16")
    if name not in _DTYPES:                     # decompress_indices_simple's rule for an unknown dtype name
        bpp = raw.numel() / (h * w) if h * w > 0 else 2
        name = "uint8" if bpp <= 1 else "uint16" if bpp <= 2 else "uint32"
    eb, dt = _DTYPES[name]
    if raw.numel() != h * w * eb:
        raise RhccqError(f"index stream of {raw.numel()} bytes, {h * w * eb} expected for a {h}x{w} {name} map")
    return pal[:3 * n_pal].reshape(n_pal, 3), raw.view(dt), (h, w)


def read_frame(path, rh=None):
    """a .rhccq file -> {"image": uint8[H, W, 3] device, "palette", "indices", "shape", "dtype"} with every zlib layer
    inflated and the palette gather done on the device (rhccq_decode: an index past the palette reads entry 0, as
    decompress_color_quantization does)"""
    rh = rh or default_context()
    pkg = load_compressed_device(path, rh)
    pal, idx, (h, w) = lossless_decompress_device(pkg, rh)
    name = {torch.uint8: "uint8", torch.int16: "uint16", torch.int32: "uint32"}[idx.dtype]
    if pal.shape[0] == 0:
        raise RhccqError("read_frame: empty palette")
    img = rh.decode(idx, pal).reshape(h, w, 3)
    return {"image": img, "palette": pal, "indices": idx, "shape": (h, w), "dtype": name}


def read_png(src, rh=None, check_crc=True):
    """a PNG file -> {"image": uint8[H, W, 3] device, "alpha": uint8[H, W] device or None, "shape": (H, W), "info": {colour_type, depth,
    interlace, chunks, idat_chunks, filter_rows}} decoded on the device (include/rhccq.h "PNG files read on the device": chunk CRCs, IDAT
    join, inflate, unfilter, expand).  src: a file name, bytes, or a uint8 device tensor holding the file (read back once for its
    framing).  Colour type 3 also gives "palette" (uint8[K, 3] device), "palette_alpha" (uint8[K] device or None), "indices" (uint8, flat)
    and "dtype" ("uint8"): what read_frame returns, so write_png, write_frame and reduce_frame's steps take it as they take a .rhccq
    file's frame.  The host reads the file once, parses its framing (rhccq_png_parse_host) and uploads it once; one read of the two status
    words and the five filter counts is the only wait.  A file the definition refuses raises RhccqError naming status and detail.
    check_crc=False skips the chunk CRCs.  Not read: interlaced files, 16-bit output (a 16-bit sample gives its high byte), gamma and
    colour-management chunks, APNG."""
    from .ops import PNG_STATUS, png_parse
    rh = rh or default_context()
    if isinstance(src, torch.Tensor):
        if src.dtype != torch.uint8:
            raise RhccqError("read_png: a file name, bytes or a uint8 device tensor is required")
        data, file = rh.to_host(src.reshape(-1).to(rh.device)).tobytes(), src
    elif isinstance(src, (bytes, bytearray, memoryview)):
        data = bytearray(src)                                    # (writable: torch takes the buffer as it is)
        file = np.frombuffer(data, np.uint8)
    else:
        with open(src, "rb") as f:
            data = bytearray(os.fstat(f.fileno()).st_size)
            del data[f.readinto(data):]
        file = np.frombuffer(data, np.uint8)
    info, table = png_parse(data)

    def refuse(status, detail):
        raise RhccqError(f"read_png: RHCCQ_PNG_{PNG_STATUS[status]} (status {status}), detail {detail}")
    if info.status:
        refuse(info.status, info.detail)
    out = rh.png_decode(file, info, table, check_crc=check_crc)
    H, W = info.height, info.width
    types = out["scan"][::info.rowbytes + 1]
    rows = (types.unsqueeze(1) == torch.arange(5, device=types.device, dtype=torch.uint8)).sum(0)
    status, rows = rh.to_host(out["status"], rows)
    if int(status[0]):
        refuse(int(status[0]), int(status[1]))
    res = {"image": out["rgb"], "alpha": out["alpha"], "shape": (H, W),
           "info": {"colour_type": info.colour_type, "depth": info.depth, "interlace": info.interlace, "chunks": info.n_chunks, "idat_chunks": info.n_idat,
                    "filter_rows": [int(v) for v in rows]}}
    if info.colour_type == 3:
        K = info.palette_rows
        res["palette"] = out["file"][info.plte_offset:info.plte_offset + 3 * K].reshape(K, 3).clone()
        res["palette_alpha"] = None
        if info.trns_bytes:
            res["palette_alpha"] = torch.full((K,), 255, dtype=torch.uint8, device=rh.device)
            res["palette_alpha"][:info.trns_bytes] = out["file"][info.trns_offset:info.trns_offset + info.trns_bytes]
        res["indices"] = out["indices"].reshape(-1)
        res["dtype"] = "uint8"
    return res


def read_gif(src, rh=None):
    """a GIF file (87a or 89a, animated or not) -> {"images": uint8[F, H, W, 3] device, "alpha": uint8[F, H, W] device, "shape": (H, W),
    "loop": the file's loop count or None, "delays": [centiseconds a frame], "frames": [{"rect": (x, y, w, h), "interlaced", "disposal",
    "transparent": index or None, "palette": uint8[k, 3] (the frame's table, local or global), "indices": uint8[h, w] device}], "stats":
    {"bytes", "frames", "segments", "stream_bytes": [a frame], "seconds"}} decoded on the device (include/rhccq.h "GIF files read on the
    device": sub-block join, Clear-to-Clear parallel LZW decode, composition).  images[f] is the logical screen after frame f painted
    (transparency and the disposal methods applied); alpha[f] is 255 where some frame has painted and 0 elsewhere, and such an uncovered
    pixel has colour (0, 0, 0).  src: a file name or bytes.  The host reads the file once, parses its framing (rhccq_gif_parse_host) and
    uploads it once; one read of the status words is the only wait.  A file the definition refuses raises RhccqError naming status and
    detail (its .status and .detail carry them).  Not done: the plain-text extension is skipped, not drawn; the background colour index
    is ignored."""
    from .ops import GIF_READ_STATUS, gif_parse
    rh = rh or default_context()
    t0 = time.perf_counter()
    if isinstance(src, (bytes, bytearray, memoryview)):
        data = bytearray(src)
    else:
        with open(src, "rb") as f:
            data = bytearray(os.fstat(f.fileno()).st_size)
            del data[f.readinto(data):]
    parsed = gif_parse(data)
    info, table = parsed[0], parsed[1]

    def refuse(status, detail):
        e = RhccqError(f"read_gif: RHCCQ_GIFR_{GIF_READ_STATUS[status]} (status {status}), detail {detail}")
        e.status, e.detail = status, detail
        raise e
    if info.status:
        refuse(info.status, info.detail)
    out = rh.gif_decode(np.frombuffer(data, np.uint8), parsed)
    status, head = rh.to_host(out["status"], out["head"])
    if int(status[0]):
        refuse(int(status[0]), int(status[1]))
    host = np.frombuffer(data, np.uint8)
    frames = []
    for f in range(info.n_frames):
        fr = table[f]
        at = fr.pixel_offset
        frames.append({"rect": (fr.x, fr.y, fr.w, fr.h), "interlaced": bool(fr.interlace), "disposal": fr.disposal,
                       "transparent": None if fr.transparent < 0 else fr.transparent,
                       "palette": host[fr.table_offset:fr.table_offset + 3 * fr.table_rows].reshape(-1, 3).copy(),
                       "indices": out["indices"][at:at + fr.w * fr.h].reshape(fr.h, fr.w)})
    return {"images": out["rgb"], "alpha": out["alpha"], "shape": (info.height, info.width), "loop": None if info.loop < 0 else info.loop,
            "delays": [table[f].delay for f in range(info.n_frames)], "frames": frames,
            "stats": {"bytes": len(data), "frames": info.n_frames, "segments": int(head[2]) & 0xFFFFFFFF,
                      "stream_bytes": [table[f].stream_bytes for f in range(info.n_frames)], "seconds": round(time.perf_counter() - t0, 4)}}


def reduce_gif(src, dst, colours, rh=None, delta=True, refine=0, pattern=None, pattern_size=4):
    """an animated GIF to one of at most `colours` colours, on the device from end to end: read_gif, then ImageEncoder.animate over the
    composed frames with the file's own delays and loop count (0 where it has none), written to dst.  The frames enter as the viewer
    shows them, so cropped rectangles, transparency and disposal methods are gone from the result; a pixel no frame has covered enters
    as colour (0, 0, 0).  -> animate's dict, with stats["read"] = read_gif's stats."""
    from .image import ImageEncoder
    rh = rh or default_context()
    src = read_gif(src, rh)
    enc = ImageEncoder(rh)
    res = enc.animate(src["images"], colours, gif_path=dst, delay=src["delays"], loop=src["loop"] or 0, delta=delta, refine=refine, pattern=pattern,
                      pattern_size=pattern_size)
    res["stats"]["read"] = src["stats"]
    return res


def index_histogram(indices, n_rows, rh=None, weights=None):
    """how often every palette row is used: int64[n_rows] on the device from an index map (uint8, int16 holding uint16, int32 or
    int64, any shape), by torch.bincount.  An index past the palette counts for row 0, the row a decoder shows for it.  weights:
    an int64 tensor with one element per index, added instead of 1."""
    rh = rh or default_context()
    wide = indices.reshape(-1).to(torch.int64)
    if indices.dtype == torch.int16:
        wide = wide & 0xFFFF
    wide = torch.where(wide < n_rows, wide, torch.zeros_like(wide))
    if weights is None:
        return torch.bincount(wide, minlength=n_rows)
    # float64 weights: every partial sum is an integer below 2^53, so the sums are exact
    return torch.bincount(wide, weights=weights.reshape(-1).to(torch.float64), minlength=n_rows).to(torch.int64)


def reduce_png(src, dst, colours, rh=None, exact=False):
    """reduce_frame for a palette PNG (colour type 3): read_png, the same reduction over the file's own PLTE and index map, write_png at
    the end.  -> reduce_frame's dict ("bytes" is the PNG file's length).  Any other colour type raises RhccqError."""
    rh = rh or default_context()
    fr = read_png(src, rh)
    if "palette" not in fr:
        raise RhccqError(f"reduce_png: a palette PNG (colour type 3) is required, the file has colour type {fr['info']['colour_type']}")
    return _reduce_read(fr, write_png, "reduce_png", dst, colours, rh, exact)


def reduce_frame(src, dst, colours, rh=None, exact=False):
    """a .rhccq file to one of at most `colours` palette rows, without the source image: read_frame, the histogram of the indices,
    Rhccq.palette_reduce (exact pairwise merging, include/rhccq.h), every index through the reduction's map (no pixel carries an
    unused row, so no -1 is read), write_frame.  A file that has no more than `colours` used rows only loses its unused ones.
    -> {"from": rows read, "to": rows written, "bytes": write_frame's value, "psnr": the new decode against the old decode (inf
    when nothing merged)}.  The palette may have at most ops.palette_reduce_max_rows() rows (RhccqError)."""
    rh = rh or default_context()
    return _reduce_read(read_frame(src, rh), write_frame, "reduce_frame", dst, colours, rh, exact)


def _reduce_read(fr, write, fn, dst, colours, rh, exact):
    """reduce_frame's steps behind the read: fr is read_frame's or read_png's dict, write is write_frame or write_png"""
    from .ops import psnr_from_sse
    pal = fr["palette"].contiguous()
    K = int(pal.shape[0])
    if int(colours) < 1:
        raise ValueError(f"{fn}: colours >= 1 is expected")
    h, w = fr["shape"]
    wide = fr["indices"].reshape(-1).to(torch.int32)
    if fr["indices"].dtype == torch.int16:
        wide = wide & 0xFFFF
    wide = torch.where(wide < K, wide, torch.zeros_like(wide)).contiguous()
    new_pal, _, map_, _ = rh.palette_reduce(pal, index_histogram(wide, K, rh), min(int(colours), K))
    idx = rh.remap(wide, map_.contiguous())
    res = {"palette": rh.to_host(new_pal), "indices": idx, "shape": (h, w)}
    size = write(res, dst, rh, exact=exact)
    one_class = torch.zeros((h, w), dtype=torch.uint8, device=rh.device)
    row = rh.class_error_sums_indexed(fr["image"].contiguous(), idx, new_pal.contiguous(), one_class, 1)[0]
    return {"from": K, "to": int(new_pal.shape[0]), "bytes": size, "psnr": psnr_from_sse(int(row[0]) + int(row[1]) + int(row[2]), h * w)}
