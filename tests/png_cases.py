"""Shared cases of the PNG-writing tests (tests/test_png_write_cpu.py, tests/test_gpu_png_write.py): a plain helper module, not a
conftest.

`scanlines_reference` and `png_reference` are the numpy / struct / zlib statement of the file include/rhccq.h defines ("indexed PNG files
written on the device"), `chunks` a small chunk parser.  Every case and every reference is computed once per process and shared (do not
modify what the cached functions return).  The cases are the smallest shapes at which each part can go wrong; the module asserts its own
preconditions (the "every filter" picture really has all five types winning, the flat picture really ties)."""
import ctypes as C
import functools
import struct
import zlib

import numpy as np

E_ARG, E_LIMIT = -1, -3
EXACT, DEPTH8, NO_FILTER = 1, 2, 4
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CRC_PIECE = 16384                      # bytes of a workgroup's piece (csrc/png_write.h: 256 lanes x 64 bytes)
CRC_SEGMENT = 256 * CRC_PIECE          # the combining workgroup's lanes take one piece each up to here, then several


def depth_of(K, depth8=False):
    if K > 256:
        return 8
    if depth8 or K > 16:
        return 8
    return 1 if K <= 2 else 2 if K <= 4 else 4


def clamped(idx, K):
    idx = np.asarray(idx).astype(np.int64)
    return np.where((idx >= 0) & (idx < K), idx, 0)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def scanlines_reference(idx, palette, depth8=False, filter=True):
    """-> (scan uint8[H * row bytes], filter_rows int64[5], costs int64[H, 5] or None for colour type 3)"""
    palette = np.asarray(palette, np.uint8).reshape(-1, 3)
    K = len(palette)
    idx = clamped(idx, K)
    H, W = idx.shape
    if K <= 256:
        d = depth_of(K, depth8)
        ppb = 8 // d
        nb = (W * d + 7) // 8
        padded = np.zeros((H, nb * ppb), np.int64)
        padded[:, :W] = idx
        packed = np.zeros((H, nb), np.int64)
        for j in range(ppb):
            packed = (packed << d) | padded[:, j::ppb]
        rows = np.concatenate([np.zeros((H, 1), np.int64), packed], axis=1).astype(np.uint8)
        return rows.reshape(-1), np.array([H, 0, 0, 0, 0], np.int64), None
    raw = palette[idx].astype(np.int64).reshape(H, 3 * W)
    a = np.zeros_like(raw)
    a[:, 3:] = raw[:, :-3]
    b = np.zeros_like(raw)
    b[1:] = raw[:-1]
    c = np.zeros_like(raw)
    c[1:, 3:] = raw[:-1, :-3]
    filtered = np.stack([raw, raw - a, raw - b, raw - (a + b) // 2, raw - _paeth(a, b, c)]) & 255          # [5, H, 3 W]
    costs = np.where(filtered < 128, filtered, 256 - filtered).sum(axis=2).T                             # [H, 5]
    best = costs.argmin(axis=1) if filter else np.zeros(H, np.int64)                                      # (argmin: the first minimum)
    chosen = filtered[best, np.arange(H)]
    rows = np.concatenate([best[:, None], chosen], axis=1).astype(np.uint8)
    return rows.reshape(-1), np.bincount(best, minlength=5).astype(np.int64), costs


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_reference(idx, palette, depth8=False, filter=True, stream=None):
    """the whole file; stream: IDAT's data (default zlib.compress(scanlines, 9), what RHCCQ_PNG_EXACT writes)"""
    palette = np.asarray(palette, np.uint8).reshape(-1, 3)
    K = len(palette)
    H, W = np.asarray(idx).shape
    scan = scanlines_reference(idx, palette, depth8, filter)[0].tobytes()
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth_of(K, depth8), 3 if K <= 256 else 2, 0, 0, 0))
    if K <= 256:
        out += chunk(b"PLTE", palette.tobytes())
    return out + chunk(b"IDAT", zlib.compress(scan, 9) if stream is None else stream) + chunk(b"IEND", b"")


def chunks(data):
    """a PNG file -> [(type, data, stored crc, zlib.crc32 of type + data)]; asserts the signature and that nothing is left over"""
    data = bytes(data)
    assert data[:8] == SIGNATURE
    out, p = [], 8
    while p < len(data):
        n, kind = struct.unpack(">I", data[p:p + 4])[0], data[p + 4:p + 8]
        body = data[p + 8:p + 8 + n]
        assert len(body) == n and p + 12 + n <= len(data), "truncated chunk"
        out.append((kind, body, struct.unpack(">I", data[p + 8 + n:p + 12 + n])[0], zlib.crc32(kind + body)))
        p += 12 + n
    assert p == len(data)
    return out


def decoded(idx, palette):
    """what a viewer shows: palette[clamped idx]"""
    palette = np.asarray(palette, np.uint8).reshape(-1, 3)
    return palette[clamped(idx, len(palette))]


def pillow_image(data):
    """-> (mode, uint8[H, W, 3], PLTE's entries as uint8[n, 3] or None) by Pillow"""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(data)))
    im.load()
    pal = None
    if im.mode == "P":
        pal = np.array(im.getpalette(), np.uint8).reshape(-1, 3)
    return im.mode, np.asarray(im.convert("RGB")), pal


# ---- the cases: name -> (idx int64[H, W], palette uint8[K, 3], depth8, filter) ---------------------------------------------------------
def _palette(K, seed):
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(0, 256, (K, 3)).astype(np.uint8)


def _random(H, W, K, seed, hi=None):
    rng = np.random.default_rng(seed)
    return rng.integers(0, K if hi is None else hi, (H, W)).astype(np.int64)


def five_bands(K=300):
    """40 x 64: five 8-row bands (horizontal ramp, vertical ramp, diagonal, noise, flat) over a grey-ramp palette with distinct rows"""
    pal = np.zeros((K, 3), np.uint8)
    g = np.arange(K)
    pal[:, 0], pal[:, 1], pal[:, 2] = g % 256, (g * 7) % 256, (g // 256) * 80 + (g % 256) // 4
    y, x = np.mgrid[0:8, 0:64]
    rng = np.random.default_rng(5)
    bands = [3 * x + 0 * y, 20 * y + 40 + 0 * x, (5 * x + 9 * y) % 256, rng.integers(0, K, (8, 64)), np.full((8, 64), 77)]
    return np.concatenate(bands).astype(np.int64), pal


@functools.lru_cache(maxsize=None)
def _cases():
    c = {}
    for K in (1, 2):
        for W in (1, 7, 8, 9):
            c[f"d1_k{K}_w{W}"] = (_random(3, W, K, W), _palette(K, K), False, True)
    for K in (3, 4):
        for W in (3, 4, 5):
            c[f"d2_k{K}_w{W}"] = (_random(3, W, K, 10 + W), _palette(K, K), False, True)
    for K in (5, 16):
        for W in (1, 2, 3):
            c[f"d4_k{K}_w{W}"] = (_random(3, W, K, 20 + W), _palette(K, K), False, True)
    for K in (17, 255, 256):
        c[f"d8_k{K}"] = (_random(5, 13, K, 30 + K), _palette(K, K), False, True)
    for K, W in ((2, 9), (4, 5), (16, 3), (256, 11)):
        c[f"h1_k{K}"] = (_random(1, W, K, 40 + K), _palette(K, K), False, True)
    for K in (2, 4, 16, 200):
        c[f"wg3x701_k{K}"] = (_random(3, 701, K, 50 + K), _palette(K, K), False, True)
        c[f"wg5x4099_k{K}"] = (_random(5, 4099, K, 60 + K), _palette(K, K), False, True)
    for K in (2, 3, 16, 100):
        c[f"clamp_k{K}"] = (_random(4, 37, K, 70 + K, hi=K + 40), _palette(K, K), False, True)
    c["clamp_k300"] = (_random(4, 37, 300, 75, hi=70000), _palette(300, 300), False, True)
    c["depth8_k2"] = (_random(3, 9, 2, 80), _palette(2, 2), True, True)
    for K in (257, 300):
        for H, W in ((1, 1), (1, 5), (6, 1), (9, 33)):
            c[f"rgb_k{K}_{H}x{W}"] = (_random(H, W, K, 90 + H + W), _palette(K, K), False, True)
    c["rgb_w256"] = (_random(5, 256, 400, 94), _palette(400, 400), False, True)             # the widest row a single wave takes
    c["rgb_wide"] = (_random(6, 300, 1000, 95), _palette(1000, 1000), False, True)           # a workgroup a row, some lanes without a pixel
    c["rgb_wider"] = (_random(3, 1100, 300, 96), _palette(300, 300), False, True)            # a lane takes several pixels of a row
    idx, pal = five_bands()
    c["rgb_bands"] = (idx, pal, False, True)
    c["rgb_bands_nofilter"] = (idx, pal, False, False)
    c["rgb_bands_wide"] = (np.tile(idx, (1, 5)), pal, False, True)                           # 40 x 320: the reduction across a workgroup's waves
    flat = _palette(300, 7)
    flat[123] = 0                      # a flat BLACK picture: every filtered byte is 0 under every filter (any other colour lets Up win)
    c["rgb_flat"] = (np.full((6, 10), 123, np.int64), flat, False, True)
    for v in c.values():
        v[0].setflags(write=False)
        v[1].setflags(write=False)
    return c


def names():
    return list(_cases())


def case(name):
    return _cases()[name]


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (scan uint8[...], filter_rows int64[5], costs)"""
    idx, pal, depth8, flt = case(name)
    out = scanlines_reference(idx, pal, depth8, flt)
    out[0].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_file(name):
    idx, pal, depth8, flt = case(name)
    return png_reference(idx, pal, depth8, flt)


def flags_of(name, exact=True):
    _, _, depth8, flt = case(name)
    return (EXACT if exact else 0) | (DEPTH8 if depth8 else 0) | (0 if flt else NO_FILTER)


def index_widths(K):
    """the element widths that hold rows below K"""
    return (1, 2, 4) if K <= 256 else (2, 4)


def index_array(idx, eb):
    """int64 indices in the storage of width eb; values past the type wrap as the storage does (they stay >= K in these cases or are
    taken out before by the caller)"""
    return np.ascontiguousarray(np.asarray(idx).astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[eb]))


def storable(name, eb):
    """whether the case's indices (clamp cases go past K) fit the width without changing what the clamp sees"""
    idx, pal, _, _ = case(name)
    lim = 1 << (8 * eb)
    return len(pal) <= lim and int(idx.max()) < lim


def _check_preconditions():
    _, rows, costs = reference("rgb_bands")
    assert (rows > 0).all(), rows                                    # every filter wins at least one row
    assert (reference("rgb_bands_wide")[1] > 0).all()
    _, rows, costs = reference("rgb_flat")
    assert rows.tolist() == [6, 0, 0, 0, 0]
    assert all(len(set(r)) == 1 for r in costs.tolist()), costs       # all five costs tie on every row: type 0 is taken
    assert reference("rgb_bands_nofilter")[1].tolist() == [40, 0, 0, 0, 0]
    for n in ("clamp_k2", "clamp_k3", "clamp_k16", "clamp_k100", "clamp_k300"):
        idx, pal, _, _ = case(n)
        assert (idx >= len(pal)).any()
    # every alignment of a row start modulo 4 occurs in the several-workgroup cases
    for n, rb in (("wg3x701_k200", 702), ("wg5x4099_k200", 4100), ("wg3x701_k2", 1 + 88), ("wg5x4099_k16", 1 + 2050)):
        idx, pal, _, _ = case(n)
        assert len(reference(n)[0]) == idx.shape[0] * rb
    assert {(y * 89) % 4 for y in range(3)} | {(y * 2051) % 4 for y in range(5)} == {0, 1, 2, 3}


_check_preconditions()


# ---- CRC cases ------------------------------------------------------------------------------------------------------------------------
CRC_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, CRC_PIECE - 1, CRC_PIECE, CRC_PIECE + 1, 2 * CRC_PIECE + 7, 1000003)
CRC_LONG = CRC_SEGMENT + 1            # one more than the combining workgroup's lanes take at one piece each: 4 MiB + 1


@functools.lru_cache(maxsize=None)
def crc_bytes(n):
    a = np.random.default_rng(n + 17).integers(0, 256, n).astype(np.uint8)
    a.setflags(write=False)
    return a


# ---- the host forms through ctypes -------------------------------------------------------------------------------------------------------
def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def lib():
    from roibasedimagecompression_amd import _lib
    return _lib.load()


def sizes(H, W, K, flags):
    s, w, b = C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib().rhccq_png_sizes(H, W, K, flags, C.byref(s), C.byref(w), C.byref(b))
    return rc, s.value, w.value, b.value


def host_scanlines(idx, pal, flags, eb):
    H, W = idx.shape
    pal = np.ascontiguousarray(pal, np.uint8)
    rc, n, _, _ = sizes(H, W, len(pal), flags)
    assert rc == 0
    scan = np.full(n + 8, 0xA5, np.uint8)
    rows = np.full(5, -1, np.int64)
    arr = index_array(idx, eb)
    rc = lib().rhccq_png_scanlines_host(_ptr(arr), eb, H, W, _ptr(pal), len(pal), flags, _ptr(scan), _ptr(rows))
    assert (scan[n:] == 0xA5).all()
    return rc, scan[:n], rows


def host_crc32(a):
    out = C.c_uint32(0xDEADBEEF)
    rc = lib().rhccq_crc32_host(_ptr(a) if len(a) else C.c_void_p(0), len(a), C.byref(out))
    return rc, out.value


def host_png(idx, pal, flags, eb):
    H, W = idx.shape
    pal = np.ascontiguousarray(pal, np.uint8)
    rc, _, _, bound = sizes(H, W, len(pal), flags)
    assert rc == 0
    out = np.full(bound + 8, 0xA5, np.uint8)
    n = C.c_int64(-1)
    arr = index_array(idx, eb)
    rc = lib().rhccq_png_encode_host(_ptr(arr), eb, H, W, _ptr(pal), len(pal), flags, _ptr(out), bound, C.byref(n))
    assert (out[bound:] == 0xA5).all()
    return rc, out[:max(n.value, 0)].tobytes()
