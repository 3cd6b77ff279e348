"""Shared cases of the GIF-writing tests (tests/test_gif_write_cpu.py, tests/test_gpu_gif_write.py): a plain helper module, not a conftest.

`lzw_reference` and `gif_reference` are the dict / struct statement of the file include/rhccq.h defines ("GIF files written on the
device"), written from that text.  Every case and every reference is computed once per process and shared (do not modify what the cached
functions return).  Frames are small: the risks sit at edges (a segment's first and last code, the width rule, the table-full Clear, the
sub-block boundaries, misaligned starts), and the module asserts that each named edge really occurs in its case."""
import ctypes as C
import functools
import struct

import numpy as np

E_ARG, E_LIMIT = -1, -3
LOCAL, DELTA, TRIE = 1, 2, 4            # TRIE: the other dictionary of the LZW step; the bytes are the same
S = 16384                                  # rhccq_gif_segment_pixels()


def table_bits(entries):
    return max(1, int(entries - 1).bit_length())


def min_code(entries):
    return max(2, table_bits(entries))


def sub_pos(o):
    return o + o // 255 + 1


def clamped(idx, K):
    idx = np.asarray(idx).astype(np.int64)
    return np.where((idx >= 0) & (idx < K), idx, 0)


# ---- the code stream ---------------------------------------------------------------------------------------------------------------------
def lzw_segment(px, m, opening, last):
    """one segment -> ([(code, width)], {"table_full": Clears for a full table, "last_widens": the width rule fired behind the last data
    code, "last_fills": next reached 4096 with the last data code})"""
    clear, end = 1 << m, (1 << m) + 1
    codes = [(clear, m + 1)] if opening else []
    table, nxt, width = {}, clear + 2, m + 1
    info = {"table_full": 0, "last_widens": False, "last_fills": False}
    cur = int(px[0])
    for k in px[1:]:
        k = int(k)
        hit = table.get((cur, k))
        if hit is not None:
            cur = hit
            continue
        codes.append((cur, width))
        if nxt < 4096:
            table[(cur, k)] = nxt
        if nxt == 1 << width and width < 12:
            width += 1
        nxt += 1
        cur = k
        if nxt == 4096:
            codes.append((clear, width))
            table, nxt, width = {}, clear + 2, m + 1
            info["table_full"] += 1
    codes.append((cur, width))
    if nxt == 1 << width and width < 12:
        width += 1
        info["last_widens"] = True
    nxt += 1
    info["last_fills"] = nxt == 4096
    codes.append((end if last else clear, width))
    return codes, info


def pack(codes):
    out, acc, fill = bytearray(), 0, 0
    for code, width in codes:
        acc |= code << fill
        fill += width
        while fill >= 8:
            out.append(acc & 255)
            acc >>= 8
            fill -= 8
    if fill:
        out.append(acc & 255)
    return bytes(out)


def lzw_reference(pixels, m, segment=S):
    """the pixels a frame writes (flat, clamped and substituted) -> (stream bytes, [info per segment])"""
    pixels = np.asarray(pixels).reshape(-1)
    codes, infos = [], []
    n = len(pixels)
    for p0 in range(0, n, segment):
        c, info = lzw_segment(pixels[p0:p0 + segment].tolist(), m, p0 == 0, p0 + segment >= n)
        codes += c
        infos.append(info)
    return pack(codes), infos


def written_pixels(frames, K, delta):
    """idx[n, H, W] -> what every frame writes: the clamp, then T = K where the frame in front shows the same"""
    c = clamped(frames, K)
    if not delta:
        return c
    out = c.copy()
    out[1:][c[1:] == c[:-1]] = K
    return out


def gif_reference(frames, palettes, delays, loop=0, delta=False, segment=S):
    """frames int[n, H, W]; palettes: ONE uint8[K, 3] (a global table) or a list of n (local tables) -> (file bytes, [stream bytes])"""
    frames = np.asarray(frames)
    n, H, W = frames.shape
    local = isinstance(palettes, (list, tuple))
    assert not (local and delta)

    def table(pal, entries):
        pal = np.asarray(pal, np.uint8).reshape(-1, 3)
        t = np.zeros((1 << table_bits(entries), 3), np.uint8)
        t[:len(pal)] = pal
        return t.tobytes()
    out = b"GIF89a"
    if local:
        out += struct.pack("<HHBBB", W, H, 0x70, 0, 0)
    else:
        K = len(palettes)
        entries = K + (1 if delta else 0)
        tb = table_bits(entries)
        out += struct.pack("<HHBBB", W, H, 0x80 | (tb - 1) << 4 | (tb - 1), 0, 0) + table(palettes, entries)
    if n > 1:
        out += b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00"
    lengths = []
    for f in range(n):
        K = len(palettes[f]) if local else len(palettes)
        entries = K + (1 if delta else 0)
        transparent = delta and f > 0
        out += b"\x21\xf9\x04" + struct.pack("<BHBB", 1 << 2 | (1 if transparent else 0), delays[f], K if transparent else 0, 0)
        out += b"\x2c" + struct.pack("<HHHHB", 0, 0, W, H, 0x80 | (table_bits(K) - 1) if local else 0)
        if local:
            out += table(palettes[f], K)
        m = min_code(entries)
        px = clamped(frames[f], K)
        if transparent:
            px = np.where(px == clamped(frames[f - 1], K), K, px)
        stream, _ = lzw_reference(px, m, segment)
        lengths.append(len(stream))
        out += bytes([m])
        for o in range(0, len(stream), 255):
            out += bytes([min(255, len(stream) - o)]) + stream[o:o + 255]
        out += b"\x00"
    return out + b"\x3b", lengths


# ---- a decoder of the framing (the tests' own, beside Pillow) ---------------------------------------------------------------------------------
def parse(data):
    """-> {"W", "H", "global": entries or 0, "loop": count or None, "frames": [{"delay", "transparent": index or None, "local", "m", "stream"}]}"""
    data = bytes(data)
    assert data[:6] == b"GIF89a"
    W, H, packed, _, _ = struct.unpack("<HHBBB", data[6:13])
    p = 13
    out = {"W": W, "H": H, "global": 0, "loop": None, "frames": []}
    if packed & 0x80:
        out["global"] = 2 << (packed & 7)
        p += 3 * out["global"]
    gce = None
    while data[p] != 0x3B:
        if data[p] == 0x21 and data[p + 1] == 0xFF:
            assert data[p + 2:p + 14] == b"\x0bNETSCAPE2.0" and data[p + 14:p + 16] == b"\x03\x01" and data[p + 18] == 0
            out["loop"] = struct.unpack("<H", data[p + 16:p + 18])[0]
            p += 19
        elif data[p] == 0x21 and data[p + 1] == 0xF9:
            assert data[p + 2] == 4 and data[p + 7] == 0
            flags, delay, t = struct.unpack("<BHB", data[p + 3:p + 7])
            assert flags >> 2 == 1
            gce = {"delay": delay, "transparent": t if flags & 1 else None}
            p += 8
        else:
            assert data[p] == 0x2C and gce is not None
            x, y, w, h, packed = struct.unpack("<HHHHB", data[p + 1:p + 10])
            assert (x, y, w, h) == (0, 0, W, H) and not packed & 0x40
            p += 10
            local = 2 << (packed & 7) if packed & 0x80 else 0
            p += 3 * local
            m = data[p]
            p += 1
            stream = b""
            while data[p]:
                stream += data[p + 1:p + 1 + data[p]]
                p += 1 + data[p]
            p += 1
            out["frames"].append(dict(gce, local=local, m=m, stream=stream))
            gce = None
    assert p == len(data) - 1
    return out


def pillow_frames(data):
    """-> (frames uint8[n, H, W, 3] as Pillow composes them, [duration in ms], loop or None)"""
    import io
    from PIL import GifImagePlugin, Image
    keep = GifImagePlugin.LOADING_STRATEGY
    GifImagePlugin.LOADING_STRATEGY = GifImagePlugin.LoadingStrategy.RGB_ALWAYS
    try:
        im = Image.open(io.BytesIO(bytes(data)))
        frames, durations = [], []
        for f in range(getattr(im, "n_frames", 1)):
            im.seek(f)
            frames.append(np.asarray(im.convert("RGB")).copy())
            durations.append(im.info.get("duration"))
        return np.stack(frames), durations, im.info.get("loop")
    finally:
        GifImagePlugin.LOADING_STRATEGY = keep


def decoded(frames, palettes):
    """what a viewer shows: palette[clamped idx] per frame"""
    frames = np.asarray(frames)
    local = isinstance(palettes, (list, tuple))
    return np.stack([np.asarray(palettes[f] if local else palettes, np.uint8)[clamped(frames[f], len(palettes[f] if local else palettes))]
                     for f in range(len(frames))])


# ---- searches with the reference -------------------------------------------------------------------------------------------------------------
def trace(px, m):
    """one pass over a segment's pixels -> for every length n = 1..len(px), had the segment (a frame's only one) ended there:
    (stream bits int64[len], next in front of the last data code, width in front of it)"""
    clear = 1 << m
    table, nxt, width, bits = {}, clear + 2, m + 1, m + 1
    cur = int(px[0])
    tot, nx, wd = [], [], []

    def ended():
        w2 = width + 1 if nxt == 1 << width and width < 12 else width
        tot.append(bits + width + w2)
        nx.append(nxt)
        wd.append(width)
    ended()
    for k in px[1:]:
        k = int(k)
        hit = table.get((cur, k))
        if hit is not None:
            cur = hit
        else:
            bits += width
            if nxt < 4096:
                table[(cur, k)] = nxt
            if nxt == 1 << width and width < 12:
                width += 1
            nxt += 1
            cur = k
            if nxt == 4096:
                bits += width
                table, nxt, width = {}, clear + 2, m + 1
        ended()
    return np.array(tot), np.array(nx), np.array(wd)


def _noise(n, K, seed):
    return np.random.default_rng(seed).integers(0, K, n).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _found():
    """lengths at which the named edges occur"""
    out = {}
    px = _noise(S, 256, 7)
    tot, nx, wd = trace(px.tolist(), 8)
    out["last_widens"] = int(np.nonzero((nx == 1 << wd) & (wd < 12))[0][1]) + 1       # the second: 1024 entries, not 512
    out["last_fills"] = int(np.nonzero(nx == 4095)[0][0]) + 1
    # a full first segment whose last code widens: a noise pixels of two rows, then a third row to the segment's end.  The parse of the noise
    # does not depend on what follows it, and a flat run of n pixels takes the least c with c (c + 1) / 2 >= n codes.
    _, nx2, _ = trace(_noise(S, 2, 11).tolist(), 2)
    a = np.arange(1, S)
    flat_codes = np.ceil((np.sqrt(8.0 * (S - a) + 1) - 1) / 2).astype(np.int64)
    last_next = nx2[a - 1] + flat_codes
    out["closing_clear_widens"] = int(a[np.nonzero((last_next == 512) | (last_next == 1024) | (last_next == 256))[0][0]])
    px4 = _noise(4000, 4, 8)
    tot4, _, _ = trace(px4.tolist(), 2)
    by = (tot4 + 7) // 8
    for r in (0, 1, 254):
        out[f"mod{r}"] = int(np.nonzero((by % 255 == r) & (by > 255))[0][0]) + 1
    return out


# ---- the cases: name -> {"frames": int64[n, H, W], "palettes": uint8[K, 3] or [uint8[K_f, 3]], "delays": [..], "loop", "delta"} --------------
def _palette(K, seed):
    return np.random.default_rng(2000 + seed).integers(0, 256, (K, 3)).astype(np.uint8)


def _case(frames, palettes, delays=None, loop=0, delta=False):
    frames = np.asarray(frames, np.int64)
    if frames.ndim == 2:
        frames = frames[None]
    return {"frames": frames, "palettes": palettes, "delays": list(delays) if delays else [4 + f for f in range(len(frames))], "loop": loop,
            "delta": delta}


@functools.lru_cache(maxsize=None)
def _cases():
    c = {}
    found = _found()
    # pixel counts and shapes around the segment length
    c["px1"] = _case(np.array([[2]]), _palette(5, 1))
    c["row_s_minus_1"] = _case(_noise(S - 1, 16, 2).reshape(1, S - 1), _palette(16, 2))
    c["col_s"] = _case(_noise(S, 17, 3).reshape(S, 1), _palette(17, 3))
    c["s_plus_1"] = _case(_noise(S + 1, 5, 4).reshape(113, 145), _palette(5, 4))               # the last segment is one pixel
    c["two_s_plus_1"] = _case(np.full((99, 331), 3), _palette(4, 5))                           # flat: one string grows to each segment's end
    y, x = np.mgrid[0:128, 0:385]
    c["ramp_3s"] = _case((x * 255 // 384 + y) % 256, _palette(256, 6))                          # about 3 S pixels
    # K and the table bits
    for K in (1, 2, 3, 4, 5, 16, 17, 255, 256):
        c[f"k{K}"] = _case(_noise(37 * 53, K, 10 + K).reshape(37, 53), _palette(K, K))
    # the dictionary fills: uniform noise at K = 256 over a full segment
    c["noise_full"] = _case(_noise(S, 256, 7).reshape(128, 128), _palette(256, 7))
    c["last_widens"] = _case(_noise(S, 256, 7)[:found["last_widens"]].reshape(1, -1), _palette(256, 7))
    c["last_fills"] = _case(_noise(S, 256, 7)[:found["last_fills"]].reshape(1, -1), _palette(256, 7))
    head = found["closing_clear_widens"]                                 # segment 0: `head` noise pixels of rows 0 and 1, then row 2 to its end
    c["closing_clear_widens"] = _case(np.concatenate([_noise(S, 2, 11)[:head], np.full(S - head, 2), _noise(100, 3, 12)]).reshape(1, -1), _palette(3, 7))
    for r in (0, 1, 254):
        c[f"sub_mod{r}"] = _case(_noise(4000, 4, 8)[:found[f"mod{r}"]].reshape(1, -1), _palette(4, 8))
    # indices past the palette
    c["clamp_k100"] = _case(_noise(37 * 53, 140, 20).reshape(37, 53), _palette(100, 20))
    c["clamp_wide"] = _case(_noise(37 * 53, 70000, 21).reshape(37, 53), _palette(200, 21))
    # several frames
    rng = np.random.default_rng(30)
    for K in (3, 4, 15, 16, 127, 128, 255):                              # T = K is the table's last entry, or opens a larger table
        a = _noise(37 * 53, K, 30 + K).reshape(37, 53)
        b = np.where(rng.random((37, 53)) < 0.7, a, _noise(37 * 53, K, 40 + K).reshape(37, 53))
        c[f"delta_k{K}"] = _case(np.stack([a, b]), _palette(K, K), delta=True, loop=K)
    a = _noise(S + 77, 40, 50).reshape(1, -1)
    frames = np.stack([a, a, np.where(rng.random(a.shape) < 0.9, a, 7), a + 0, _noise(S + 77, 60, 51).reshape(1, -1)])
    c["delta_five"] = _case(frames, _palette(40, 50), delays=[0, 1, 65535, 10, 7], loop=65535, delta=True)   # 1 and 3 are all T; 4 goes past K
    c["plain_five"] = _case(frames, _palette(40, 50), delays=[0, 1, 65535, 10, 7], loop=3)
    c["plain_two"] = _case(frames[[0, 4]], _palette(64, 52), loop=0)
    c["local_mixed"] = [_noise(37 * 53, k, 60 + k).reshape(37, 53) for k in (2, 200, 17, 256, 5)]
    c["local_mixed"] = _case(np.stack(c["local_mixed"]), [_palette(k, 60 + k) for k in (2, 200, 17, 256, 5)])
    c["local_one"] = _case(_noise(300, 9, 70).reshape(12, 25), [_palette(9, 70)])
    for v in c.values():
        v["frames"].setflags(write=False)
    return c


def names():
    return list(_cases())


def case(name):
    return _cases()[name]


def flags_of(name):
    v = case(name)
    return (LOCAL if isinstance(v["palettes"], list) else 0) | (DELTA if v["delta"] else 0)


def rows_of(name):
    v = case(name)
    return [len(p) for p in v["palettes"]] if isinstance(v["palettes"], list) else [len(v["palettes"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (file bytes, [stream bytes per frame])"""
    v = case(name)
    return gif_reference(v["frames"], v["palettes"], v["delays"], v["loop"], v["delta"])


@functools.lru_cache(maxsize=None)
def reference_streams(name):
    """-> [the code stream of every frame]"""
    return [f["stream"] for f in parse(reference(name)[0])["frames"]]


def index_array(frames, eb):
    return np.ascontiguousarray(np.asarray(frames).astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[eb]))


def widths(name):
    """the element widths that hold the case's indices without changing what the clamp sees"""
    top = int(case(name)["frames"].max())
    return [eb for eb in (1, 2, 4) if top < 1 << (8 * eb)]


def _check_preconditions():
    def infos(name, f=0):
        v = case(name)
        K = rows_of(name)[0]
        px = written_pixels(v["frames"], K, v["delta"])[f]
        return lzw_reference(px, min_code(K + (1 if v["delta"] else 0)))[1]
    assert infos("noise_full")[0]["table_full"] >= 2
    assert infos("last_widens")[0]["last_widens"] and infos("last_fills")[0]["last_fills"] and not infos("last_fills")[0]["table_full"]
    two = infos("closing_clear_widens")
    assert len(two) == 2 and two[0]["last_widens"]                       # the closing Clear of segment 0 is one bit wider
    assert case("s_plus_1")["frames"].size == S + 1 and case("two_s_plus_1")["frames"].size == 2 * S + 1
    assert case("row_s_minus_1")["frames"].size == S - 1 and case("col_s")["frames"].size == S
    for r in (0, 1, 254):
        n = reference(f"sub_mod{r}")[1][0]
        assert n % 255 == r and n > 255, (r, n)
    assert (case("clamp_k100")["frames"] >= 100).any() and (case("clamp_wide")["frames"] >= 65536).any()
    five = written_pixels(case("delta_five")["frames"], 40, True)
    assert (five[1] == 40).all() and (five[3] != 40).any() and (five[2] == 40).mean() > 0.8
    assert (case("delta_five")["frames"][4] >= 40).any()
    assert [min_code(K + 1) for K in (3, 4, 15, 16, 127, 128, 255)] == [2, 3, 4, 5, 7, 8, 8]
    assert [table_bits(K) for K in (1, 2, 3, 4, 5, 16, 17, 255, 256)] == [1, 1, 2, 2, 3, 4, 5, 8, 8]
    assert [sub_pos(o) for o in (0, 1, 254, 255, 256, 509, 510, 511)] == [1, 2, 255, 257, 258, 511, 513, 514]


_check_preconditions()


# ---- the host forms through ctypes -------------------------------------------------------------------------------------------------------
def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def lib():
    from roibasedimagecompression_amd import _lib
    return _lib.load()


def sizes(n, H, W, flags):
    w, s, b = C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib().rhccq_gif_sizes(n, H, W, flags, C.byref(w), C.byref(s), C.byref(b))
    return rc, w.value, s.value, b.value


def palette_block(name):
    """-> (uint8 palettes as rhccq_gif_encode takes them, k_stride, int32 k_rows)"""
    v = case(name)
    rows = rows_of(name)
    if not isinstance(v["palettes"], list):
        return np.ascontiguousarray(v["palettes"], np.uint8), rows[0], np.array(rows, np.int32)
    stride = max(rows)
    block = np.full((len(rows), stride, 3), 0xEE, np.uint8)               # (rows past k_rows[f] must not reach the file)
    for f, p in enumerate(v["palettes"]):
        block[f, :len(p)] = p
    return block, stride, np.array(rows, np.int32)


def shifted(arr, shift):
    """a copy of the array whose first byte lies `shift` bytes (a multiple of the element) behind a 16-byte boundary"""
    raw = np.zeros(arr.nbytes + 32, np.uint8)
    at = (-raw.ctypes.data) % 16 + shift
    out = raw[at:at + arr.nbytes].view(arr.dtype).reshape(arr.shape)
    out[...] = arr
    return out


def host_lzw(name, eb, shift=0, trie=False):
    v = case(name)
    n, H, W = v["frames"].shape
    flags = flags_of(name) | (TRIE if trie else 0)
    rc, _, stride, _ = sizes(n, H, W, flags)
    assert rc == 0
    arr = shifted(index_array(v["frames"], eb), shift)
    streams = np.full((n, stride + 8), 0xA5, np.uint8)
    lens = np.full(n, -1, np.int64)
    rc = lib().rhccq_gif_lzw_host(_ptr(arr), eb, n, H, W, _ptr(np.array(rows_of(name), np.int32)), flags, _ptr(streams), stride + 8, _ptr(lens))
    assert all((streams[f, max(lens[f], 0):] == 0xA5).all() for f in range(n)), "bytes behind a stream were written"
    return rc, [streams[f, :lens[f]].tobytes() for f in range(n)]


def host_gif(name, eb, shift=0, trie=False):
    v = case(name)
    n, H, W = v["frames"].shape
    flags = flags_of(name) | (TRIE if trie else 0)
    rc, _, _, bound = sizes(n, H, W, flags)
    assert rc == 0
    arr = shifted(index_array(v["frames"], eb), shift)
    pal, stride, rows = palette_block(name)
    out = np.full(bound + 8, 0xA5, np.uint8)
    length = C.c_int64(-1)
    lens = np.full(n, -1, np.int64)
    rc = lib().rhccq_gif_encode_host(_ptr(arr), eb, n, H, W, _ptr(pal), stride, _ptr(rows), _ptr(np.array(v["delays"], np.int32)), v["loop"], flags,
                                     _ptr(out), bound, C.byref(length), _ptr(lens))
    assert (out[max(length.value, 0):] == 0xA5).all(), "bytes behind the file were written"
    return rc, out[:max(length.value, 0)].tobytes(), lens.tolist()


def write_corpus(folder):
    """every case as files the native test reads: NAME.in (a header of int32: n, H, W, flags, loop, k_stride, then k_rows[n], delays[n]; the
    palettes; the uint32 indices) and NAME.gif (the reference's file) -> the names"""
    import os
    for name in names():
        v = case(name)
        n, H, W = v["frames"].shape
        pal, stride, rows = palette_block(name)
        k_rows = np.resize(rows, n).astype(np.int32)
        head = np.array([n, H, W, flags_of(name), v["loop"], stride], np.int32)
        with open(os.path.join(folder, name + ".in"), "wb") as f:
            f.write(head.tobytes() + k_rows.tobytes() + np.array(v["delays"], np.int32).tobytes() + np.ascontiguousarray(pal).tobytes())
            f.write(index_array(v["frames"], 4).tobytes())
        with open(os.path.join(folder, name + ".gif"), "wb") as f:
            f.write(reference(name)[0])
    return names()
