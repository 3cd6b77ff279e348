"""The optimising JPEG writer's cases (include/rhccq.h "JPEG files written with optimised Huffman tables"): the smallest pictures at which
each part can go wrong, the reference the bytes Pillow saves with optimize=True; synthetic symbol counts, the reference libjpeg's
jpeg_gen_optimal_table stated in plain Python."""
import ctypes as C
import functools
import io

import numpy as np
from PIL import Image

import jpeg_cases as J
from jpegwrite_cases import MODE

# name -> (H, W, mode, quality, restart rows, noise amplitude)
CASES = {
    "1x1_grey": (1, 1, "grey", 75, 0, 128),                 # one block; a DC table of one real symbol
    "8x8_flat": (8, 8, "444", 90, 0, 0),                    # two symbols a table
    "17x23_420": (17, 23, "420", 85, 0, 128),               # dummy blocks: their repeated DC feeds the DC counts
    "17x23_422": (17, 23, "422", 85, 0, 128),
    "40x56_rst": (40, 56, "420", 75, 1, 128),               # several intervals: the DC reset changes the histogram
    "64x64_q100": (64, 64, "444", 100, 0, 255),             # near-complete AC tables, ZRL
    "33x70_q5": (33, 70, "444", 5, 0, 128),                 # almost only EOB: every lane of a wave on one symbol
    "264x200_444": (264, 200, "444", 75, 0, 128),           # 2475 blocks: more than the histogram grid's first stride, many flushes
}


@functools.lru_cache(maxsize=None)
def image(name):
    H, W, mode, _, _, amp = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    yy, xx = np.mgrid[0:H, 0:W]
    img = (rng.integers(0, amp + 1, (H, W, 3)) + ((yy + 2 * xx)[..., None] if amp == 128 else 0 if amp else 97)).clip(0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[..., 0] if mode == "grey" else img)


@functools.lru_cache(maxsize=None)
def pillow(name):
    _, _, mode, quality, rows, _ = CASES[name]
    out, kw = io.BytesIO(), {"restart_marker_rows": rows} if rows else {}
    if mode != "grey":
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[mode]
    Image.fromarray(image(name)).save(out, "JPEG", quality=quality, optimize=True, **kw)
    return out.getvalue()


@functools.lru_cache(maxsize=None)
def host(name):
    """the host forms -> (coefficients, counts uint32[4, 256], the file's bytes)"""
    lib, img = J.lib(), image(name)
    H, W, mode, quality, rows, _ = CASES[name]
    sizes = [C.c_int64() for _ in range(4)]
    assert lib.rhccq_jpeg_optimize_sizes(H, W, MODE[mode], quality, rows, *[C.byref(s) for s in sizes]) == 0
    coef, counts, out, n = np.zeros((sizes[0].value // 64, 64), np.int16), np.zeros((4, 256), np.uint32), np.zeros(sizes[3].value, np.uint8), C.c_int64()
    assert lib.rhccq_jpeg_blocks_host(J._ptr(img), H, W, MODE[mode], quality, J._ptr(coef)) == 0
    assert lib.rhccq_jpeg_histogram_host(J._ptr(coef), H, W, MODE[mode], rows, J._ptr(counts)) == 0
    assert lib.rhccq_jpeg_encode_optimize_host(J._ptr(img), H, W, MODE[mode], quality, rows, 1, J._ptr(out), out.size, C.byref(n)) == 0
    return coef, counts, out[:n.value].tobytes()


# ---- synthetic counts ------------------------------------------------------------------------------------------------------------------
def _table(kind):
    c = np.zeros(256, np.uint32)
    if kind == "fibonacci":                                  # 40 symbols (with the ties of 1, 1 and the reserved 1, 30 reach 16 bits only)
        a, b = 1, 1
        for i in range(40):
            c[(37 * i + 5) % 256] = a
            a, b = b, a + b
    elif kind == "equal":                                    # every tie rule
        c[:] = 7
    elif kind == "one":
        c[200] = 9
    elif kind == "two":
        c[3], c[130] = 4, 1
    elif kind == "apart":                                    # ties inside one lane's registers (64 apart) and across lanes
        c[[3, 67, 131, 195, 4, 68, 250]] = 5
        c[[9, 73]] = 10
        c[17] = 2
    return c


# name -> (mode, the four tables' kinds); a grey frame builds the first two only
COUNT_CASES = {
    "fold_ties": ("444", ("fibonacci", "equal", "one", "two")),
    "lanes": ("420", ("two", "apart", "apart", "fibonacci")),
    "grey": ("grey", ("apart", "fibonacci", "equal", "equal")),
    "no_room": ("444", ("equal", "equal", "equal", "equal")),      # 4 x 277 bytes of DHT do not fit the struct's header: left out
}


def counts_of(name):
    return np.stack([_table(k) for k in COUNT_CASES[name][1]])


def gen_optimal_table(counts):
    """jchuff.c's jpeg_gen_optimal_table -> (bits[1..16], huffval, the deepest length before the fold)"""
    freq, codesize, others = [int(v) for v in counts] + [1], [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    deepest = max(codesize)
    bits = [0] * (max(deepest, 32) + 1)
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(len(bits) - 1, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    return bits[1:17], [j for i in range(1, deepest + 1) for j in range(256) if codesize[j] == i], deepest


def standard_tables(mode, H=16, W=16):
    lib = J.lib()
    t = np.zeros(lib.rhccq_jpeg_write_tables_bytes(), np.uint8)
    assert lib.rhccq_jpeg_write_tables_host(H, W, MODE[mode], 75, 0, J._ptr(t)) == 0
    return t


def host_tables(name):
    mode = COUNT_CASES[name][0]
    std, out, counts = standard_tables(mode), np.full(J.lib().rhccq_jpeg_write_tables_bytes(), 0xAA, np.uint8), counts_of(name)
    assert J.lib().rhccq_jpeg_huffman_host(J._ptr(counts), 16, 16, MODE[mode], 0, J._ptr(std), J._ptr(out)) == 0
    return out


def check_tables(name, made):
    """a table struct (uint8: div uint16[3][64], code uint16[4][256], len uint8[4][256], header_len, pad, header[640]) against
    gen_optimal_table of the case's counts -> the deepest length before the fold over its tables"""
    mode = COUNT_CASES[name][0]
    std, counts, n_tables = standard_tables(mode), counts_of(name), 2 if mode == "grey" else 4
    code, length = made[384:2432].view(np.uint16).reshape(4, 256), made[2432:3456].reshape(4, 256)
    header_len, header = int(made[3456:3460].view(np.int32)[0]), made[3464:].tobytes()
    assert np.array_equal(made[:384], std[:384]) and not made[3460:3464].any()
    std_len, std_header = int(std[3456:3460].view(np.int32)[0]), std[3464:].tobytes()
    dht, tail, want, deepest = std_header.index(b"\xff\xc4"), std_header.index(b"\xff\xda"), b"", 0
    for t in range(4):
        bits, vals, deep = gen_optimal_table(counts[t]) if t < n_tables else ([0] * 16, [], 0)
        deepest = max(deepest, deep)
        c, at, codes, lens = 0, 0, np.zeros(256, np.uint16), np.zeros(256, np.uint8)
        for l in range(1, 17):
            for _ in range(bits[l - 1]):
                codes[vals[at]], lens[vals[at]] = c, l
                c, at = c + 1, at + 1
            c <<= 1
        assert at == len(vals) and np.array_equal(code[t], codes) and np.array_equal(length[t], lens), (name, t)
        if t < n_tables:
            want += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([(t & 1) << 4 | t >> 1] + bits + vals)
    want = std_header[:dht] + want + std_header[tail:std_len]
    if len(want) > 640:
        assert header_len == 0 and not any(header), name
    else:
        assert header_len == len(want) and header[:header_len] == want and not any(header[header_len:]), name
    return deepest
