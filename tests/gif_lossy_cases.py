"""Shared cases of the lossy GIF tests (tests/test_gif_lossy_cpu.py, tests/test_gpu_gif_lossy.py): a plain helper module, not a conftest.

`lossy_segment` is the dict statement of the lossy step of include/rhccq.h ("GIF files written on the device", paragraph "lossy"), written
from that text; packing, framing and decoding are those of tests/gif_cases.py.  Every reference is computed once per process and shared."""
import ctypes as C
import functools

import numpy as np

import gif_cases as G

S, MAX_SLACK = G.S, 3 * 255 * 255


def dist(pal):
    p = np.asarray(pal, np.int64)
    return ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)


def lossy_segment(px, m, opening, last, D, K, slack):
    """one segment -> ([(code, width)], the written pixels, {"table_full": Clears for a full table, "ties": steps two candidates tied in})"""
    clear, end = 1 << m, (1 << m) + 1
    codes = [(clear, m + 1)] if opening else []
    table, nxt, width = {}, clear + 2, m + 1
    info = {"table_full": 0, "ties": 0}
    cur = int(px[0])
    written = [cur]
    for p in px[1:]:
        p = int(p)
        hit = table.get((cur, p))
        w = p
        if hit is None and p < K:                                      # (p == K is the transparent index: never substituted)
            cands = sorted((D[p][q], q) for q in range(K) if q != p and D[p][q] <= slack and (cur, q) in table)
            if cands:
                w = cands[0][1]
                hit = table[(cur, w)]
                info["ties"] += len(cands) > 1 and cands[1][0] == cands[0][0]
        written.append(w)
        if hit is not None:
            cur = hit
            continue
        codes.append((cur, width))
        if nxt < 4096:
            table[(cur, p)] = nxt
        if nxt == 1 << width and width < 12:
            width += 1
        nxt += 1
        cur = p
        if nxt == 4096:
            codes.append((clear, width))
            table, nxt, width = {}, clear + 2, m + 1
            info["table_full"] += 1
    codes.append((cur, width))
    if nxt == 1 << width and width < 12:
        width += 1
    codes.append((end if last else clear, width))
    return codes, written, info


def splice(file, streams):
    """the lossless reference's file with every frame's code stream replaced"""
    parsed = G.parse(file)
    p = 13 + 3 * parsed["global"] + (19 if parsed["loop"] is not None else 0)
    out = file[:p]
    for fr, st in zip(parsed["frames"], streams):
        head, L = 18 + 3 * fr["local"] + 1, len(fr["stream"])
        out += file[p:p + head] + b"".join(bytes([len(st[o:o + 255])]) + st[o:o + 255] for o in range(0, len(st), 255)) + b"\x00"
        p += head + L + (L + 254) // 255 + 1
    return out + b"\x3b"


# ---- the cases: gif_cases' dict with "slack" ---------------------------------------------------------------------------------------------
def _near(K, seed, step=6):
    """K distinct rows a short way from each other: a random walk from mid grey"""
    rng = np.random.default_rng(3000 + seed)
    while True:
        pal = np.clip(128 + np.cumsum(rng.integers(-step, step + 1, (K, 3)), 0), 0, 255).astype(np.uint8)
        if len(np.unique(pal, axis=0)) == K:
            return pal[rng.permutation(K)]


def _noise(n, K, seed):
    """a slow ramp with noise on it: neighbours in the walk follow each other, so strings repeat and near rows are in reach"""
    rng = np.random.default_rng(seed)
    return (np.arange(n) * K // max(n, 1) // 4 * 4 + rng.integers(0, min(K, 6), n)) % K


def _case(frames, palettes, slack, delta=False):
    v = G._case(frames, palettes, delta=delta)
    v["frames"].setflags(write=False)
    return dict(v, slack=slack)


@functools.lru_cache(maxsize=None)
def _cases():
    c = {}
    rng = np.random.default_rng(5)
    c["k2"] = _case(rng.integers(0, 2, (30, 50)), np.array([[0, 0, 0], [3, 3, 3]], np.uint8), 27)
    c["k64"] = _case(_noise(3000, 64, 1).reshape(40, 75), _near(64, 1), 128)
    c["k256_slots"] = _case(rng.integers(0, 256, (64, 64)), _near(256, 2, 3)[np.argsort(rng.random(256))], 300)
    line = np.zeros((16, 3), np.uint8)
    line[:, 0] = 16 * np.arange(16)                                       # a row's two neighbours are equally far: 256
    c["ties"] = _case(rng.integers(0, 16, (40, 50)), line, 256)
    c["duplicate_rows"] = _case(rng.integers(0, 12, (40, 50)), np.repeat(_near(6, 3, 40), 2, 0), 0)
    c["slack_max"] = _case(rng.integers(0, 256, (25, 41)), G._palette(256, 6), MAX_SLACK)
    c["slack0"] = _case(_noise(3000, 256, 4).reshape(40, 75), _near(256, 4), 0)
    for n in (1, 63, 64, 65, 1023, 1024, 1025, S, S + 1, 2 * S + 1):
        c[f"px{n}"] = _case(_noise(n, 16, n).reshape(1, n), _near(16, 5), 128)
    c["table_full"] = _case(G._noise(S, 256, 7).reshape(128, 128), G._palette(256, 7), 48)
    a = _noise(37 * 53, 255, 8).reshape(37, 53)
    b = np.where(rng.random((37, 53)) < 0.6, a, (a + 3) % 255)
    c["delta"] = _case(np.stack([a, b, np.where(rng.random((37, 53)) < 0.6, b, a)]), _near(255, 6), 200, delta=True)
    rows = (5, 200, 64)
    c["local"] = _case(np.stack([_noise(37 * 53, k, 9 + k).reshape(37, 53) for k in rows]), [_near(k, k) for k in rows], 150)
    c["clamp"] = _case(rng.integers(0, 300, (37, 53)), _near(100, 7), 100)
    return c


def names():
    return list(_cases())


def case(name):
    return _cases()[name]


def pals_of(name):
    v = case(name)
    return v["palettes"] if isinstance(v["palettes"], list) else [v["palettes"]] * len(v["frames"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (file bytes, [stream bytes per frame], written uint8[n, H, W], [info per segment])"""
    v = case(name)
    streams, written, infos = [], [], []
    for f, pal in enumerate(pals_of(name)):
        K = len(pal)
        m = G.min_code(K + (1 if v["delta"] else 0))
        px = G.written_pixels(v["frames"], K, v["delta"])[f].reshape(-1)
        D = dist(pal).tolist()
        codes, wr = [], []
        for p0 in range(0, len(px), S):
            cd, w, info = lossy_segment(px[p0:p0 + S].tolist(), m, p0 == 0, p0 + S >= len(px), D, K, v["slack"])
            codes += cd
            wr += w
            infos.append(info)
        streams.append(G.pack(codes))
        written.append(np.array(wr, np.uint8).reshape(v["frames"].shape[1:]))
    lossless = G.gif_reference(v["frames"], v["palettes"], v["delays"], v["loop"], v["delta"])[0]
    return splice(lossless, streams), streams, np.stack(written), infos


def check(name, data, written):
    """the four properties of a lossy file: the reference's bytes and written pixels, Pillow's picture, the bound"""
    v = case(name)
    want, _, wr, _ = reference(name)
    assert bytes(data) == want, (name, len(data), len(want))
    assert np.array_equal(np.asarray(written).reshape(wr.shape), wr), name
    shown, asked, pillow = [], [], G.pillow_frames(data)[0]
    for f, pal in enumerate(pals_of(name)):
        K = len(pal)
        cur = wr[f].astype(np.int64)
        shown.append(np.where(cur == K, shown[-1], cur) if v["delta"] and f else cur)      # (T resolved frame by frame)
        asked.append(G.clamped(v["frames"][f], K))
        assert (dist(pal)[asked[f], shown[f]] <= v["slack"]).all(), (name, f)
        assert np.array_equal(pillow[f], np.asarray(pal, np.uint8)[shown[f]]), (name, f)
    if v["slack"] == 0 and all(len(np.unique(p, axis=0)) == len(p) for p in pals_of(name)):
        assert want == G.gif_reference(v["frames"], v["palettes"], v["delays"], v["loop"], v["delta"])[0], name


def _check_preconditions():
    moved = {n: reference(n)[2] != G.written_pixels(case(n)["frames"], len(pals_of(n)[0]), case(n)["delta"]) for n in ("k2", "k64", "k256_slots", "delta")}
    assert all(m.any() for m in moved.values())
    assert set((reference("k256_slots")[2][moved["k256_slots"]] >> 6).tolist()) == {0, 1, 2, 3}       # a winner in each register slot
    assert sum(i["ties"] for i in reference("ties")[3]) > 10
    assert (reference("duplicate_rows")[2] != case("duplicate_rows")["frames"]).any() and reference("table_full")[3][0]["table_full"] >= 1
    wr = reference("delta")[2]
    assert (wr[1:] == 255).any() and (wr[1:] != 255).any() and (reference(f"px{S + 1}")[2].reshape(-1)[S] == case(f"px{S + 1}")["frames"].reshape(-1)[S])
    assert (case("clamp")["frames"] >= 100).any()


_check_preconditions()


# ---- the host forms through ctypes -------------------------------------------------------------------------------------------------------
def block(name):
    """-> (palettes as the entries take them, k_stride, int32 k_rows, flags)"""
    v = case(name)
    flags = (G.LOCAL if isinstance(v["palettes"], list) else 0) | (G.DELTA if v["delta"] else 0)
    if not flags & G.LOCAL:
        return np.ascontiguousarray(v["palettes"], np.uint8), len(v["palettes"]), np.array([len(v["palettes"])], np.int32), flags
    stride = max(len(p) for p in v["palettes"])
    blk = np.full((len(v["palettes"]), stride, 3), 0xEE, np.uint8)
    for f, p in enumerate(v["palettes"]):
        blk[f, :len(p)] = p
    return blk, stride, np.array([len(p) for p in v["palettes"]], np.int32), flags


def host(name, eb=4, shift=0, slack=None, flags_or=0):
    """rhccq_gif_encode_lossy_host and rhccq_gif_lzw_lossy_host -> (rc of each, file bytes, [stream bytes], written of each)"""
    v = case(name)
    n, H, W = v["frames"].shape
    pal, stride, rows, flags = block(name)
    flags |= flags_or
    slack = v["slack"] if slack is None else slack
    _, _, sbound, bound = G.sizes(n, H, W, flags & 3)
    arr = G.shifted(G.index_array(v["frames"], eb), shift)
    out, length, lens = np.full(bound, 0xA5, np.uint8), C.c_int64(0), np.zeros(n, np.int64)
    wr1, wr2 = np.full((n, H, W), 0xA5, np.uint8), np.full((n, H, W), 0xA5, np.uint8)
    rc1 = G.lib().rhccq_gif_encode_lossy_host(G._ptr(arr), eb, n, H, W, G._ptr(pal), stride, G._ptr(rows), G._ptr(np.array(v["delays"], np.int32)), v["loop"],
                                              flags, slack, G._ptr(out), bound, C.byref(length), G._ptr(lens), G._ptr(wr1))
    streams = np.full((n, sbound), 0xA5, np.uint8)
    rc2 = G.lib().rhccq_gif_lzw_lossy_host(G._ptr(arr), eb, n, H, W, G._ptr(pal), stride, G._ptr(rows), flags, slack, G._ptr(streams), sbound, G._ptr(lens),
                                           G._ptr(wr2))
    return (rc1, rc2), out[:length.value].tobytes(), [streams[f, :max(lens[f], 0)].tobytes() for f in range(n)], (wr1, wr2)
