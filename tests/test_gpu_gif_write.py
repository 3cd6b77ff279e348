"""GIF files written on the device (csrc/gif_write.hip: Rhccq.gif_lzw / gif_encode, container.write_gif, the gif_path keyword of
ImageEncoder.quantize / encode_with_palette / encode / quantize_batch, ImageEncoder.animate, the command line) against the dict / struct
reference of tests/gif_cases.py, byte for byte, and against Pillow.  GPU only."""
import json
import os

import numpy as np
import pytest

import gif_cases as GC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_NDT = {1: np.uint8, 2: np.int16, 4: np.int32}


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


@pytest.fixture(scope="module")
def enc(rh):
    from roibasedimagecompression_amd.image import ImageEncoder
    return ImageEncoder(rh)


@pytest.fixture(scope="module")
def crop():
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "kodak_1.png")).convert("RGB"))[100:164, 200:296])


def _dev_idx(rh, frames, eb, shift=0):
    """the frames in the storage of width eb on the device, `shift` bytes (a multiple of eb) behind a 256-byte boundary"""
    import torch
    raw = GC.index_array(frames, eb).view(np.uint8).reshape(-1)
    buf = torch.zeros((len(raw) + 64,), dtype=torch.uint8, device=rh.device)
    buf[shift:shift + len(raw)] = rh.dev(raw)
    return buf, buf[shift:shift + len(raw)]


def _shifts(eb, k):
    return ((0, 1, 2, 3, 5, 15) if eb == 1 else (0, 2, 6) if eb == 2 else (0, 4, 12)) if k == 0 else (0,)


def _raw_lzw(rh, name, eb, shift, trie=False):
    import torch
    v = GC.case(name)
    n, H, W = v["frames"].shape
    flags = GC.flags_of(name) | (GC.TRIE if trie else 0)
    rc, ws, stride, _ = GC.sizes(n, H, W, flags)
    assert rc == 0
    work = torch.full((ws,), 0xC3, dtype=torch.uint8, device=rh.device)
    out = torch.full((n, stride + 16), 0xA5, dtype=torch.uint8, device=rh.device)
    lens = torch.full((n,), -1, dtype=torch.int64, device=rh.device)
    keep, idx = _dev_idx(rh, v["frames"], eb, shift)
    rows = np.array(GC.rows_of(name), np.int32)
    rc = rh.lib.rhccq_gif_lzw(rh.ctx, rh._p(idx), eb, n, H, W, GC._ptr(rows), flags, rh._p(work), rh._p(out), stride + 16, rh._p(lens))
    host, lens = out.cpu().numpy(), lens.cpu().numpy()
    assert all((host[f, max(lens[f], 0):] == 0xA5).all() for f in range(n)), "bytes behind a stream were written"
    return rc, [host[f, :lens[f]].tobytes() for f in range(n)]


def _raw_encode(rh, name, eb, shift, trie=False):
    import torch
    v = GC.case(name)
    n, H, W = v["frames"].shape
    flags = GC.flags_of(name) | (GC.TRIE if trie else 0)
    rc, ws, _, bound = GC.sizes(n, H, W, flags)
    assert rc == 0
    work = torch.full((ws,), 0xC3, dtype=torch.uint8, device=rh.device)
    out = torch.full((bound + 16,), 0xA5, dtype=torch.uint8, device=rh.device)
    length = torch.full((1,), -1, dtype=torch.int64, device=rh.device)
    keep, idx = _dev_idx(rh, v["frames"], eb, shift)
    pal, stride, rows = GC.palette_block(name)
    delays = np.array(v["delays"], np.int32)
    rc = rh.lib.rhccq_gif_encode(rh.ctx, rh._p(idx), eb, n, H, W, rh._p(rh.dev(pal)), stride, GC._ptr(rows), GC._ptr(delays), v["loop"], flags, rh._p(work),
                                 rh._p(out), bound, rh._p(length))
    host, length = out.cpu().numpy(), int(length.cpu()[0])
    assert (host[max(length, 0):] == 0xA5).all(), "bytes behind the file were written"
    return rc, host[:max(length, 0)].tobytes(), work[:8 * n].view(torch.int64).cpu().tolist()


@pytest.mark.parametrize("name", GC.names())
def test_device_streams_equal_reference(rh, name):
    want = GC.reference_streams(name)
    for k, eb in enumerate(GC.widths(name)):
        for shift in _shifts(eb, k):
            rc, streams = _raw_lzw(rh, name, eb, shift)
            assert rc == 0, (name, eb, shift)
            assert streams == want, (name, eb, shift, [len(s) for s in streams], [len(s) for s in want])
        for shift in _shifts(eb, k)[-1:] + (0,):                              # the trie dictionary: the same streams
            rc, streams = _raw_lzw(rh, name, eb, shift, trie=True)
            assert rc == 0 and streams == want, (name, eb, shift, "trie")


@pytest.mark.parametrize("name", GC.names())
def test_device_file_equals_reference(rh, name):
    want, lengths = GC.reference(name)
    for k, eb in enumerate(GC.widths(name)):
        for shift in _shifts(eb, k)[:3]:
            rc, data, lens = _raw_encode(rh, name, eb, shift)
            assert rc == 0, (name, eb, shift)
            assert lens == lengths, (name, eb, shift)
            assert data == want, (name, eb, shift, len(data), len(want))
        rc, data, lens = _raw_encode(rh, name, eb, eb, trie=True)
        assert rc == 0 and lens == lengths and data == want, (name, eb, "trie")


@pytest.mark.parametrize("name", ["k5", "delta_five", "local_mixed", "clamp_wide"])
def test_wrappers_equal_reference(rh, name):
    v = GC.case(name)
    n, H, W = v["frames"].shape
    local = isinstance(v["palettes"], list)
    pal, stride, rows = GC.palette_block(name)
    assert rh.gif_encode(v["frames"], n, H, W, pal, rows.tolist() if local else None, v["delays"], v["loop"], v["delta"]) == GC.reference(name)[0]
    streams, lens = rh.gif_lzw(v["frames"], n, H, W, rows.tolist(), local, v["delta"])
    assert streams.is_cuda and lens.is_cuda and str(lens.dtype) == "torch.int64"
    host, lens = streams.cpu().numpy(), lens.cpu().tolist()
    assert [host[f, :lens[f]].tobytes() for f in range(n)] == GC.reference_streams(name)
    out, length, lens = rh.gif_encode_async(v["frames"], n, H, W, pal, rows.tolist() if local else None, v["delays"], v["loop"], v["delta"])
    assert out.is_cuda and length.is_cuda and lens.cpu().tolist() == GC.reference(name)[1]


def test_device_entries_refuse_bad_arguments_before_any_launch(rh):
    """every refusal that only rhccq_gif_lzw and rhccq_gif_encode make (the host forms cannot reach them): E_ARG or E_LIMIT, and neither
    the output nor the workspace is touched"""
    import torch
    n, H, W = 2, 5, 7
    rc, ws, stream, bound = GC.sizes(n, H, W, 0)
    assert rc == 0
    idx = torch.zeros((n * H * W,), dtype=torch.uint8, device=rh.device)
    pal = torch.zeros((8, 3), dtype=torch.uint8, device=rh.device)
    work = torch.full((ws + 256,), 0xC3, dtype=torch.uint8, device=rh.device)
    out = torch.full((bound + 64,), 0xA5, dtype=torch.uint8, device=rh.device)
    streams = torch.full((n * (stream + 8) + 64,), 0xA5, dtype=torch.uint8, device=rh.device)
    words = torch.full((8,), -7, dtype=torch.int64, device=rh.device)                    # out_len / stream_bytes
    rows, rows_local, delays = np.array([5], np.int32), np.array([5, 9], np.int32), np.array([1, 2], np.int32)
    null = None

    def p(t, off=0):
        return rh._p(t[off:]) if t is not None else rh._p(None)

    def lzw(i=idx, eb=1, n=n, H=H, W=W, k=rows, flags=0, w=work, woff=0, o=streams, stride=stream + 8, ln=words, lnoff=0):
        return rh.lib.rhccq_gif_lzw(rh.ctx, p(i), eb, n, H, W, GC._ptr(k), flags, p(w, woff), p(o), stride, p(ln.view(torch.uint8) if ln is not None else None, lnoff))

    def encode(i=idx, eb=1, n=n, H=H, W=W, pl=pal, ks=8, k=rows, d=delays, loop=0, flags=0, w=work, woff=0, o=out, cap=bound, ln=words, lnoff=0):
        return rh.lib.rhccq_gif_encode(rh.ctx, p(i), eb, n, H, W, p(pl), ks, GC._ptr(k), GC._ptr(d), loop, flags, p(w, woff), p(o), cap,
                                       p(ln.view(torch.uint8) if ln is not None else None, lnoff))

    for call in (lzw, encode):
        assert call(w=null) == GC.E_ARG and call(o=null) == GC.E_ARG and call(ln=null) == GC.E_ARG and call(i=null) == GC.E_ARG and call(k=None) == GC.E_ARG
        assert call(woff=1) == GC.E_ARG and call(woff=128) == GC.E_ARG                  # the workspace is aligned to 256
        assert call(lnoff=4) == GC.E_ARG and call(lnoff=1) == GC.E_ARG                  # out_len / stream_bytes to 8
        assert call(n=0) == GC.E_ARG and call(H=0) == GC.E_ARG and call(W=65536) == GC.E_ARG and call(eb=3) == GC.E_ARG and call(eb=2, i=idx[1:]) == GC.E_ARG
        assert call(flags=8) == GC.E_ARG and call(flags=GC.LOCAL | GC.DELTA) == GC.E_ARG and call(k=np.array([0], np.int32)) == GC.E_ARG
        assert call(k=np.array([256], np.int32), flags=GC.DELTA) == GC.E_ARG and call(k=np.array([5, 257], np.int32), flags=GC.LOCAL) == GC.E_ARG
    assert lzw(stride=stream - 1) == GC.E_LIMIT and lzw(stride=0) == GC.E_LIMIT
    assert encode(cap=bound - 1) == GC.E_LIMIT and encode(cap=0) == GC.E_LIMIT           # as rhccq_png_encode reports it
    assert encode(pl=null) == GC.E_ARG and encode(ks=0) == GC.E_ARG and encode(ks=257) == GC.E_ARG and encode(ks=4) == GC.E_ARG
    assert encode(k=rows_local, flags=GC.LOCAL) == GC.E_ARG                              # 9 rows in a block of k_stride = 8
    assert encode(d=None) == GC.E_ARG and encode(d=np.array([1, 65536], np.int32)) == GC.E_ARG and encode(d=np.array([-1, 0], np.int32)) == GC.E_ARG
    assert encode(loop=-1) == GC.E_ARG and encode(loop=65536) == GC.E_ARG
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((streams == 0xA5).all()) and bool((work == 0xC3).all()) and bool((words == -7).all()), "a refused call wrote"
    # the same arguments, valid: both run, and write
    assert lzw() == 0 and encode() == 0 and encode(k=np.array([5, 8], np.int32), flags=GC.LOCAL, pl=torch.zeros((2, 8, 3), dtype=torch.uint8, device=rh.device)) == 0
    assert lzw(flags=GC.TRIE) == 0 and encode(flags=GC.TRIE | GC.DELTA) == 0
    torch.cuda.synchronize()
    assert int(words[0]) > 0 and not bool((out == 0xA5).all())


def test_wrapper_argument_errors(rh):
    idx, pal = np.zeros((2, 2, 3), np.uint8), np.zeros((4, 3), np.uint8)
    for bad, text in ((lambda: rh.gif_encode(idx, 2, 2, 4, pal), "gif_encode: indices must have H * W elements"),
                      (lambda: rh.gif_encode(idx, 2, 2, 3, np.zeros((4, 4), np.uint8)), "gif_encode: palettes [K, 3] or [n, K, 3] are expected"),
                      (lambda: rh.gif_encode(idx, 2, 2, 3, np.zeros((257, 3), np.uint8)), "gif_encode: a table must have 1..256 rows, all of them in palettes"),
                      (lambda: rh.gif_encode(idx, 2, 2, 3, np.zeros((256, 3), np.uint8), delta=True),
                       "gif_encode: delta needs a table of at most 255 rows (the transparent index is one more entry)"),
                      (lambda: rh.gif_encode(idx, 2, 2, 3, np.zeros((2, 4, 3), np.uint8), delta=True), "gif_encode: delta needs a global table"),
                      (lambda: rh.gif_encode(idx, 2, 2, 3, pal, delays=[1, 2, 3]),
                       "gif_encode: delays must be one number or one a frame, each 0..65535 centiseconds"),
                      (lambda: rh.gif_encode(idx, 2, 2, 3, pal, delays=65536), "gif_encode: delays must be one number or one a frame, each 0..65535 centiseconds"),
                      (lambda: rh.gif_encode(idx, 2, 2, 3, pal, loop=-1), "gif_encode: loop must be 0..65535"),
                      (lambda: rh.gif_lzw(idx, 2, 2, 3, [0]), "gif_lzw: a table must have 1..256 rows"),
                      (lambda: rh.gif_lzw(idx, 2, 2, 3, [4, 4, 4], local=True), "gif_lzw: one row count per table is expected"),
                      (lambda: rh.gif_lzw(np.zeros(0, np.uint8), 0, 2, 3, [4]), "gif_lzw: at least one frame is expected"),
                      (lambda: rh.gif_lzw(idx, 2, 2, 3, [4], dictionary="tree"), 'gif: dictionary must be "hash" or "trie"')):
        with pytest.raises(ValueError) as e:
            bad()
        assert str(e.value) == text


# ---- the container layer, the encoder's keyword, the animation and the command line ----------------------------------------------------------
def _indices(res):
    idx = res["indices"].cpu().numpy()
    return (idx.view(np.uint16) if idx.dtype == np.int16 else idx).astype(np.int64)


def _host_file(frames, palettes, delays, loop=0, delta=False):
    """the host form's file of returned indices (frames int[n, H, W]; palettes one array or a list)"""
    import ctypes as C
    frames = np.ascontiguousarray(frames, np.uint32)
    n, H, W = frames.shape
    local = isinstance(palettes, list)
    flags = (GC.LOCAL if local else 0) | (GC.DELTA if delta else 0)
    rows = np.array([len(p) for p in palettes] if local else [len(palettes)], np.int32)
    stride = int(rows.max())
    block = np.zeros((len(rows), stride, 3), np.uint8)
    for f, p in enumerate(palettes if local else [palettes]):
        block[f, :len(p)] = p
    rc, _, _, bound = GC.sizes(n, H, W, flags)
    out, length = np.zeros(bound, np.uint8), C.c_int64()
    rc = GC.lib().rhccq_gif_encode_host(GC._ptr(frames), 4, n, H, W, GC._ptr(block), stride, GC._ptr(rows), GC._ptr(np.array(delays, np.int32)), loop, flags,
                                        GC._ptr(out), bound, C.byref(length), None)
    assert rc == 0
    return out[:length.value].tobytes()


@pytest.mark.parametrize("colours", [2, 16, 256])
def test_write_gif_of_quantize_results(rh, enc, crop, tmp_path, colours):
    from roibasedimagecompression_amd import container
    res = enc.quantize(crop, colours=colours)
    fn = str(tmp_path / "q.gif")
    size = container.write_gif(res, fn, rh)
    data = open(fn, "rb").read()
    idx = _indices(res).reshape((1,) + tuple(res["shape"]))
    pal = np.asarray(res["palette"], np.uint8)
    assert size == len(data) and data == _host_file(idx, pal, [4]) == GC.gif_reference(idx, pal, [4])[0]
    frames, durations, loop = GC.pillow_frames(data)
    assert np.array_equal(frames, GC.decoded(idx, pal)) and durations == [40] and loop is None
    # the same picture three times with another: a global table, delta, per-frame delays
    other = enc.encode_with_palette(crop[::-1].copy(), pal)
    seq = [res, res, other, res]
    data, row = container.gif_file(seq, rh, delay=[1, 2, 3, 4], loop=7, delta=colours < 256)
    all_idx = np.stack([_indices(r).reshape(res["shape"]) for r in seq])
    assert data == _host_file(all_idx, pal, [1, 2, 3, 4], 7, colours < 256)
    assert row == {"bytes": len(data), "frames": 4, "table": "global", "colours": len(pal), "delta": colours < 256,
                   "stream_bytes": [len(f["stream"]) for f in GC.parse(data)["frames"]]}
    frames, durations, loop = GC.pillow_frames(data)
    assert np.array_equal(frames, GC.decoded(all_idx, pal)) and durations == [10, 20, 30, 40] and loop == 7
    if colours < 256:
        with pytest.raises(ValueError):
            container.gif_bytes([res, enc.quantize(255 - crop, colours=colours)], rh, delta=True)             # two palettes: local tables
    else:
        with pytest.raises(ValueError):
            container.gif_bytes(seq, rh, delta=True)


def test_write_gif_with_local_tables(rh, enc, crop):
    from roibasedimagecompression_amd import container
    seq = [enc.quantize(crop, colours=k) for k in (5, 200, 16)]
    data, row = container.gif_file(seq, rh, delay=9)
    idx = np.stack([_indices(r).reshape(r["shape"]) for r in seq])
    pals = [np.asarray(r["palette"], np.uint8) for r in seq]
    assert data == _host_file(idx, pals, [9, 9, 9]) and row["table"] == "local" and row["colours"] == max(len(p) for p in pals)
    frames, durations, loop = GC.pillow_frames(data)
    assert np.array_equal(frames, GC.decoded(idx, pals)) and durations == [90, 90, 90] and loop == 0
    with pytest.raises(ValueError):
        container.gif_bytes([seq[0], enc.quantize(crop[:32], colours=5)], rh)


def test_gif_path_fills_stats_and_changes_nothing_else(rh, enc, crop, tmp_path):
    import torch
    pal = enc.quantize(crop, colours=12)["palette"]
    calls = {"quantize": lambda **kw: enc.quantize(crop, colours=12, **kw),
             "encode_with_palette": lambda **kw: enc.encode_with_palette(crop, pal, **kw),
             "encode": lambda **kw: enc.encode(crop, 2, 1, max_colours=200, **kw)}
    for name, call in calls.items():
        fn = str(tmp_path / f"{name}.gif")
        plain = call()
        res = call(gif_path=fn)
        assert "gif" not in plain["stats"]
        assert np.array_equal(plain["palette"], res["palette"]) and torch.equal(plain["indices"], res["indices"]), name
        assert set(res["stats"]) - {"gif"} == set(plain["stats"]), name
        data = open(fn, "rb").read()
        idx = _indices(res).reshape((1,) + tuple(res["shape"]))
        p = np.asarray(res["palette"], np.uint8)
        assert data == _host_file(idx, p, [4]), name
        row = res["stats"]["gif"]
        assert row["bytes"] == len(data) and row["frames"] == 1 and row["table"] == "global" and row["colours"] == len(p) and not row["delta"]
        assert np.array_equal(GC.pillow_frames(data)[0], GC.decoded(idx, p))
    with pytest.raises(ValueError):
        enc.encode_with_palette(crop, np.random.default_rng(3).integers(0, 256, (300, 3)).astype(np.uint8), gif_path=str(tmp_path / "big.gif"))


def test_quantize_batch_writes_one_file(rh, enc, crop, tmp_path):
    fn = str(tmp_path / "b.gif")
    images = [crop, 255 - crop, crop // 2]                                    # (three pictures, three palettes)
    plain = enc.quantize_batch(images, colours=16)
    res = enc.quantize_batch(images, colours=16, gif_path=fn, delay=[5, 6, 7])
    data = open(fn, "rb").read()
    idx = np.stack([_indices(r).reshape(r["shape"]) for r in res])
    pals = [np.asarray(r["palette"], np.uint8) for r in res]
    assert all(np.array_equal(a["palette"], b["palette"]) and np.array_equal(_indices(a), _indices(b)) for a, b in zip(plain, res))
    assert data == _host_file(idx, pals, [5, 6, 7])
    frames, durations, _ = GC.pillow_frames(data)
    assert np.array_equal(frames, GC.decoded(idx, pals)) and durations == [50, 60, 70]
    assert res[0]["stats"]["gif"]["table"] == "local" and res[0]["stats"]["gif"]["frames"] == 3
    with pytest.raises(ValueError):
        enc.quantize_batch([crop, crop[:32]], colours=16, gif_path=fn)


@pytest.mark.parametrize("pattern", [None, 160])
def test_animate(rh, enc, crop, tmp_path, pattern):
    fn = str(tmp_path / "a.gif")
    images = [crop, crop, crop, np.roll(crop, 7, axis=1), crop[::-1].copy()]
    res = enc.animate(images, colours=32, gif_path=fn, delay=[1, 2, 3, 4, 5], loop=2, pattern=pattern)
    pal = np.asarray(res["palette"], np.uint8)
    assert res["indices"].is_cuda and tuple(res["indices"].shape) == (5,) + crop.shape[:2] and len(pal) <= 32
    idx = _indices(res)
    data = open(fn, "rb").read()
    assert data == _host_file(idx, pal, [1, 2, 3, 4, 5], 2, True)
    row = res["stats"]["gif"]
    assert row["bytes"] == len(data) and row["delta"] and row["colours"] == len(pal) and row["frames"] == 5 and row["table"] == "global"
    parsed = GC.parse(data)
    assert parsed["loop"] == 2 and [f["transparent"] for f in parsed["frames"]] == [None] + [len(pal)] * 4
    frames, durations, loop = GC.pillow_frames(data)
    assert np.array_equal(frames, GC.decoded(idx, pal)) and durations == [10, 20, 30, 40, 50] and loop == 2
    # a frame repeated three times: frames 1 and 2 are all transparent, so their streams are those of a flat frame of T
    flat = GC.lzw_reference(np.full(crop.shape[0] * crop.shape[1], len(pal)), GC.min_code(len(pal) + 1))[0]
    assert parsed["frames"][1]["stream"] == parsed["frames"][2]["stream"] == flat
    kw = {"pattern": pattern} if pattern else {}
    for f, img in enumerate(images):
        one = enc.encode_with_palette(img, pal, **kw)
        assert np.array_equal(_indices(one).reshape(crop.shape[:2]), idx[f]), f
    assert len(res["stats"]["pattern" if pattern else "remap"]) == 5
    full = enc.animate(images[:2], colours=256, delta=False)
    assert len(full["palette"]) <= 256 and not full["stats"]["gif"]["delta"] and full["stats"]["gif"]["bytes"] > 0
    assert set(full) == {"palette", "indices", "indices_dtype", "shape", "stats"}
    assert full["stats"]["build"]["asked"] == 256 and enc.animate(images[:2], colours=256)["stats"]["build"]["asked"] == 255     # T takes an entry


def test_animate_refuses(rh, enc, crop):
    for bad, text in ((lambda: enc.animate([crop, crop[:32]], 16), "ImageEncoder.animate: every frame must have the same shape"),
                      (lambda: enc.animate(np.zeros((2, 4, 4, 3), np.int32), 16), "ImageEncoder.animate: a uint8 B x H x W x 3 tensor is expected"),
                      (lambda: enc.animate(np.zeros((2, 4, 4, 4), np.uint8), 16), "ImageEncoder.animate: a uint8 B x H x W x 3 tensor is expected"),
                      (lambda: enc.animate([crop, crop], 16, roi_masks=[None]), "ImageEncoder.animate: at least one frame, and one mask (or None) per frame, are expected"),
                      (lambda: enc.animate([], 16), "ImageEncoder.animate: at least one frame, and one mask (or None) per frame, are expected"),
                      (lambda: enc.animate([crop], 16, roi_weight=3), "ImageEncoder.animate: roi_weight (1..255) other than 1 needs roi_masks"),
                      (lambda: enc.animate([crop[..., 0]], 16), "ImageEncoder.animate: a uint8 H x W x 3 image is expected")):
        with pytest.raises(ValueError) as e:
            bad()
        assert str(e.value) == text


def test_command_line(rh, enc, crop, tmp_path, capsys):
    from roibasedimagecompression_amd import container, gif
    names = []
    for i, img in enumerate((crop, np.roll(crop, 5, axis=0))):
        names.append(str(tmp_path / f"in{i}.png"))
        container.write_png(enc.quantize(img, colours=64), names[-1], rh)
    out = str(tmp_path / "out.gif")
    assert gif.main(names + [out, "--colours", "20", "--delay", "6", "--loop", "3"]) == 0
    stats = json.loads(capsys.readouterr().out)
    data = open(out, "rb").read()
    assert stats["gif"]["bytes"] == len(data) and stats["gif"]["frames"] == 2 and stats["gif"]["delta"] and stats["gif"]["colours"] <= 20
    frames, durations, loop = GC.pillow_frames(data)
    assert frames.shape == (2,) + crop.shape and durations == [60, 60] and loop == 3
    assert gif.main(names + [out, "--colours", "256", "--no-delta", "--pattern", "128", "--pattern-size", "2"]) == 0
    stats = json.loads(capsys.readouterr().out)
    assert not stats["gif"]["delta"] and len(GC.parse(open(out, "rb").read())["frames"]) == 2
