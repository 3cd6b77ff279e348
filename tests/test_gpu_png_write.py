"""PNG files written on the device (csrc/png_write.hip: Rhccq.png_scanlines / crc32 / png_encode, container.write_png, the png_path
keyword of ImageEncoder.encode_with_palette / quantize / encode) against the numpy / struct / zlib reference of tests/png_cases.py, bit
for bit, and against Pillow and the .rhccq read path.  GPU only."""
import os
import zlib

import numpy as np
import pytest

import png_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TDT = {1: "uint8", 2: "int16", 4: "int32"}
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


def widths(name):
    return [eb for eb in PC.index_widths(len(PC.case(name)[1])) if PC.storable(name, eb)]


def _dev_idx(rh, idx, eb):
    return rh.dev(PC.index_array(idx, eb).view(_NDT[eb]).reshape(-1))


def _raw_scanlines(rh, idx, pal, flags, eb, shift):
    """rhccq_png_scanlines itself into a pre-filled buffer, `shift` bytes off a 4-byte boundary"""
    import torch
    H, W = idx.shape
    rc, n, _, _ = PC.sizes(H, W, len(pal), flags)
    assert rc == 0
    buf = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device=rh.device)
    rows = torch.full((5,), -7, dtype=torch.int64, device=rh.device)
    d_idx, d_pal = _dev_idx(rh, idx, eb), rh.dev(np.ascontiguousarray(pal))
    rc = rh.lib.rhccq_png_scanlines(rh.ctx, rh._p(d_idx), eb, H, W, rh._p(d_pal), len(pal), flags, rh._p(buf[4 + shift:]), rh._p(rows))
    host = buf.cpu().numpy()
    assert (host[:4 + shift] == 0xA5).all() and (host[4 + shift + n:] == 0xA5).all(), "bytes outside the scanlines were written"
    return rc, host[4 + shift:4 + shift + n], rows.cpu().numpy()


@pytest.mark.parametrize("name", PC.names())
def test_device_scanlines_equal_reference(rh, name):
    idx, pal, depth8, flt = PC.case(name)
    want_scan, want_rows, _ = PC.reference(name)
    for k, eb in enumerate(widths(name)):
        for shift in ((0, 1, 2, 3) if k == 0 else (k,)):
            rc, scan, rows = _raw_scanlines(rh, idx, pal, PC.flags_of(name, exact=False), eb, shift)
            assert rc == 0, (name, eb, shift)
            assert np.array_equal(scan, want_scan), (name, eb, shift)
            assert np.array_equal(rows, want_rows), (name, eb, shift)
    scan, rows = rh.png_scanlines(idx, idx.shape[0], idx.shape[1], pal, depth8=depth8, filter=flt)
    assert scan.is_cuda and rows.is_cuda and np.array_equal(scan.cpu().numpy(), want_scan) and np.array_equal(rows.cpu().numpy(), want_rows)


@pytest.mark.parametrize("n", PC.CRC_LENGTHS + (PC.CRC_LONG,))
def test_device_crc32_equals_zlib(rh, n):
    import torch
    a = PC.crc_bytes(n)
    want = zlib.crc32(a.tobytes())
    assert rh.crc32(rh.dev(a) if n else torch.empty((0,), dtype=torch.uint8, device=rh.device)) == want
    if n:
        # every alignment of the first byte modulo 16 that a short run of offsets reaches, other bytes in front and behind
        buf = torch.full((n + 40,), 0x5A, dtype=torch.uint8, device=rh.device)
        for off in ((1, 3, 4, 7, 8, 13, 15, 16) if n < 100000 else (5,)):
            buf[off:off + n] = rh.dev(a)
            assert rh.crc32(buf[off:off + n]) == want, (n, off)


def test_device_crc32_takes_a_device_side_length(rh):
    import torch
    a = PC.crc_bytes(2 * PC.CRC_PIECE + 7)
    d = rh.dev(a)
    for n in (0, 1, 5, PC.CRC_PIECE - 1, PC.CRC_PIECE, PC.CRC_PIECE + 1, len(a) - 1, len(a)):
        n_dev = torch.tensor([n], dtype=torch.int64, device=rh.device)
        out = rh.crc32_async(d, n_dev)
        assert out.is_cuda and out.dtype == torch.int32
        assert int(out.cpu()[0]) & 0xFFFFFFFF == zlib.crc32(a[:n].tobytes()), n              # (the bytes behind n differ from zeros)
        assert rh.crc32(d, n_dev) == rh.crc32(d, n) == zlib.crc32(a[:n].tobytes())
    over = torch.tensor([len(a) + 1000], dtype=torch.int64, device=rh.device)
    assert rh.crc32(d, over) == zlib.crc32(a.tobytes())                                     # clamped to the buffer
    under = torch.tensor([-3], dtype=torch.int64, device=rh.device)
    assert rh.crc32(d, under) == 0


def _raw_encode(rh, idx, pal, flags, eb):
    import torch
    H, W = idx.shape
    rc, _, ws, bound = PC.sizes(H, W, len(pal), flags)
    assert rc == 0
    work = torch.full((ws,), 0xC3, dtype=torch.uint8, device=rh.device)
    out = torch.full((bound + 16,), 0xA5, dtype=torch.uint8, device=rh.device)
    n = torch.full((1,), -1, dtype=torch.int64, device=rh.device)
    d_idx, d_pal = _dev_idx(rh, idx, eb), rh.dev(np.ascontiguousarray(pal))
    rc = rh.lib.rhccq_png_encode(rh.ctx, rh._p(d_idx), eb, H, W, rh._p(d_pal), len(pal), flags, rh._p(work), rh._p(out), bound, rh._p(n))
    host, n = out.cpu().numpy(), int(n.cpu()[0])
    assert (host[bound:] == 0xA5).all(), "bytes past the bound were written"
    return rc, host[:max(n, 0)].tobytes()


@pytest.mark.parametrize("name", PC.names())
def test_device_file_exact_equals_reference(rh, name):
    idx, pal, depth8, flt = PC.case(name)
    want = PC.reference_file(name)
    for eb in widths(name):
        rc, data = _raw_encode(rh, idx, pal, PC.flags_of(name), eb)
        assert rc == 0 and data == want, (name, eb)
    assert rh.png_encode(idx, idx.shape[0], idx.shape[1], pal, exact=True, depth8=depth8, filter=flt) == want


@pytest.mark.parametrize("name", PC.names())
def test_device_file_fast_is_a_valid_png(rh, name):
    idx, pal, depth8, flt = PC.case(name)
    K = len(pal)
    H, W = idx.shape
    rc, data = _raw_encode(rh, idx, pal, PC.flags_of(name, exact=False), widths(name)[-1])
    assert rc == 0
    parsed = PC.chunks(data)
    assert [c[0] for c in parsed] == ([b"IHDR", b"PLTE", b"IDAT", b"IEND"] if K <= 256 else [b"IHDR", b"IDAT", b"IEND"])
    assert all(stored == crc for _, _, stored, crc in parsed), [(c[0], hex(c[2]), hex(c[3])) for c in parsed]
    want = PC.chunks(PC.reference_file(name))
    assert parsed[0][1] == want[0][1] and parsed[-1][1] == b""
    if K <= 256:
        assert parsed[1][1] == pal.tobytes()
    assert zlib.decompress(parsed[-2][1]) == PC.reference(name)[0].tobytes()
    mode, img, plte = PC.pillow_image(data)
    assert mode == ("P" if K <= 256 else "RGB") and np.array_equal(img, PC.decoded(idx, pal))
    out, length = rh.png_encode_async(idx, H, W, pal, depth8=depth8, filter=flt)
    assert out.is_cuda and length.is_cuda and str(out.dtype) == "torch.uint8" and str(length.dtype) == "torch.int64"
    assert int(length.cpu()[0]) == len(rh.png_encode(idx, H, W, pal, depth8=depth8, filter=flt)) == len(data)


def test_wrapper_argument_errors(rh):
    from roibasedimagecompression_amd import RhccqError
    idx, pal = np.zeros((2, 3), np.uint8), np.zeros((4, 3), np.uint8)
    with pytest.raises(ValueError) as e:
        rh.png_encode(idx, 2, 4, pal)
    assert str(e.value) == "png_encode: indices must have H * W elements"
    with pytest.raises(ValueError) as e:
        rh.png_scanlines(idx, 2, 3, np.zeros((4, 4), np.uint8))
    assert str(e.value) == "png_scanlines: palette [K, 3] is expected"
    with pytest.raises(TypeError) as e:
        rh.png_encode(idx, 2, 3, pal.astype(np.int32))
    assert str(e.value).startswith("png_encode: palette must be uint8")
    with pytest.raises(RhccqError):
        rh.png_encode(idx, 2, 3, np.zeros((0, 3), np.uint8))


# ---- the container layer and the encoder's keyword ---------------------------------------------------------------------------------------
def _same_picture(rh, res, png, tmp_path, exact=False):
    """the PNG file opens in Pillow and shows what read_frame shows for the .rhccq written from the same result"""
    from roibasedimagecompression_amd import container
    fn = str(tmp_path / "same.rhccq")
    container.write_frame(res, fn, rh, exact=exact)
    want = container.read_frame(fn, rh)["image"].cpu().numpy()
    mode, img, plte = PC.pillow_image(png)
    assert np.array_equal(img, want)
    return mode, plte


@pytest.mark.parametrize("colours", [2, 16, 256])
def test_write_png_of_quantize_results(rh, enc, crop, tmp_path, colours):
    from roibasedimagecompression_amd import container
    res = enc.quantize(crop, colours=colours)
    fn = str(tmp_path / "q.png")
    size = container.write_png(res, fn, rh)
    data = open(fn, "rb").read()
    assert size == len(data) == os.path.getsize(fn)
    mode, plte = _same_picture(rh, res, data, tmp_path)
    assert mode == "P" and np.array_equal(plte, np.asarray(res["palette"], np.uint8))
    exact = container.png_bytes(res, rh, exact=True)
    idx = res["indices"].cpu().numpy().reshape(res["shape"])
    assert exact == PC.png_reference(idx, res["palette"])
    assert container.png_bytes(res, rh, exact=True, depth8=True) == PC.png_reference(idx, res["palette"], depth8=True)


def test_write_png_above_256_rows(rh, enc, crop, tmp_path):
    from roibasedimagecompression_amd import container
    res = enc.encode_with_palette(crop, np.random.default_rng(3).integers(0, 256, (700, 3)).astype(np.uint8))
    K = len(res["palette"])
    assert K == 700 and res["indices_dtype"] == "uint16"
    data, row = container.png_file(res, rh, exact=True)
    idx = res["indices"].cpu().numpy().view(np.uint16).reshape(res["shape"])
    assert data == PC.png_reference(idx, res["palette"])
    assert row == {"bytes": len(data), "colour_type": 2, "depth": 8, "filter_rows": PC.scanlines_reference(idx, res["palette"])[1].tolist()}
    assert _same_picture(rh, res, data, tmp_path, exact=True)[0] == "RGB"
    plain = container.png_bytes(res, rh, exact=True, filter=False)
    assert plain == PC.png_reference(idx, res["palette"], filter=False) and _same_picture(rh, res, plain, tmp_path)[0] == "RGB"
    # a list palette and host indices, as write_frame takes them
    host = {"palette": [list(map(int, r)) for r in res["palette"]], "indices": idx.reshape(-1).astype(np.int64).tolist(), "shape": res["shape"]}
    assert container.png_bytes(host, rh, exact=True) == data


def test_png_path_fills_stats_and_changes_nothing_else(rh, enc, crop, tmp_path):
    import torch
    pal = enc.quantize(crop, colours=12)["palette"]
    calls = {"quantize": lambda **kw: enc.quantize(crop, colours=12, **kw),
             "encode_with_palette": lambda **kw: enc.encode_with_palette(crop, pal, **kw),
             "encode": lambda **kw: enc.encode(crop, 20, 10, **kw)}
    for name, call in calls.items():
        fn = str(tmp_path / f"{name}.png")
        plain = call()
        res = call(png_path=fn, exact=True)
        assert "png" not in plain["stats"] and "png" not in plain["stats"]["seconds"]
        assert np.array_equal(plain["palette"], res["palette"]) and torch.equal(plain["indices"], res["indices"]), name
        assert set(res["stats"]) - {"png"} == set(plain["stats"]), name
        data = open(fn, "rb").read()
        K = len(res["palette"])
        idx = res["indices"].cpu().numpy()
        idx = (idx.view(np.uint16) if idx.dtype == np.int16 else idx).reshape(res["shape"])
        assert data == PC.png_reference(idx, res["palette"]), name
        row = res["stats"]["png"]
        assert row["bytes"] == len(data) and row["colour_type"] == (3 if K <= 256 else 2) and row["depth"] == PC.depth_of(K)
        assert row["filter_rows"] == PC.scanlines_reference(idx, res["palette"])[1].tolist() and sum(row["filter_rows"]) == idx.shape[0]
        assert _same_picture(rh, res, data, tmp_path)[0] == ("P" if K <= 256 else "RGB")


@pytest.mark.parametrize("kw", [{"dither": 256}, {"pattern": 200, "pattern_size": 4}])
def test_dithered_results_are_written_as_returned(rh, enc, crop, tmp_path, kw):
    fn, rq = str(tmp_path / "d.png"), str(tmp_path / "d.rhccq")
    res = enc.quantize(crop, colours=8, png_path=fn, out_path=rq, **kw)
    key = "dither" if "dither" in kw else "pattern"
    assert res["stats"][key]["moved"]["all"] > 0 and res["stats"]["png"]["depth"] == 4
    from roibasedimagecompression_amd import container
    want = container.read_frame(rq, rh)["image"].cpu().numpy()
    mode, img, plte = PC.pillow_image(open(fn, "rb").read())
    assert mode == "P" and np.array_equal(img, want)
    assert np.array_equal(img, PC.decoded(res["indices"].cpu().numpy().reshape(res["shape"]), res["palette"]))
