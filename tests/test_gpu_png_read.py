"""PNG files read on the device (csrc/png_read.hip: Rhccq.crc32_segments / png_unfilter / png_expand / png_decode, container.read_png /
reduce_png, a file name as the image of ImageEncoder.quantize, the command line of roibasedimagecompression_amd.png) against the numpy /
struct / zlib reference of tests/pngread_cases.py, bit for bit, and against Pillow.  GPU only.  The shapes of the unfilter tests are built
from the kernel's own band height R, tile T and granule G (ops.png_unfilter_*).  No test provokes the bounded wait's abort path."""
import json
import os
import zlib

import numpy as np
import pytest

import pngread_cases as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BPPS = (1, 2, 3, 4, 6, 8)


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


def geometry():
    from roibasedimagecompression_amd import ops
    return ops.png_unfilter_band_rows(), ops.png_unfilter_tile(), ops.png_unfilter_granule()


def heights():
    R = geometry()[0]
    return (1, 2, R - 1, R, R + 1, 2 * R + 1)


def unit_widths():
    _, T, G = geometry()
    return (1, 2, G - 1, G, G + 1, T - 1, T, T + 1)


# ---- unfilter alone ---------------------------------------------------------------------------------------------------------------------
def _unfilter(rh, scan, H, rowbytes, bpp, shift):
    """rhccq_png_unfilter itself: scan and raw_out `shift` bytes off a 4-byte boundary, raw_out inside a pre-filled buffer"""
    import torch
    n = H * rowbytes
    src = torch.full((len(scan) + 8,), 0x3C, dtype=torch.uint8, device=rh.device)
    src[4 + shift:4 + shift + len(scan)] = rh.dev(np.frombuffer(scan, np.uint8).copy())
    buf = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device=rh.device)
    ws = rh._raw.rhccq_png_unfilter_bytes(H, rowbytes, bpp)
    assert ws >= 256
    work = torch.full((ws // 4,), -1, dtype=torch.int32, device=rh.device)                      # (the call clears what it needs)
    status = torch.full((2,), -7, dtype=torch.int32, device=rh.device)
    rc = rh.lib.rhccq_png_unfilter(rh.ctx, rh._p(src[4 + shift:]), H, rowbytes, bpp, rh._p(buf[4 + shift:]), rh._p(work), rh._p(status))
    host = buf.cpu().numpy()
    assert (host[:4 + shift] == 0xA5).all() and (host[4 + shift + n:] == 0xA5).all(), "bytes outside the raw rows were written"
    return rc, host[4 + shift:4 + shift + n], tuple(int(v) for v in status.cpu().numpy())


def _check_unfilter(rh, rng, H, units, bpp, types, shift, special=False):
    rb = units * bpp
    raw = rng.choice(np.array([0, 1, 127, 128, 255], np.uint8), size=(H, rb)) if special else rng.integers(0, 256, size=(H, rb), dtype=np.uint8)
    scan = P.filter_scan(raw, bpp, types)
    want, want_status = P.unfilter_reference(scan, H, rb, bpp)
    assert np.array_equal(want.reshape(H, rb), raw) and want_status == (P.OK, 0)                # (the builder and the reference agree)
    rc, got, status = _unfilter(rh, scan, H, rb, bpp, shift)
    assert rc == 0 and status == (P.OK, 0), (H, units, bpp, shift, status)
    assert np.array_equal(got, want), (H, units, bpp, shift, list(types))


@pytest.mark.parametrize("bpp", BPPS)
def test_unfilter_every_shape_with_random_types(rh, bpp):
    rng = np.random.default_rng(1000 + bpp)
    k = 0
    for H in heights():
        for units in unit_widths():
            _check_unfilter(rh, rng, H, units, bpp, rng.integers(0, 5, size=H), k % 4)
            k += 1


@pytest.mark.parametrize("t", range(5))
def test_unfilter_every_row_of_one_type(rh, t):
    """row 0 of every type included: the row above it and the bytes left of a row are zero"""
    _, T, G = geometry()
    rng = np.random.default_rng(1100 + t)
    for H in heights():
        for bpp in BPPS:
            for units in (G + 1, T + 1):
                _check_unfilter(rh, rng, H, units, bpp, [t] * H, (H + bpp) % 4)


@pytest.mark.parametrize("where", ("band_starts", "band_ends", "nowhere"))
def test_unfilter_independent_rows_at_band_edges(rh, where):
    """rows of type 0 or 1 (which need nothing of the row above) exactly at band starts -- those bands wait for nothing --, exactly at band
    ends, and nowhere -- every band waits for the one above"""
    R, T, _ = geometry()
    H = 2 * R + 1
    rng = np.random.default_rng(1200)
    for bpp in BPPS:
        for free in (0, 1):
            types = rng.integers(2, 5, size=H)
            if where == "band_starts":
                types[R::R] = free
            elif where == "band_ends":
                types[R - 1::R] = free
            _check_unfilter(rh, rng, H, T + 1, bpp, types, bpp % 4)


@pytest.mark.parametrize("bpp", BPPS)
def test_unfilter_special_bytes(rh, bpp):
    """bytes from {0, 1, 127, 128, 255}: Paeth's ties and Average's ninth bit"""
    R, T, G = geometry()
    rng = np.random.default_rng(1300 + bpp)
    for types in ([3] * (R + 1), [4] * (R + 1), rng.integers(0, 5, size=R + 1)):
        for units in (G + 1, T + 1):
            _check_unfilter(rh, rng, R + 1, units, bpp, types, units % 4, special=True)


def test_unfilter_reports_the_first_bad_filter_row(rh):
    R = geometry()[0]
    rng = np.random.default_rng(1400)
    H, units, bpp = 2 * R + 1, 5, 3
    raw = rng.integers(0, 256, size=(H, units * bpp), dtype=np.uint8)
    types = rng.integers(0, 5, size=H)
    types[[R + 3, R - 1, 2 * R]] = (200, 5, 9)
    scan = P.filter_scan(raw, bpp, types)
    want, want_status = P.unfilter_reference(scan, H, units * bpp, bpp)
    assert want_status == (P.BAD_FILTER, R - 1)
    rc, got, status = _unfilter(rh, scan, H, units * bpp, bpp, 1)
    assert rc == 0 and status == want_status and np.array_equal(got, want)
    out, st = rh.png_unfilter(np.frombuffer(scan, np.uint8).copy(), H, units * bpp, bpp)
    assert out.is_cuda and st.is_cuda and np.array_equal(out.cpu().numpy(), want) and tuple(st.cpu().tolist()) == want_status


def test_unfilter_wrapper_validates(rh):
    from roibasedimagecompression_amd import RhccqError
    scan = np.zeros(2 * 7, np.uint8)
    with pytest.raises(RhccqError):
        rh.png_unfilter(scan, 2, 6, 5)
    with pytest.raises(RhccqError):
        rh.png_unfilter(scan, 2, 6, 4)                                                         # rowbytes not a multiple of bpp
    with pytest.raises(ValueError):
        rh.png_unfilter(scan, 3, 6, 3)
    with pytest.raises(TypeError):
        rh.png_unfilter(scan.astype(np.int32), 2, 6, 3)


# ---- segment CRCs -----------------------------------------------------------------------------------------------------------------------
def _crcs(rh, data, segments, extra=0):
    return [int(v) & 0xFFFFFFFF for v in rh.crc32_segments(data, segments, extra).cpu().numpy()]


def test_segment_crcs_lengths_and_alignments(rh):
    piece = 16384
    rng = np.random.default_rng(1500)
    data = rng.integers(0, 256, size=12 * piece, dtype=np.uint8)
    segments, at = [], 0
    for k, ln in enumerate((0, 1, 4, piece - 1, piece, piece + 1, 3 * piece + 5, 0, 2 * piece - 17, 15, 16, 17)):
        at += k % 5                                                                             # misaligned starts, gaps between the ranges
        segments.append((at, ln))
        at += ln
    assert at <= len(data)
    segments += [(7, 5), (7, 5), (len(data) - 3, 3), (len(data), 0)]                            # overlapping and repeated ranges, the buffer's end
    want = [zlib.crc32(data[o:o + n].tobytes()) for o, n in segments]
    assert _crcs(rh, data, segments) == want
    rc, host = P.host_crc_segments(data, segments)
    assert rc == 0 and host == want
    assert _crcs(rh, data, [(o, n - 4) for o, n in segments if n >= 4], extra=4) == [w for (o, n), w in zip(segments, want) if n >= 4]
    # a range that does not lie inside the buffer counts as empty
    assert _crcs(rh, data, [(len(data) - 2, 3), (-1, 4), (5, -1), (0, 2)]) == [0, 0, 0, zlib.crc32(data[:2].tobytes())]
    assert _crcs(rh, data, []) == []


def test_segment_crcs_thousands_of_one_byte_ranges(rh):
    rng = np.random.default_rng(1501)
    data = rng.integers(0, 256, size=5000, dtype=np.uint8)
    segments = [(int(o), 1) for o in rng.permutation(5000)[:4099]]
    out = rh.crc32_segments(data, segments)
    assert out.is_cuda and _crcs(rh, data, segments) == [zlib.crc32(bytes([data[o]])) for o, _ in segments]


def test_segment_crcs_of_a_files_chunks(rh):
    from roibasedimagecompression_amd.ops import png_parse
    data = P.case("split_8k")
    info, table = png_parse(data)
    assert info.status == 0 and info.n_idat >= 4
    got = _crcs(rh, np.frombuffer(data, np.uint8).copy(), table[:, :2], extra=4)
    assert got == [int.from_bytes(data[o + 4 + n:o + 8 + n], "big") for o, n in table[:, :2].tolist()]


# ---- whole files ------------------------------------------------------------------------------------------------------------------------
def _decode(rh, data, check_crc=True):
    out = rh.png_decode(data, check_crc=check_crc)
    status = tuple(int(v) for v in out["status"].cpu().numpy())
    return out, status


@pytest.mark.parametrize("name", P.names())
def test_device_file_equals_reference(rh, name):
    ref = P.reference(name)
    out, status = _decode(rh, P.case(name))
    assert status == (ref["status"], ref["detail"]) == (P.OK, 0)
    z = ref["info"]
    assert np.array_equal(out["rgb"].cpu().numpy(), ref["rgb"])
    has_alpha = z["colour_type"] in (4, 6) or len(z["trns"]) > 0
    assert (out["alpha"] is not None) == has_alpha
    if has_alpha:
        assert np.array_equal(out["alpha"].cpu().numpy(), ref["alpha"])
    assert (out["indices"] is not None) == (z["colour_type"] == 3)
    if z["colour_type"] == 3:
        assert np.array_equal(out["indices"].cpu().numpy(), ref["idx"])
    H, rb = z["height"], z["rowbytes"]
    scan = out["scan"].cpu().numpy().reshape(H, rb + 1)
    assert np.array_equal(scan, np.frombuffer(zlib.decompress(z["idat"]), np.uint8).reshape(H, rb + 1))
    # the stages alone, through their wrappers
    raw, st = rh.png_unfilter(out["scan"], H, rb, z["bpp"])
    assert tuple(st.cpu().tolist()) == (P.OK, 0) and np.array_equal(raw.cpu().numpy().reshape(H, rb), ref["raw"])
    rgb, alpha, idx = rh.png_expand(raw, H, z["width"], z["colour_type"], z["depth"], z["palette"], z["trns"])
    assert np.array_equal(rgb.cpu().numpy(), ref["rgb"]) and np.array_equal(alpha.cpu().numpy(), ref["alpha"])
    assert (idx is None) == (ref["idx"] is None) and (idx is None or np.array_equal(idx.cpu().numpy(), ref["idx"]))


@pytest.mark.parametrize("name", P.malformed_names())
def test_device_malformed_file_gives_its_status(rh, name):
    from roibasedimagecompression_amd import RhccqError, container
    want = P.expected(name)
    _, status = _decode(rh, P.case(name))
    assert status == want
    with pytest.raises(RhccqError) as e:
        container.read_png(P.case(name), rh)
    assert str(e.value) == f"read_png: RHCCQ_PNG_{P.STATUS_NAMES[want[0]]} (status {want[0]}), detail {want[1]}"


def test_crc_check_can_be_switched_off(rh):
    from roibasedimagecompression_amd import container
    for name in ("crc_of_text", "crc_of_iend"):
        _, status = _decode(rh, P.case(name), check_crc=False)
        assert status == (P.OK, 0)
        assert np.array_equal(container.read_png(P.case(name), rh, check_crc=False)["image"].cpu().numpy(), P.read_reference(P.case(name), check_crc=False)["rgb"])
    _, status = _decode(rh, P.case("crc_and_bad_stream"), check_crc=False)
    assert status == (P.BAD_STREAM, P.ZS_BAD_HEADER)


@pytest.mark.parametrize("name", P.FIXTURES)
def test_fixture_equals_pillow(rh, name):
    import torch
    from roibasedimagecompression_amd import container
    path = os.path.join(P.GOLDEN, name)
    want = P.pillow_rgb(P.fixture(name))
    fr = container.read_png(path, rh)
    assert fr["image"].is_cuda and fr["shape"] == want.shape[:2] and fr["alpha"] is None
    assert np.array_equal(fr["image"].cpu().numpy(), want)
    info = fr["info"]
    assert info["colour_type"] == 2 and info["depth"] == 8 and info["interlace"] == 0 and sum(info["filter_rows"]) == want.shape[0]
    if name == "kodak_1.png":
        assert info["filter_rows"] == [want.shape[0], 0, 0, 0, 0]
    if name == "kodak_20.png":
        assert info["filter_rows"] == [0, want.shape[0], 0, 0, 0]
    if name == "Lenna.png":
        assert info["filter_rows"][2:] == [115, 289, 107]
        # the same bytes as bytes and as a device tensor at an odd offset of a larger buffer
        data = P.fixture(name)
        assert np.array_equal(container.read_png(data, rh)["image"].cpu().numpy(), want)
        buf = torch.zeros(len(data) + 5, dtype=torch.uint8, device=rh.device)
        buf[3:3 + len(data)] = rh.dev(np.frombuffer(data, np.uint8).copy())
        assert np.array_equal(container.read_png(buf[3:3 + len(data)], rh)["image"].cpu().numpy(), want)


# ---- round trips ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colours", (2, 4, 16, 256, 1024))
def test_write_png_then_read_png(rh, enc, crop, tmp_path, colours):
    from roibasedimagecompression_amd import container
    res = enc.quantize(crop, colours)
    path = str(tmp_path / "q.png")
    container.write_png(res, path, rh)
    fr = container.read_png(path, rh)
    pal = np.asarray(res["palette"], np.uint8)
    idx = res["indices"].cpu().numpy().astype(np.int64).reshape(64, 96) & 0xFFFF
    assert fr["shape"] == (64, 96) and fr["alpha"] is None
    assert np.array_equal(fr["image"].cpu().numpy(), pal[idx])
    assert np.array_equal(fr["image"].cpu().numpy(), rh.decode(res["indices"], rh.dev(pal)).reshape(64, 96, 3).cpu().numpy())
    if len(pal) <= 256:
        assert fr["info"]["colour_type"] == 3 and fr["dtype"] == "uint8" and fr["palette_alpha"] is None
        assert np.array_equal(fr["palette"].cpu().numpy(), pal) and np.array_equal(fr["indices"].cpu().numpy().reshape(64, 96), idx)
        again = str(tmp_path / "again.png")                                                     # what read_png returns is a frame write_png takes
        container.write_png(fr, again, rh, exact=True)
        assert np.array_equal(P.pillow_rgb(open(again, "rb").read()), pal[idx])
    else:
        assert fr["info"]["colour_type"] == 2 and "palette" not in fr


def test_quantize_a_file_equals_quantize_its_pixels(rh, enc, crop, tmp_path):
    from PIL import Image
    path = str(tmp_path / "in.png")
    Image.fromarray(crop).save(path)
    a = enc.quantize(path, 16, refine=2)
    b = enc.quantize(crop, 16, refine=2)
    assert np.array_equal(a["palette"], b["palette"]) and np.array_equal(a["indices"].cpu().numpy(), b["indices"].cpu().numpy())
    sa = {k: v for k, v in a["stats"].items() if k not in ("seconds", "png_in")}
    sb = {k: v for k, v in b["stats"].items() if k != "seconds"}
    assert sa == sb and "png_in" not in b["stats"]
    assert a["stats"]["png_in"]["shape"] == [64, 96] and a["stats"]["png_in"]["colour_type"] == 2 and a["stats"]["png_in"]["alpha_ignored"] is False
    rgba = str(tmp_path / "rgba.png")
    Image.fromarray(np.dstack([crop, np.full((64, 96), 77, np.uint8)])).save(rgba)
    c = enc.quantize(rgba, 16, refine=2)
    assert c["stats"]["png_in"]["alpha_ignored"] is True and np.array_equal(c["indices"].cpu().numpy(), b["indices"].cpu().numpy())
    pal = enc.quantize(crop, 8)["palette"]
    d = enc.encode_with_palette(path, pal)
    e = enc.encode_with_palette(crop, pal)
    assert np.array_equal(d["indices"].cpu().numpy(), e["indices"].cpu().numpy()) and d["stats"]["png_in"]["idat_chunks"] >= 1


def test_reduce_png_equals_reduce_frame(rh, enc, crop, tmp_path):
    from roibasedimagecompression_amd import RhccqError, container
    res = enc.quantize(crop, 200)
    src_f, src_p, dst_f, dst_p = (str(tmp_path / n) for n in ("a.rhccq", "a.png", "b.rhccq", "b.png"))
    container.write_frame(res, src_f, rh)
    container.write_png(res, src_p, rh)
    rf = container.reduce_frame(src_f, dst_f, 16, rh)
    rp = container.reduce_png(src_p, dst_p, 16, rh)
    assert {k: v for k, v in rf.items() if k != "bytes"} == {k: v for k, v in rp.items() if k != "bytes"}
    assert rp["bytes"] == os.path.getsize(dst_p) and rp["to"] <= 16
    ff, fp = container.read_frame(dst_f, rh), container.read_png(dst_p, rh)
    assert np.array_equal(ff["palette"].cpu().numpy(), fp["palette"].cpu().numpy())
    assert np.array_equal(ff["indices"].cpu().numpy().reshape(-1), fp["indices"].cpu().numpy().reshape(-1))
    big = str(tmp_path / "big.png")
    container.write_png(enc.quantize(crop, 1024), big, rh)
    with pytest.raises(RhccqError):
        container.reduce_png(big, dst_p, 16, rh)                                               # truecolour: no palette to reduce


def test_command_line_in_process(rh, enc, crop, tmp_path, capsys):
    from PIL import Image
    from roibasedimagecompression_amd import png
    src, dst = str(tmp_path / "in.png"), str(tmp_path / "out.png")
    Image.fromarray(crop).save(src)
    assert png.main([src, dst, "--colours", "16", "--refine", "1", "--exact"]) == 0
    stats = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert stats["png_in"]["shape"] == [64, 96] and stats["png"]["colour_type"] == 3 and stats["build"]["asked"] == 16
    res = enc.quantize(crop, 16, refine=1)
    want = np.asarray(res["palette"], np.uint8)[res["indices"].cpu().numpy().astype(np.int64).reshape(64, 96)]
    assert np.array_equal(P.pillow_rgb(open(dst, "rb").read()), want)
