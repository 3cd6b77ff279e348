"""rhccq_png_parse_host, rhccq_png_unfilter_host, rhccq_png_expand_host, rhccq_crc32_segments_host and rhccq_png_decode_host (csrc/png_read.h
run serially: csrc/png_read.hip) against the numpy / struct / zlib reference of tests/pngread_cases.py, bit for bit; the reference itself
against Pillow; the project's fixtures; every malformed case's exact status and detail; argument errors; the command line's arguments;
and the parser and step functions once more as a stand-alone program under the host sanitizers.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import pngread_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ptr = P._ptr


@pytest.mark.parametrize("name", P.names())
def test_host_decode_equals_reference(name):
    ref = P.reference(name)
    assert (ref["status"], ref["detail"]) == (P.OK, 0)
    rc, status, detail, rgb, alpha, idx = P.host_decode(P.case(name))
    assert (rc, status, detail) == (0, P.OK, 0)
    assert np.array_equal(rgb, ref["rgb"]) and np.array_equal(alpha, ref["alpha"])
    if ref["idx"] is not None:
        assert np.array_equal(idx, ref["idx"])
    a = np.frombuffer(P.case(name), np.uint8)
    st = np.zeros(2, np.int32)
    assert P.lib().rhccq_png_decode_host(_ptr(a), len(a), 0, _ptr(rgb), None, None, _ptr(st)) == 0 and st.tolist() == [0, 0]   # alpha and idx may be NULL


@pytest.mark.parametrize("name", P.names())
def test_host_parse_and_stages_equal_reference(name):
    z = P.reference(name)["info"]
    rc, info, table = P.host_parse(P.case(name))
    assert rc == 0 and info.status == P.OK and info.n_chunks == len(table) == len(z["chunks"])
    assert (info.width, info.height, info.depth, info.colour_type, info.interlace) == (z["width"], z["height"], z["depth"], z["colour_type"], 0)
    assert (info.channels, info.bpp, info.rowbytes) == (P.CHANNELS[z["colour_type"]], z["bpp"], z["rowbytes"])
    assert info.scan_bytes == z["height"] * (1 + z["rowbytes"]) and info.idat_bytes == len(z["idat"])
    assert info.palette_rows == z["palette_rows"] and info.trns_bytes == len(z["trns"])
    assert [(int(o), int(n), int(d)) for o, n, _, d in table] == z["chunks"]
    idat = [i for i, c in enumerate(z["chunks"]) if c[2] >= 0]
    assert (info.first_idat, info.n_idat) == (idat[0], len(idat))
    data = P.case(name)
    if z["colour_type"] == 3:
        assert data[info.plte_offset - 4:info.plte_offset] == b"PLTE"
    if info.trns_bytes:
        assert data[info.trns_offset - 4:info.trns_offset] == b"tRNS" and data[info.trns_offset:info.trns_offset + info.trns_bytes] == z["trns"]
    pieces = [0 if n + 4 <= 0 else ((o & 15) + n + 4 + 16383) // 16384 for o, n, _ in z["chunks"]]
    assert table[:, 2].tolist() == np.concatenate([[0], np.cumsum(pieces)[:-1]]).tolist() and info.crc_pieces == sum(pieces)
    # the chunk CRCs as segments, then the stages one by one
    rc, crcs = P.host_crc_segments(np.frombuffer(data, np.uint8), [(o, n) for o, n, _ in z["chunks"]], extra=4)
    assert rc == 0 and crcs == [int.from_bytes(data[o + 4 + n:o + 8 + n], "big") for o, n, _ in z["chunks"]]
    H, rb = z["height"], z["rowbytes"]
    rc, raw, status = P.host_unfilter(zlib.decompress(z["idat"]), H, rb, z["bpp"])
    assert rc == 0 and status == (P.OK, 0) and np.array_equal(raw.reshape(H, rb), P.reference(name)["raw"])


@pytest.mark.parametrize("name", P.pillow_names())
def test_reference_equals_pillow(name):
    assert np.array_equal(P.reference(name)["rgb"], P.pillow_rgb(P.case(name)))


def test_pillow_is_asked_about_every_colour_type_and_depth():
    asked = set(P.pillow_names())
    for ct, depths in P.DEPTHS.items():
        for d in depths:
            assert (f"t{ct}_d{d}" in asked) == (not (ct == 0 and d == 16))


@pytest.mark.parametrize("name", P.FIXTURES)
def test_fixture_through_the_host_form_equals_pillow(name):
    data = P.fixture(name)
    want = P.pillow_rgb(data)
    rc, status, detail, rgb, _, _ = P.host_decode(data)
    assert (rc, status, detail) == (0, P.OK, 0) and np.array_equal(rgb, want)
    _, info, table = P.host_parse(data)
    assert info.n_idat >= 1 and info.n_chunks == len(table) >= 3


@pytest.mark.parametrize("name", P.malformed_names())
def test_malformed_file_gives_its_status_and_detail(name):
    want = P.expected(name)
    ref = P.read_reference(P.case(name))
    assert (ref["status"], ref["detail"]) == want
    rc, status, detail, _, _, _ = P.host_decode(P.case(name))
    assert (rc, status, detail) == (0,) + want
    rc, info, _ = P.host_parse(P.case(name))
    assert rc == 0 and ((info.status, info.detail) == want if want[0] <= P.LIMIT else info.status == P.OK)


def test_crc_check_can_be_switched_off():
    for name in ("crc_of_text", "crc_of_iend", "crc_of_ihdr_and_idat"):
        rc, status, detail, rgb, _, _ = P.host_decode(P.case(name), P.NO_CRC)
        assert (rc, status, detail) == (0, P.OK, 0) and np.array_equal(rgb, P.read_reference(P.case(name), check_crc=False)["rgb"])
    assert P.host_decode(P.case("crc_and_bad_stream"), P.NO_CRC)[:3] == (0, P.BAD_STREAM, P.ZS_BAD_HEADER)


def test_unfilter_host_on_a_bad_filter_row_and_every_bpp():
    rng = np.random.default_rng(7)
    for bpp in (1, 2, 3, 4, 6, 8):
        H, rb = 70, 5 * bpp
        raw = rng.choice(np.array([0, 1, 127, 128, 255], np.uint8), size=(H, rb))
        types = rng.integers(0, 5, size=H)
        scan = P.filter_scan(raw, bpp, types)
        rc, got, status = P.host_unfilter(scan, H, rb, bpp)
        assert rc == 0 and status == (P.OK, 0) and np.array_equal(got.reshape(H, rb), raw)
        types[[40, 9]] = (6, 77)
        scan = P.filter_scan(raw, bpp, types)
        want, want_status = P.unfilter_reference(scan, H, rb, bpp)
        rc, got, status = P.host_unfilter(scan, H, rb, bpp)
        assert rc == 0 and status == want_status == (P.BAD_FILTER, 9) and np.array_equal(got, want)


def test_host_crc_segments():
    rng = np.random.default_rng(8)
    data = rng.integers(0, 256, size=40000, dtype=np.uint8)
    segments = [(0, 0), (1, 1), (3, 4), (5, 16383), (7, 16384), (9, 16385), (11, 39989), (40000, 0), (39999, 1)]
    rc, crcs = P.host_crc_segments(data, segments)
    assert rc == 0 and crcs == [zlib.crc32(data[o:o + n].tobytes()) for o, n in segments]
    assert P.host_crc_segments(data, [(39999, 2), (-1, 1), (0, -1)]) == (0, [0, 0, 0])        # not inside the buffer: empty


def test_argument_errors():
    lib = P.lib()
    from roibasedimagecompression_amd import _lib
    a = np.frombuffer(P.case("t2_d8"), np.uint8)
    info, count = _lib.PngInfo(), C.c_int64()
    table = np.zeros((64, 4), np.int64)
    assert lib.rhccq_png_parse_host(_ptr(a), len(a), C.byref(info), _ptr(table), 64, C.byref(count)) == 0 and count.value == 3
    assert lib.rhccq_png_parse_host(_ptr(a), len(a), C.byref(info), None, 0, C.byref(count)) == 0 and count.value == 3 and info.status == 0
    assert lib.rhccq_png_parse_host(_ptr(a), len(a), C.byref(info), _ptr(table), 1, C.byref(count)) == 0 and count.value == 3
    assert lib.rhccq_png_parse_host(None, 5, C.byref(info), None, 0, C.byref(count)) == P.E_ARG
    assert lib.rhccq_png_parse_host(_ptr(a), -1, C.byref(info), None, 0, C.byref(count)) == P.E_ARG
    assert lib.rhccq_png_parse_host(_ptr(a), len(a), None, None, 0, C.byref(count)) == P.E_ARG
    assert lib.rhccq_png_parse_host(_ptr(a), len(a), C.byref(info), None, 4, C.byref(count)) == P.E_ARG
    assert lib.rhccq_png_parse_host(_ptr(a), len(a), C.byref(info), None, 0, None) == P.E_ARG
    scan, raw, st = np.zeros(14, np.uint8), np.zeros(12, np.uint8), np.zeros(2, np.int32)
    assert lib.rhccq_png_unfilter_host(_ptr(scan), 2, 6, 3, _ptr(raw), _ptr(st)) == 0
    for H, rb, bpp in ((0, 6, 3), (2, 0, 3), (2, 6, 5), (2, 6, 4), (2, 6, 0), (1 << 16, 1 << 15, 1)):
        assert lib.rhccq_png_unfilter_host(_ptr(scan), H, rb, bpp, _ptr(raw), _ptr(st)) == P.E_ARG
        assert lib.rhccq_png_unfilter_bytes(H, rb, bpp) == P.E_ARG
    assert lib.rhccq_png_unfilter_host(None, 2, 6, 3, _ptr(raw), _ptr(st)) == P.E_ARG
    assert lib.rhccq_png_unfilter_bytes(2, 6, 3) == 256 and lib.rhccq_png_unfilter_bytes(65, 6, 3) == 256 + 4 * 2
    assert lib.rhccq_png_unfilter_bytes(129, 16, 8) == 256 + 4 * 2 * 2 * 3
    rgb = np.zeros(12, np.uint8)
    assert lib.rhccq_png_expand_host(_ptr(raw), 2, 2, 2, 8, None, 0, None, 0, _ptr(rgb), None, None) == 0
    assert lib.rhccq_png_expand_host(_ptr(raw), 2, 2, 2, 4, None, 0, None, 0, _ptr(rgb), None, None) == P.E_ARG
    assert lib.rhccq_png_expand_host(_ptr(raw), 2, 2, 3, 8, None, 0, None, 0, _ptr(rgb), None, None) == P.E_ARG     # colour type 3 without a palette
    assert lib.rhccq_png_expand_host(_ptr(raw), 2, 2, 3, 8, _ptr(raw), 257, None, 0, _ptr(rgb), None, None) == P.E_ARG
    assert lib.rhccq_png_expand_host(_ptr(raw), 2, 2, 2, 8, None, 0, None, 6, _ptr(rgb), None, None) == P.E_ARG
    assert lib.rhccq_png_expand_host(_ptr(raw), 0, 2, 2, 8, None, 0, None, 0, _ptr(rgb), None, None) == P.E_ARG
    assert lib.rhccq_png_decode_host(_ptr(a), len(a), 2, _ptr(rgb), None, None, _ptr(st)) == P.E_ARG
    assert lib.rhccq_png_decode_host(_ptr(a), len(a), 0, _ptr(rgb), None, None, None) == P.E_ARG
    ws = C.c_int64()
    assert lib.rhccq_png_read_sizes(C.byref(info), len(a), C.byref(ws)) == 0 and ws.value > info.scan_bytes + info.idat_bytes
    assert lib.rhccq_png_read_scan_offset(C.byref(info)) % 256 == 0
    forged = _lib.PngInfo.from_buffer_copy(info)
    forged.plte_offset, forged.colour_type, forged.palette_rows = len(a) - 2, 3, 1
    assert lib.rhccq_png_read_sizes(C.byref(forged), len(a), C.byref(ws)) == P.E_ARG             # an info that is not this file's
    assert lib.rhccq_png_read_sizes(None, len(a), C.byref(ws)) == P.E_ARG
    total = C.c_int64()
    seg = np.array([[3, 20000, 0, 0], [5, 0, 0, 0], [16, 16384, 0, 0]], np.int64)
    assert lib.rhccq_crc32_segments_plan(_ptr(seg), 3, 0, C.byref(total)) == 0 and total.value == 3 and seg[:, 2].tolist() == [0, 2, 2]
    assert lib.rhccq_crc32_segments_plan(_ptr(seg), 3, -1, C.byref(total)) == P.E_ARG
    assert lib.rhccq_abi_version() == 1


def test_device_forms_refuse_a_null_context():
    lib = P.lib()
    assert lib.rhccq_crc32_segments(None, None, 0, None, 0, 0, 0, None, None) == P.E_ARG
    assert lib.rhccq_png_unfilter(None, None, 1, 1, 1, None, None, None) == P.E_ARG
    assert lib.rhccq_png_expand(None, None, 1, 1, 0, 8, None, 0, None, 0, None, None, None) == P.E_ARG
    assert lib.rhccq_png_decode(None, None, 0, None, None, 0, None, None, None, None, None) == P.E_ARG
    assert lib.rhccq_png_join(None, None, 0, None, 0, 0, None) == P.E_ARG


def test_geometry_is_exported():
    from roibasedimagecompression_amd import ops
    R, T, G = ops.png_unfilter_band_rows(), ops.png_unfilter_tile(), ops.png_unfilter_granule()
    assert R == 64 and T >= G >= 1 and T % G == 0
    info, table = ops.png_parse(P.case("split_8k"))
    assert info.status == 0 and len(table) == info.n_chunks and ops.PNG_STATUS[P.BAD_FILTER] == "BAD_FILTER" and tuple(ops.PNG_STATUS) == P.STATUS_NAMES


def test_command_line_arguments():
    from roibasedimagecompression_amd import png
    a = png.parser().parse_args(["in.png", "out.png", "--colours", "16"])
    assert (a.src, a.dst, a.colours, a.refine, a.dither, a.pattern, a.exact) == ("in.png", "out.png", 16, 0, None, None, False)
    a = png.parser().parse_args(["in.png", "out.png", "--colours", "300", "--refine", "3", "--pattern", "128", "--exact"])
    assert (a.colours, a.refine, a.dither, a.pattern, a.exact) == (300, 3, None, 128, True)
    assert png.parser().parse_args(["i", "o", "--colours", "2", "--dither", "256"]).dither == 256
    for bad in (["in.png", "out.png"], ["in.png", "--colours", "4"], ["i", "o", "--colours", "x"], ["i", "o", "--colours", "4", "--dither", "1", "--pattern", "1"]):
        with pytest.raises(SystemExit) as e:
            png.main(bad)
        assert e.value.code == 2


def test_a_file_name_is_read_only_with_a_device():
    """no CPU fallback: a file name as the image needs the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError, container
    if torch.cuda.is_available():
        assert container.read_png(P.case("t2_d8"))["shape"] == (9, 13)
    else:
        with pytest.raises(RhccqError):
            container.read_png(P.case("t2_d8"))


def test_parser_and_step_functions_under_the_host_sanitizers(tmp_path):
    """tests/native/png_read_host_test.cpp: csrc/png_read.h needs no HIP.  The corpus is every valid and malformed case; the parser also
    sees every prefix of each.  (rhccq_png_decode_host itself is not in the program: the inflater's host form lives in a .hip file.)"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    lines = []
    for i, name in enumerate(P.names() + P.malformed_names()):
        fn = f"{i:03d}.png"
        (corpus / fn).write_bytes(P.case(name))
        if name in P.names():
            ref = P.reference(name)
            (corpus / (fn + ".scan")).write_bytes(zlib.decompress(ref["info"]["idat"]))
            (corpus / (fn + ".rgb")).write_bytes(ref["rgb"].tobytes())
            lines.append(f"{fn} 0 0 1")
        else:
            status, detail = P.expected(name)
            lines.append(f"{fn} {status} {detail} 0" if status <= P.LIMIT else f"{fn} 0 0 0")
    (corpus / "manifest").write_text("\n".join(lines) + "\n")
    exe = tmp_path / "png_read_host_test"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "roibasedimagecompression_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "png_read_host_test.cpp"), "-o", str(exe)]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == f"png_read_host ok {len(lines)}", (r.returncode, r.stdout, r.stderr)
