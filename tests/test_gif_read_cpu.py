"""rhccq_gif_parse_host, rhccq_gif_unlzw_host, rhccq_gif_compose_host and rhccq_gif_decode_host (csrc/gif_read.h run serially; include/rhccq.h
"GIF files read on the device") against the textbook reference of tests/gifread_cases.py, bit for bit; that reference against Pillow; files
Pillow and the project's own writer make; every malformed case's status and detail; argument errors; the Python layer's checks and the
command line's parsing.  No GPU.

Pillow and the definition.  PILLOW_AGREE names the cases Pillow 12 (seek + convert("RGBA")) shows exactly as the header defines them.  Left
off are the five cases with pixels that no frame has painted, or that a disposal has cleared: the header shows such a pixel as (0, 0, 0)
with alpha 0, Pillow shows the screen's background colour there (and its alpha plane differs in places); on the pixels that are covered
the two agree in those files too, up to the frames with disposal 4 and more.  They are segment_counts, scan_step_counts and interlace_heights (frames
smaller than the screen), disposals (partial frames, disposals 2 and 3) and extensions (a first frame with disposal 2)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import gif_cases as GC
import gifread_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PILLOW_OFF = ("segment_counts", "scan_step_counts", "interlace_heights", "disposals", "extensions")
PILLOW_AGREE = [n for n in R.names() if n not in PILLOW_OFF]
_ptr = R._ptr


@pytest.mark.parametrize("name", R.names())
def test_host_decode_equals_reference(name):
    ref = R.reference(name)
    rc, st, dt, rgb, alpha, idx = R.host_decode(R.case(name))
    assert rc == 0 and (st, dt) == (R.OK, 0), (name, rc, st, dt)
    info, frames, _ = R.host_parse(R.case(name))
    assert np.array_equal(rgb, ref["images"]) and np.array_equal(alpha, ref["alpha"]), name
    assert all(np.array_equal(a, b) for a, b in zip(R.frame_maps(idx, frames, info.n_frames), ref["indices"])), name


@pytest.mark.parametrize("name", R.names())
def test_host_parse_and_stages_equal_reference(name):
    data, ref = R.case(name), R.reference(name)
    info, frames, blocks = R.host_parse(data)
    F = info.n_frames
    assert (info.status, info.detail, info.width, info.height, F) == (0, 0, ref["W"], ref["H"], len(ref["frames"]))
    assert (None if info.loop < 0 else info.loop) == ref["loop"] and info.pixels == sum(ref["counts"]) and info.n_blocks == len(blocks)
    at, row = 0, 0
    for f, fr in enumerate(ref["frames"]):
        g = frames[f]
        assert (g.x, g.y, g.w, g.h) == fr["rect"] and bool(g.interlace) == fr["interlaced"] and g.m == fr["m"] and g.table_rows == len(fr["table"])
        assert (None if g.transparent < 0 else g.transparent) == fr["transparent"] and (g.disposal, g.delay) == (fr["disposal"], fr["delay"])
        assert data[g.table_offset:g.table_offset + 3 * g.table_rows] == fr["table"].tobytes()
        assert g.stream_offset == at and g.stream_offset % 16 == 0 and g.stream_bytes == len(fr["stream"]) and g.first_row == row
        assert [(int(o), int(ln)) for o, ln, _, _ in blocks[g.first_block:g.first_block + g.n_blocks]] == fr["blocks"]
        assert (blocks[g.first_block:g.first_block + g.n_blocks, 2] == f).all()
        at = (at + g.stream_bytes + 15) // 16 * 16 + 16
        row += 8 * g.stream_bytes // (2 * (g.m + 1)) + 1
        assert ref["info"][f]["segments"] <= 8 * g.stream_bytes // (2 * (g.m + 1)) + 1, "the segment table's bound"
    assert info.stream_bytes == at and info.seg_rows == row
    streams = R.joined_streams(data)
    for f, fr in enumerate(ref["frames"]):
        assert streams[frames[f].stream_offset:frames[f].stream_offset + frames[f].stream_bytes].tobytes() == fr["stream"]
    # the two stages alone
    pixels = np.full(info.pixels + 32, 0xA5, np.uint8)
    counts, st, segs = np.full(F, -1, np.int64), np.full(2, -7, np.int32), C.c_int64(-1)
    rc = R.lib().rhccq_gif_unlzw_host(_ptr(streams), len(streams), C.cast(frames, C.c_void_p), F, _ptr(pixels[16:]), info.pixels, _ptr(counts), _ptr(st),
                                      C.byref(segs))
    assert rc == 0 and st.tolist() == [0, 0] and counts.tolist() == ref["counts"] and segs.value == sum(i["segments"] for i in ref["info"])
    assert pixels[16:-16].tobytes() == b"".join(ref["pixels"]) and (pixels[:16] == 0xA5).all() and (pixels[-16:] == 0xA5).all()
    H, W = info.height, info.width
    rgb, alpha, idx = np.zeros((F, H, W, 3), np.uint8), np.zeros((F, H, W), np.uint8), np.zeros(info.pixels, np.uint8)
    a = np.frombuffer(data, np.uint8)
    rc = R.lib().rhccq_gif_compose_host(_ptr(pixels[16:]), info.pixels, _ptr(a), len(a), C.cast(frames, C.c_void_p), F, H, W, _ptr(rgb), _ptr(alpha), _ptr(idx))
    assert rc == 0 and np.array_equal(rgb, ref["images"]) and np.array_equal(alpha, ref["alpha"])
    rgb2 = np.zeros_like(rgb)
    assert R.lib().rhccq_gif_compose_host(_ptr(pixels[16:]), info.pixels, _ptr(a), len(a), C.cast(frames, C.c_void_p), F, H, W, _ptr(rgb2), None, None) == 0
    assert np.array_equal(rgb2, rgb)                                            # alpha and idx may be NULL


@pytest.mark.parametrize("name", PILLOW_AGREE)
def test_reference_equals_pillow(name):
    ref = R.reference(name)
    view, durations, loop = R.pillow_view(R.case(name))
    assert np.array_equal(ref["images"], view[..., :3]) and np.array_equal(ref["alpha"], view[..., 3]), name
    assert loop == ref["loop"] and [d or 0 for d in durations] == [10 * d for d in ref["delays"]]


def test_pillow_is_asked_about_every_kind_of_file():
    frames = [fr for n in PILLOW_AGREE for fr in R.ref_parse(R.case(n))["frames"]]
    screens = {n: (R.ref_parse(R.case(n))["W"], R.ref_parse(R.case(n))["H"]) for n in PILLOW_AGREE}
    assert any(fr["interlaced"] for fr in frames) and any(fr["transparent"] is not None for fr in frames)
    assert any(len(R.ref_parse(R.case(n))["frames"]) > 1 for n in PILLOW_AGREE)
    assert any(fr["rect"][2:] != screens[n] for n in PILLOW_AGREE for fr in R.ref_parse(R.case(n))["frames"]), "a cropped rectangle"
    assert "local_only" in PILLOW_AGREE and "placement_mixed_tables" in PILLOW_AGREE and "transparent_over_full" in PILLOW_AGREE
    assert sorted(PILLOW_AGREE + list(PILLOW_OFF)) == sorted(R.names())


@pytest.mark.parametrize("name", list(R.pillow_files()))
def test_files_pillow_writes(name):
    data = R.pillow_files()[name]
    view, durations, loop = R.pillow_view(data)
    rc, st, dt, rgb, alpha, idx = R.host_decode(data)
    assert rc == 0 and (st, dt) == (0, 0)
    assert np.array_equal(rgb, view[..., :3]) and np.array_equal(alpha, view[..., 3]), name
    ref = R.ref_decode(data)
    assert np.array_equal(ref["images"], rgb) and ref["loop"] == loop and [10 * d for d in ref["delays"]] == [d or 0 for d in durations]


def test_pillow_files_are_what_they_are_meant_to_be():
    kinds = {n: R.ref_parse(d)["frames"] for n, d in R.pillow_files().items()}
    assert all(kinds[f"still_{k}"][0]["interlaced"] for k in (2, 16, 256)) and not kinds["still_plain_rows"][0]["interlaced"]
    assert [len(kinds[n]) for n in ("animation", "animation_disposal2", "animation_full_frames")] == [4, 4, 4]
    assert all(fr["rect"][2:] != (96, 64) and fr["transparent"] is not None for fr in kinds["animation"][1:]), "cropped, optimised frames"
    assert all(fr["disposal"] == 2 for fr in kinds["animation_disposal2"])
    assert R.ref_decode(R.pillow_files()["still_256"])["info"][0]["segments"] >= 2, "a Clear where the table fills"


@pytest.mark.parametrize("name", GC.names())
def test_files_of_the_writer_reference(name):
    v = GC.case(name)
    data = GC.reference(name)[0]
    rc, st, dt, rgb, alpha, idx = R.host_decode(data)
    assert rc == 0 and (st, dt) == (0, 0), name
    assert np.array_equal(rgb, GC.decoded(v["frames"], v["palettes"])) and (alpha == 255).all(), name
    ref = R.ref_decode(data)
    assert np.array_equal(ref["images"], rgb) and ref["delays"] == v["delays"] and ref["loop"] == (v["loop"] if len(v["frames"]) > 1 else None)
    n = v["frames"][0].size
    assert all(i["segments"] >= -(-n // GC.S) for i in ref["info"]), "a Clear per 16 384 pixels at the least (and one wherever the table fills)"


@pytest.mark.parametrize("name", R.malformed_names())
def test_malformed_file_gives_its_status_and_detail(name):
    rc, st, dt, *_ = R.host_decode(R.case(name))
    assert rc == 0 and (st, dt) == R.expected(name), (name, st, dt)
    info = R.host_parse(R.case(name))[0]
    if st <= R.LIMIT:
        assert (info.status, info.detail) == (st, dt)
    else:
        assert info.status == R.OK


def test_every_status_has_a_case():
    assert {R.expected(n)[0] for n in R.malformed_names()} == set(range(1, 11))
    assert [getattr(R, n) for n in R.STATUS_NAMES] == list(range(11))


def test_every_prefix_of_a_file_is_refused_or_read():
    """the parser on every prefix of a small animation: a status, never a read past the bytes it was given (the copies are exact)"""
    data = R.case("extensions")
    seen = set()
    for n in range(len(data) + 1):
        info = R.host_parse(bytes(data[:n]))[0]
        seen.add(info.status)
        assert info.status in (R.BAD_SIGNATURE, R.TRUNCATED) or n >= len(data) - len(b"trailing bytes \x2c\x21"), n
    assert seen == {R.BAD_SIGNATURE, R.TRUNCATED, R.OK}


def test_argument_errors():
    lib = R.lib()
    from roibasedimagecompression_amd import _lib
    data = R.case("placement_mixed_tables")
    a = np.frombuffer(data, np.uint8)
    info, frames, blocks = R.host_parse(data)
    F, H, W = info.n_frames, info.height, info.width
    nf, nb, gi = C.c_int64(), C.c_int64(), _lib.GifInfo()
    parse = lib.rhccq_gif_parse_host
    assert parse(None, 5, C.byref(gi), None, 0, C.byref(nf), None, 0, C.byref(nb)) == R.E_ARG
    assert parse(_ptr(a), -1, C.byref(gi), None, 0, C.byref(nf), None, 0, C.byref(nb)) == R.E_ARG
    assert parse(_ptr(a), len(a), None, None, 0, C.byref(nf), None, 0, C.byref(nb)) == R.E_ARG
    assert parse(_ptr(a), len(a), C.byref(gi), None, 1, C.byref(nf), None, 0, C.byref(nb)) == R.E_ARG
    assert parse(_ptr(a), len(a), C.byref(gi), None, 0, C.byref(nf), None, -1, C.byref(nb)) == R.E_ARG
    assert parse(_ptr(a), len(a), C.byref(gi), None, 0, None, None, 0, C.byref(nb)) == R.E_ARG
    # tables too small for the file change nothing but the rows they hold
    small = (_lib.GifFrame * 2)()
    rows = np.zeros((3, 4), np.int64)
    assert parse(_ptr(a), len(a), C.byref(gi), C.cast(small, C.c_void_p), 2, C.byref(nf), _ptr(rows), 3, C.byref(nb)) == 0
    assert (nf.value, nb.value, gi.status, gi.pixels, gi.seg_rows) == (F, info.n_blocks, 0, info.pixels, info.seg_rows)
    assert bytes(small) == bytes(frames)[:C.sizeof(small)] and np.array_equal(rows, blocks[:3])
    ws = C.c_int64()
    assert lib.rhccq_gif_read_sizes(C.byref(info), len(a), C.byref(ws)) == 0 and ws.value >= info.pixels + info.stream_bytes + 16 * info.seg_rows
    assert lib.rhccq_gif_read_sizes(None, len(a), C.byref(ws)) == R.E_ARG and lib.rhccq_gif_read_sizes(C.byref(info), -1, C.byref(ws)) == R.E_ARG
    assert lib.rhccq_gif_read_sizes(C.byref(info), len(a), None) == R.E_ARG
    bad = _lib.GifInfo.from_buffer_copy(info)
    bad.seg_rows = -1
    assert lib.rhccq_gif_read_sizes(C.byref(bad), len(a), C.byref(ws)) == R.E_ARG
    refused = R.host_parse(R.case("no_frames"))[0]
    assert lib.rhccq_gif_read_sizes(C.byref(refused), 1, C.byref(ws)) == 0 and ws.value == 256
    fp = C.cast(frames, C.c_void_p)
    assert lib.rhccq_gif_unlzw_bytes(fp, F) >= 16 * info.seg_rows and lib.rhccq_gif_unlzw_bytes(None, F) == R.E_ARG
    assert lib.rhccq_gif_unlzw_bytes(fp, 0) == R.E_ARG and lib.rhccq_gif_unlzw_bytes(fp, (1 << 20) + 1) == R.E_ARG
    streams = R.joined_streams(data)
    pixels, counts, st = np.zeros(info.pixels, np.uint8), np.zeros(F, np.int64), np.zeros(2, np.int32)
    unlzw = lib.rhccq_gif_unlzw_host
    assert unlzw(_ptr(streams), len(streams), fp, F, _ptr(pixels), info.pixels, _ptr(counts), _ptr(st), None) == 0 and st.tolist() == [0, 0]
    assert unlzw(None, len(streams), fp, F, _ptr(pixels), info.pixels, _ptr(counts), _ptr(st), None) == R.E_ARG
    assert unlzw(_ptr(streams), len(streams), fp, 0, _ptr(pixels), info.pixels, _ptr(counts), _ptr(st), None) == R.E_ARG
    assert unlzw(_ptr(streams), len(streams), fp, F, _ptr(pixels), info.pixels, _ptr(counts), None, None) == R.E_ARG
    assert unlzw(_ptr(streams), len(streams) - 16, fp, F, _ptr(pixels), info.pixels, _ptr(counts), _ptr(st), None) == R.E_ARG   # a short stream buffer
    assert unlzw(_ptr(streams), len(streams), fp, F, _ptr(pixels), info.pixels - 1, _ptr(counts), _ptr(st), None) == R.E_ARG    # a short pixel buffer
    moved = (_lib.GifFrame * F).from_buffer_copy(frames)
    moved[1].stream_offset += 8                                                 # (no longer a multiple of 16)
    assert unlzw(_ptr(streams), len(streams), C.cast(moved, C.c_void_p), F, _ptr(pixels), info.pixels, _ptr(counts), _ptr(st), None) == R.E_ARG
    rgb = np.zeros((F, H, W, 3), np.uint8)
    compose = lib.rhccq_gif_compose_host
    assert compose(_ptr(pixels), info.pixels, _ptr(a), len(a), fp, F, H, W, _ptr(rgb), None, None) == 0
    assert compose(None, info.pixels, _ptr(a), len(a), fp, F, H, W, _ptr(rgb), None, None) == R.E_ARG
    assert compose(_ptr(pixels), info.pixels, _ptr(a), len(a), fp, F, 0, W, _ptr(rgb), None, None) == R.E_ARG
    assert compose(_ptr(pixels), info.pixels, _ptr(a), len(a), fp, F, H, 65536, _ptr(rgb), None, None) == R.E_ARG
    assert compose(_ptr(pixels), info.pixels, _ptr(a), len(a), fp, 1 << 20, 65535, 65535, _ptr(rgb), None, None) == R.E_LIMIT
    assert compose(_ptr(pixels), info.pixels, _ptr(a), len(a), fp, F, H, W, None, None, None) == R.E_ARG
    decode = lib.rhccq_gif_decode_host
    assert decode(_ptr(a), len(a), None, None, None, _ptr(st)) == R.E_ARG and decode(_ptr(a), len(a), _ptr(rgb), None, None, None) == R.E_ARG
    assert decode(None, 3, _ptr(rgb), None, None, _ptr(st)) == R.E_ARG and decode(_ptr(a), -1, _ptr(rgb), None, None, _ptr(st)) == R.E_ARG
    assert decode(_ptr(a), len(a), _ptr(rgb), None, None, _ptr(st)) == 0 and st.tolist() == [0, 0] and np.array_equal(rgb, R.reference("placement_mixed_tables")["images"])


def test_compose_ignores_a_frame_that_does_not_fit_its_buffers():
    """a frame table that is not the parser's: the frame is skipped, nothing outside the buffers is read"""
    from roibasedimagecompression_amd import _lib
    data = R.case("local_only")
    a = np.frombuffer(data, np.uint8)
    info, frames, _ = R.host_parse(data)
    ref = R.reference("local_only")
    pixels = np.frombuffer(b"".join(ref["pixels"]), np.uint8)
    bent = (_lib.GifFrame * 3).from_buffer_copy(frames)
    bent[1].table_offset = len(a) - 5                                           # its table would leave the file
    rgb = np.zeros((3, 9, 9, 3), np.uint8)
    assert R.lib().rhccq_gif_compose_host(_ptr(pixels), len(pixels), _ptr(a), len(a), C.cast(bent, C.c_void_p), 3, 9, 9, _ptr(rgb), None, None) == 0
    assert np.array_equal(rgb[0], ref["images"][0]) and np.array_equal(rgb[1], ref["images"][0]) and np.array_equal(rgb[2], ref["images"][2])


def test_device_forms_refuse_a_null_context():
    lib = R.lib()
    assert lib.rhccq_gif_join(None, None, 0, None, 0, 0, None) == R.E_ARG
    assert lib.rhccq_gif_unlzw(None, None, 0, None, None, 1, None, None, 0, None, None) == R.E_ARG
    assert lib.rhccq_gif_compose(None, None, 0, None, 0, None, 1, 1, 1, None, None, None) == R.E_ARG
    assert lib.rhccq_gif_decode(None, None, 0, None, None, None, None, None, None, None, None, None) == R.E_ARG


def test_geometry_is_exported():
    from roibasedimagecompression_amd import ops
    assert ops.gif_read_tile() == R.T and ops.gif_read_threads() == R.T and ops.gif_read_scan_step() == R.SCAN
    assert tuple(ops.GIF_READ_STATUS) == R.STATUS_NAMES
    info, frames, blocks = ops.gif_parse(R.case("tile_counts"))
    assert info.status == 0 and info.n_frames == 7 and len(blocks) == info.n_blocks
    assert len(ops.gif_frames_array(frames, 7)) == 7 * 88


def test_command_line_arguments():
    from roibasedimagecompression_amd import gif
    a = gif.parser().parse_args(["in.gif", "out.gif", "--colours", "16"])
    assert a.files == ["in.gif", "out.gif"] and a.colours == 16 and a.delay is None and a.loop is None and not a.no_delta
    assert gif.gif_input(["in.gif"]) and gif.gif_input(["IN.GIF"]) and not gif.gif_input(["a.gif", "b.gif"]) and not gif.gif_input(["a.png"])
    a = gif.parser().parse_args(["in.gif", "out.gif", "--colours", "8", "--delay", "5", "--loop", "3", "--refine", "2", "--pattern", "64", "--pattern-size", "8"])
    assert (a.delay, a.loop, a.refine, a.pattern, a.pattern_size) == (5, 3, 2, 64, 8)
    for bad in (["in.gif", "out.gif"], ["in.gif", "--colours", "4"], ["in.gif", "out.gif", "--colours", "x"], ["in.gif", "out.gif", "--colours", "4", "--delay", "x"]):
        with pytest.raises(SystemExit) as e:
            gif.main(bad)
        assert e.value.code == 2


def test_animate_checks_its_keywords_before_it_reads_a_gif():
    from roibasedimagecompression_amd.image import ImageEncoder
    enc = ImageEncoder.__new__(ImageEncoder)                                    # (no context: the checks come first)
    enc.rh = None
    for colours in (0, 257):
        with pytest.raises(ValueError) as e:
            enc.animate("missing.gif", colours)
        assert str(e.value) == "ImageEncoder.animate: colours must be 1..256 (a GIF colour table has at most 256 rows)"
    with pytest.raises(ValueError) as e:
        enc.animate(b"GIF89a", 16, refine=65)
    assert str(e.value) == "ImageEncoder.animate: refine must be 0..64"


def test_device_entry_point_raises_without_a_gpu():
    """no CPU fallback: container.read_gif needs the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError, container
    if torch.cuda.is_available():
        assert container.read_gif(R.case("px1"))["shape"] == (1, 1)
    else:
        with pytest.raises(RhccqError):
            container.read_gif(R.case("px1"))
        with pytest.raises(RhccqError):
            container.reduce_gif(R.case("px1"), "unused.gif", 4)


def test_parser_and_step_functions_under_the_host_sanitizers(tmp_path):
    """tests/native/gif_read_host_test.cpp: csrc/gif_read.h needs no HIP.  The corpus is every valid and malformed case (the large flat frame
    left out: the sanitizers take a minute over it); the parser also sees every prefix of each, the decoder buffers of exactly the promised
    sizes."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    lines = []
    for i, name in enumerate([n for n in R.names() if n != "flat_deep"] + R.malformed_names()):
        fn = f"{i:03d}.gif"
        (corpus / fn).write_bytes(R.case(name))
        if name in R.names():
            ref = R.reference(name)
            (corpus / (fn + ".rgb")).write_bytes(ref["images"].tobytes())
            (corpus / (fn + ".alpha")).write_bytes(ref["alpha"].tobytes())
            lines.append(f"{fn} 0 0 1")
        else:
            status, detail = R.expected(name)
            lines.append(f"{fn} {status} {detail} 0")
    (corpus / "manifest").write_text("\n".join(lines) + "\n")
    exe = tmp_path / "gif_read_host_test"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "roibasedimagecompression_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "gif_read_host_test.cpp"), "-o", str(exe)]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == f"gif_read_host ok {len(lines)}", (r.returncode, r.stdout, r.stderr)
