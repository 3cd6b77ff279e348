"""GIF files read on the device (csrc/gif_read.hip: Rhccq.gif_unlzw / gif_compose / gif_decode, container.read_gif / reduce_gif, a GIF as
the images of ImageEncoder.animate, the command line of roibasedimagecompression_amd.gif) against the textbook reference of
tests/gifread_cases.py, bit for bit, against the project's own writer and against Pillow.  GPU only.  The cases' code counts and segment
counts are built around the kernels' own tile and scan step (ops.gif_read_tile / gif_read_scan_step / gif_read_threads); the file reaches
the kernels at several misalignments.  No test provokes a fault: a malformed stream ends
in a status, and every output lies inside a pre-filled buffer whose other bytes are checked."""
import io
import json
import os

import numpy as np
import pytest

import gif_cases as GC
import gifread_cases as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


@pytest.fixture(scope="module")
def enc(rh):
    from roibasedimagecompression_amd.image import ImageEncoder
    return ImageEncoder(rh)


def _guarded(rh, n):
    """-> (a pre-filled device buffer, the view of n bytes inside it that a call writes)"""
    import torch
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=rh.device)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n):
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + n:] == 0xA5).all(), "bytes outside an output were written"
    return host[GUARD:GUARD + n]


def _file_tensor(rh, data, shift):
    """the file on the device, its first byte `shift` bytes behind a 16-byte boundary"""
    import torch
    raw = torch.zeros((len(data) + 32,), dtype=torch.uint8, device=rh.device)
    at = (-raw.data_ptr()) % 16 + shift
    raw[at:at + len(data)] = rh.dev(np.frombuffer(bytes(data), np.uint8).copy())
    return raw[at:at + len(data)]


def _decode(rh, data, shift=0):
    """Rhccq.gif_decode with every output inside a guarded buffer -> (status, detail, rgb, alpha, [index maps], head)"""
    from roibasedimagecompression_amd import ops
    parsed = ops.gif_parse(bytes(data))
    info, frames, _ = parsed
    if info.status:
        out = rh.gif_decode(bytes(data), parsed)
        st = out["status"].cpu().numpy()
        assert out["rgb"] is None
        return int(st[0]), int(st[1]), None, None, None, None
    F, H, W = info.n_frames, info.height, info.width
    sizes = (F * H * W * 3, F * H * W, info.pixels)
    bufs = [_guarded(rh, n) for n in sizes]
    out = rh.gif_decode(_file_tensor(rh, data, shift), parsed, rgb=bufs[0][1], alpha=bufs[1][1], idx=bufs[2][1])
    st, head = out["status"].cpu().numpy(), out["head"].cpu().numpy()
    rgb, alpha, idx = (_guards_intact(b[0], n) for b, n in zip(bufs, sizes))
    return int(st[0]), int(st[1]), rgb.reshape(F, H, W, 3), alpha.reshape(F, H, W), R.frame_maps(idx, frames, F), head


def test_geometry_is_what_the_cases_were_built_for():
    from roibasedimagecompression_amd import ops
    assert ops.gif_read_tile() == R.T and ops.gif_read_threads() == R.T and ops.gif_read_scan_step() == R.SCAN


@pytest.mark.parametrize("name", R.names())
def test_decode_equals_reference(rh, name):
    ref = R.reference(name)
    for shift in ((0, 1, 7, 15) if len(R.case(name)) < 20000 else (0, 5)):
        st, dt, rgb, alpha, maps, head = _decode(rh, R.case(name), shift)
        assert (st, dt) == (R.OK, 0), (name, shift, st, dt)
        assert np.array_equal(rgb, ref["images"]) and np.array_equal(alpha, ref["alpha"]), (name, shift)
        assert all(np.array_equal(a, b) for a, b in zip(maps, ref["indices"])), (name, shift)
        assert int(head[2]) == sum(i["segments"] for i in ref["info"]), (name, "segments")


@pytest.mark.parametrize("name", R.names())
def test_unlzw_and_compose_equal_reference(rh, name):
    from roibasedimagecompression_amd import ops
    data, ref = R.case(name), R.reference(name)
    info, frames, _ = ops.gif_parse(data)
    F = info.n_frames
    want = b"".join(ref["pixels"])
    buf, view = _guarded(rh, info.pixels)
    pixels, counts, status, head = rh.gif_unlzw(R.joined_streams(data), frames, F, pixels=view)
    assert status.cpu().numpy().tolist() == [R.OK, 0] and counts.cpu().numpy().tolist() == ref["counts"], name
    assert _guards_intact(buf, info.pixels).tobytes() == want, name
    assert head.cpu().numpy()[:3].tolist() == [-1, -1, sum(i["segments"] for i in ref["info"])]
    bufs = [_guarded(rh, n) for n in (F * info.height * info.width * 3, F * info.height * info.width, info.pixels)]
    rh.gif_compose(np.frombuffer(want, np.uint8), np.frombuffer(data, np.uint8), frames, F, info.height, info.width, rgb=bufs[0][1], alpha=bufs[1][1],
                   idx=bufs[2][1])
    rgb, alpha, idx = (_guards_intact(b[0], b[1].numel()) for b in bufs)
    assert rgb.tobytes() == ref["images"].tobytes() and alpha.tobytes() == ref["alpha"].tobytes(), name
    assert all(np.array_equal(a, b) for a, b in zip(R.frame_maps(idx, frames, F), ref["indices"])), name
    rgb2, alpha2, idx2 = rh.gif_compose(np.frombuffer(want, np.uint8), np.frombuffer(data, np.uint8), frames, F, info.height, info.width, want_idx=False)
    assert idx2 is None and rgb2.cpu().numpy().tobytes() == ref["images"].tobytes()


@pytest.mark.parametrize("name", R.malformed_names())
def test_malformed_file_gives_its_status_and_detail(rh, name):
    from roibasedimagecompression_amd import RhccqError, container
    st, dt = _decode(rh, R.case(name))[:2]
    assert (st, dt) == R.expected(name), (name, st, dt)
    with pytest.raises(RhccqError) as e:
        container.read_gif(R.case(name), rh)
    assert (e.value.status, e.value.detail) == R.expected(name) and f"RHCCQ_GIFR_{R.STATUS_NAMES[st]}" in str(e.value)


def test_device_equals_host_form_on_refused_streams(rh):
    """the status words of device form and host form agree on every malformed case (the cases above pin both to the reference)"""
    for name in R.malformed_names():
        rc, st, dt, *_ = R.host_decode(R.case(name))
        assert rc == 0 and (st, dt) == _decode(rh, R.case(name))[:2], name


def test_chains_resolved_in_order_give_the_same_pixels(rh):
    """RHCCQ_OPT_GIF_READ_CHAIN = 1 (one lane walks a segment's entries in order instead of pointer doubling): the same outputs and statuses"""
    from roibasedimagecompression_amd import RhccqError
    try:
        rh.set_option(rh.OPT_GIF_READ_CHAIN, 1)
        for name in ("m2", "flat_small", "kwkwk_4095", "last_fills", "deferred", "tile_counts", "flat_deep", "interlace_heights"):
            ref = R.reference(name)
            st, dt, rgb, alpha, maps, _ = _decode(rh, R.case(name))
            assert (st, dt) == (R.OK, 0) and np.array_equal(rgb, ref["images"]) and np.array_equal(alpha, ref["alpha"]), name
            assert all(np.array_equal(a, b) for a, b in zip(maps, ref["indices"])), name
        for name in ("bad_code_frame_1_of_3", "bad_code_large", "too_short", "far_too_long"):
            assert _decode(rh, R.case(name))[:2] == R.expected(name), name
    finally:
        rh.set_option(rh.OPT_GIF_READ_CHAIN, 0)
    with pytest.raises(RhccqError):
        rh.set_option(rh.OPT_GIF_READ_CHAIN, 2)
    assert _decode(rh, R.case("flat_small"))[:2] == (R.OK, 0)


@pytest.mark.parametrize("name", GC.names())
def test_files_of_the_device_writer_round_trip(rh, name):
    """every case of the writer, written by Rhccq.gif_encode with both dictionaries and read by read_gif: palette[indices], and for delta
    files the full frames back"""
    from roibasedimagecompression_amd import container
    v = GC.case(name)
    n, H, W = v["frames"].shape
    pal, stride, rows = GC.palette_block(name)
    local = isinstance(v["palettes"], list)
    want = GC.decoded(v["frames"], v["palettes"])
    for dictionary in ("hash", "trie"):
        out, length, _ = rh.gif_encode_async(v["frames"], n, H, W, pal, rows.tolist() if local else None, v["delays"],
                                             v["loop"], v["delta"], dictionary)
        data = rh.to_host(out[:int(length.item())]).tobytes()
        assert data == GC.reference(name)[0]
        got = container.read_gif(data, rh)
        assert got["shape"] == (H, W) and got["delays"] == v["delays"] and got["loop"] == (v["loop"] if n > 1 else None)
        assert np.array_equal(got["images"].cpu().numpy(), want), (name, dictionary)
        assert (got["alpha"].cpu().numpy() == 255).all()
        written = GC.written_pixels(v["frames"], rows[0], v["delta"]) if not local else GC.clamped(v["frames"], 1 << 30)
        for f, fr in enumerate(got["frames"]):
            assert fr["rect"] == (0, 0, W, H) and not fr["interlaced"] and fr["disposal"] == 1
            K = rows[f] if local else rows[0]
            assert np.array_equal(fr["palette"][:K], np.asarray(v["palettes"][f] if local else v["palettes"], np.uint8))
            idx = fr["indices"].cpu().numpy()
            assert np.array_equal(idx, GC.clamped(v["frames"][f], K) if local else written[f]), (name, f)
            assert fr["transparent"] == (K if v["delta"] and f > 0 else None)
        assert got["stats"]["frames"] == n and got["stats"]["segments"] >= n


@pytest.mark.parametrize("name", list(R.pillow_files()))
def test_files_pillow_writes_are_read_as_pillow_shows_them(rh, name):
    from roibasedimagecompression_amd import container
    data = R.pillow_files()[name]
    view, durations, loop = R.pillow_view(data)
    got = container.read_gif(data, rh)
    assert np.array_equal(got["images"].cpu().numpy(), view[..., :3]) and np.array_equal(got["alpha"].cpu().numpy(), view[..., 3]), name
    assert [10 * d for d in got["delays"]] == [d or 0 for d in durations] and got["loop"] == loop
    ref = R.ref_decode(data)
    assert all(np.array_equal(fr["indices"].cpu().numpy(), want) for fr, want in zip(got["frames"], ref["indices"]))
    if name == "animation":
        assert len(got["frames"]) == 4 and all(fr["rect"][2:] != (96, 64) and fr["transparent"] is not None for fr in got["frames"][1:]), "Pillow crops"
    if name.startswith("still_") and name != "still_plain_rows":
        assert got["frames"][0]["interlaced"]


@pytest.fixture(scope="module")
def three_frames(tmp_path_factory):
    """a three-frame file of a 64 x 96 crop, written by Pillow: cropped, interlaced frames, delays of 30, 70 and 110 ms, loop 5"""
    from PIL import Image
    base = R.golden_crop(64, 96, 100, 200)
    frames = [Image.fromarray(np.roll(base, 9 * f, axis=1)) for f in range(3)]
    b = io.BytesIO()
    frames[0].save(b, format="GIF", save_all=True, append_images=frames[1:], duration=[30, 70, 110], loop=5)
    path = tmp_path_factory.mktemp("gif") / "three.gif"
    path.write_bytes(b.getvalue())
    return str(path), b.getvalue()


def _same_animation(path, frames, durations, loop):
    view, d, lp = R.pillow_view(open(path, "rb").read())
    assert len(view) == frames and d == durations and lp == loop
    return view


def test_animate_takes_a_gif(rh, enc, three_frames, tmp_path):
    from roibasedimagecompression_amd import container
    path, data = three_frames
    src = container.read_gif(path, rh)
    out = str(tmp_path / "a.gif")
    res = enc.animate(path, 16, gif_path=out)
    assert res["indices"].shape == (3, 64, 96) and len(res["palette"]) <= 16
    _same_animation(out, 3, [30, 70, 110], 5)
    plain = enc.animate(src["images"], 16, delay=[3, 7, 11], loop=5)
    assert np.array_equal(plain["palette"], res["palette"]) and np.array_equal(plain["indices"].cpu().numpy(), res["indices"].cpu().numpy())
    res = enc.animate(data, 16, gif_path=out, delay=9, loop=0)                  # bytes, and the caller's own timing
    _same_animation(out, 3, [90, 90, 90], 0)


def test_reduce_gif(rh, three_frames, tmp_path):
    from roibasedimagecompression_amd import container
    path, data = three_frames
    out = str(tmp_path / "r.gif")
    res = container.reduce_gif(path, out, 8, rh, refine=2)
    assert len(res["palette"]) <= 8 and res["stats"]["read"]["frames"] == 3 and res["stats"]["gif"]["bytes"] == os.path.getsize(out)
    view = _same_animation(out, 3, [30, 70, 110], 5)
    back = container.read_gif(out, rh)
    assert np.array_equal(back["images"].cpu().numpy(), view[..., :3])
    assert np.array_equal(back["images"].cpu().numpy(), res["palette"][res["indices"].cpu().numpy()])
    assert len(np.unique(view[..., :3].reshape(-1, 3), axis=0)) <= 8


def test_command_line_takes_a_gif(rh, three_frames, tmp_path, capsys):
    from roibasedimagecompression_amd import gif
    path, _ = three_frames
    out = str(tmp_path / "c.gif")
    assert gif.main([path, out, "--colours", "12", "--no-delta"]) == 0
    stats = json.loads(capsys.readouterr().out)
    assert stats["gif"]["frames"] == 3 and stats["gif"]["colours"] <= 12 and not stats["gif"]["delta"]
    _same_animation(out, 3, [30, 70, 110], 5)
    assert gif.main([path, out, "--colours", "12", "--delay", "4", "--loop", "1"]) == 0
    capsys.readouterr()
    _same_animation(out, 3, [40, 40, 40], 1)


def test_wrapper_argument_errors(rh):
    from roibasedimagecompression_amd import ops
    data = R.case("px1")
    info, frames, blocks = ops.gif_parse(data)
    for bad in (lambda: rh.gif_unlzw(R.joined_streams(data), [frames[0]], 1), lambda: rh.gif_unlzw(R.joined_streams(data), frames, 2),
                lambda: rh.gif_compose(np.zeros(1, np.uint8), np.frombuffer(data, np.uint8), frames, 1, 0, 1),
                lambda: rh.gif_decode(data, (info, frames, blocks[:0])),
                lambda: rh.gif_decode(data, (info, frames, blocks), rgb=rh.empty((2,), __import__("torch").uint8))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ops.RhccqError):                                        # a stream buffer shorter than the frame table says
        rh.gif_unlzw(np.zeros(16, np.uint8), frames, 1)
