"""rhccq_gif_lzw_host and rhccq_gif_encode_host (csrc/gif_write.h run serially: csrc/gif_write.hip) against the dict / struct reference of
tests/gif_cases.py, byte for byte; Pillow reads every file; the bounds of rhccq_gif_sizes; argument errors of the C entries and every
ValueError of the Python layer; and the step functions once more as a stand-alone program under the host sanitizers.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import gif_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ptr = GC._ptr


def test_segment_length_and_position_function():
    from roibasedimagecompression_amd import ops
    assert ops.gif_segment_pixels() == GC.S == 16384
    assert [GC.sub_pos(o) for o in (0, 1, 254, 255, 256, 509, 510, 511)] == [1, 2, 255, 257, 258, 511, 513, 514]
    # the library's position function, seen through a file: stream byte o of the 0-mod-255 case stands at sub_pos(o) in the sub-blocks, which start behind the m byte
    data, lens = GC.reference("sub_mod0")
    rc, host, _ = GC.host_gif("sub_mod0", 1)
    at = 13 + 3 * (1 << GC.table_bits(GC.rows_of("sub_mod0")[0])) + 8 + 10      # the m byte: header, global table, extension, descriptor
    assert host[at - 10] == 0x2C and host[at] == 2
    stream = GC.reference_streams("sub_mod0")[0]
    assert len(stream) >= 510 and len(stream) % 255 == 0
    assert rc == 0 and all(host[at + 1 + GC.sub_pos(o)] == stream[o] for o in (0, 1, 254, 255, 256, 509, len(stream) - 1))
    assert host[at + 1] == 255 and host[at + 1 + GC.sub_pos(len(stream) - 1) + 1] == 0 and host[at + 1 + 256] == 255 and host[-1] == 0x3B


@pytest.mark.parametrize("name", GC.names())
def test_host_streams_equal_reference(name):
    want = GC.reference_streams(name)
    for k, eb in enumerate(GC.widths(name)):
        for shift in ((0, eb, 3 * eb) if k == 0 else (0,)):
            rc, streams = GC.host_lzw(name, eb, shift)
            assert rc == 0 and streams == want, (name, eb, shift)
    rc, streams = GC.host_lzw(name, GC.widths(name)[-1], trie=True)                 # the trie dictionary writes the same streams
    assert rc == 0 and streams == want, name


@pytest.mark.parametrize("name", GC.names())
def test_host_file_equals_reference_and_pillow_reads_it(name):
    v = GC.case(name)
    want, lengths = GC.reference(name)
    for eb in GC.widths(name):
        for trie in (False, True):
            rc, data, lens = GC.host_gif(name, eb, eb, trie)
            assert rc == 0 and lens == lengths and data == want, (name, eb, trie)
    n = len(v["frames"])
    parsed = GC.parse(want)
    local = isinstance(v["palettes"], list)
    assert len(parsed["frames"]) == n and (parsed["global"] == 0) == local and all((f["local"] != 0) == local for f in parsed["frames"])
    assert parsed["loop"] == (v["loop"] if n > 1 else None) and [f["delay"] for f in parsed["frames"]] == v["delays"]
    K = GC.rows_of(name)[0]
    assert [f["transparent"] for f in parsed["frames"]] == [None] + [K if v["delta"] else None] * (n - 1)
    frames, durations, loop = GC.pillow_frames(want)
    assert frames.shape[0] == n and np.array_equal(frames, GC.decoded(v["frames"], v["palettes"])), name
    assert durations == [10 * d for d in v["delays"]] and loop == (v["loop"] if n > 1 else None)


def test_sizes_bound_the_noise_cases():
    for name in ("noise_full", "k256", "k255", "last_fills", "clamp_wide", "delta_k255", "local_mixed"):
        v = GC.case(name)
        n, H, W = v["frames"].shape
        rc, ws, stream, bound = GC.sizes(n, H, W, GC.flags_of(name))
        data, lengths = GC.reference(name)
        assert rc == 0 and max(lengths) <= stream and len(data) <= bound and ws >= 4 * n * ((H * W + GC.S - 1) // GC.S)
        assert stream >= (12 * H * W + 7) // 8                                 # a 12-bit code a pixel is possible
    # (host_gif and host_lzw assert that bytes behind the file and behind every stream stay untouched)
    lib = GC.lib()
    assert lib.rhccq_gif_sizes(3, 5, 7, 0, None, None, None) == 0                # any of the three may be NULL


def test_argument_errors_and_limits():
    lib = GC.lib()
    idx = np.zeros((2, 2, 3), np.uint32)
    pal = np.zeros((5, 3), np.uint8)
    rows, delays = np.array([5], np.int32), np.array([1, 2], np.int32)
    out, streams = np.zeros(4096, np.uint8), np.zeros((2, 64), np.uint8)
    n, lens = C.c_int64(), np.zeros(2, np.int64)

    def lzw(i=idx, eb=4, n=2, H=2, W=3, k=rows, flags=0, o=streams, stride=64, ln=lens):
        return lib.rhccq_gif_lzw_host(_ptr(i), eb, n, H, W, _ptr(k), flags, _ptr(o), stride, _ptr(ln))

    def encode(i=idx, eb=4, n=2, H=2, W=3, p=pal, ks=5, k=rows, d=delays, loop=0, flags=0, o=out, cap=4096, ln=n):
        return lib.rhccq_gif_encode_host(_ptr(i), eb, n, H, W, _ptr(p), ks, _ptr(k), _ptr(d), loop, flags, _ptr(o), cap, C.byref(ln) if ln is not None else None,
                                         None)

    assert lzw() == 0 and encode() == 0
    for call in (lzw, encode):
        assert call(n=0) == GC.E_ARG and call(n=-1) == GC.E_ARG and call(n=(1 << 20) + 1) == GC.E_ARG
        assert call(H=0) == GC.E_ARG and call(W=0) == GC.E_ARG and call(H=65536) == GC.E_ARG and call(W=65536) == GC.E_ARG
        assert call(eb=3) == GC.E_ARG and call(eb=8) == GC.E_ARG
        assert call(flags=8) == GC.E_ARG and call(flags=-1) == GC.E_ARG and call(flags=GC.LOCAL | GC.DELTA) == GC.E_ARG
        assert call(i=None) == GC.E_ARG and call(k=None) == GC.E_ARG and call(o=None) == GC.E_ARG and call(ln=None) == GC.E_ARG
        assert call(k=np.array([0], np.int32)) == GC.E_ARG and call(k=np.array([257], np.int32)) == GC.E_ARG
        assert call(k=np.array([5, 0], np.int32), flags=GC.LOCAL) == GC.E_ARG
        assert call(i=idx.view(np.uint8).reshape(-1)[1:], eb=2) == GC.E_ARG                  # not aligned to its element
    big = np.zeros((256, 3), np.uint8)
    assert encode(p=big, ks=256, k=np.array([256], np.int32), flags=GC.DELTA) == GC.E_ARG and lzw(k=np.array([256], np.int32), flags=GC.DELTA) == GC.E_ARG
    assert encode(p=big, ks=256, k=np.array([255], np.int32), flags=GC.DELTA) == 0 and encode(p=big, ks=256, k=np.array([256], np.int32)) == 0
    assert encode(p=None) == GC.E_ARG and encode(ks=0) == GC.E_ARG and encode(ks=257) == GC.E_ARG and encode(ks=4) == GC.E_ARG
    assert encode(d=None) == GC.E_ARG and encode(d=np.array([1, -1], np.int32)) == GC.E_ARG and encode(d=np.array([65536, 0], np.int32)) == GC.E_ARG
    assert encode(loop=-1) == GC.E_ARG and encode(loop=65536) == GC.E_ARG and encode(loop=65535) == 0
    rc, _, stream, bound = GC.sizes(2, 2, 3, 0)
    assert rc == 0 and encode(cap=bound) == 0 and encode(cap=bound - 1) == GC.E_LIMIT
    assert lzw(stride=stream) == 0 and lzw(stride=stream - 1) == GC.E_LIMIT
    s = C.c_int64()
    assert lib.rhccq_gif_sizes(0, 2, 3, 0, C.byref(s), None, None) == GC.E_ARG and lib.rhccq_gif_sizes(1, 0, 3, 0, C.byref(s), None, None) == GC.E_ARG
    assert lib.rhccq_gif_sizes(1, 2, 65536, 0, C.byref(s), None, None) == GC.E_ARG and lib.rhccq_gif_sizes(1, 2, 3, 8, C.byref(s), None, None) == GC.E_ARG
    assert lib.rhccq_gif_sizes(1, 2, 3, GC.LOCAL | GC.DELTA, C.byref(s), None, None) == GC.E_ARG
    assert lib.rhccq_gif_sizes(1, 40000, 40000, 0, C.byref(s), None, None) == GC.E_LIMIT             # a file of 2 GiB or more
    assert lib.rhccq_gif_sizes(1 << 20, 64, 64, 0, C.byref(s), None, None) == GC.E_LIMIT
    assert lib.rhccq_gif_sizes(1, 16384, 16384, 0, C.byref(s), None, None) == 0 and s.value > 0
    assert lib.rhccq_abi_version() == 1


def test_device_forms_refuse_a_null_context():
    lib = GC.lib()
    assert lib.rhccq_gif_lzw(None, None, 1, 1, 1, 1, None, 0, None, None, 0, None) == GC.E_ARG
    assert lib.rhccq_gif_encode(None, None, 1, 1, 1, 1, None, 1, None, None, 0, 0, None, None, 0, None) == GC.E_ARG


def _res(K=4, shape=(2, 3), seed=0):
    rng = np.random.default_rng(seed)
    return {"palette": rng.integers(0, 256, (K, 3)).astype(np.uint8), "indices": rng.integers(0, K, shape[0] * shape[1]).astype(np.uint8), "shape": shape}


def test_write_gif_value_errors_come_before_the_device():
    from roibasedimagecompression_amd import RhccqError, container
    cases = (([_res(), _res(shape=(3, 2))], {}, "write_gif: every frame must have the same shape"),
             ([_res(shape=(1, 65536))], {}, "write_gif: a GIF frame is at most 65535 x 65535"),
             ([_res(shape=(65536, 1))], {}, "write_gif: a GIF frame is at most 65535 x 65535"),
             ([_res(K=257)], {}, "write_gif: a GIF colour table has at most 256 rows"),
             ([_res(), _res(seed=1)], {"delta": True}, "write_gif: delta needs one palette for all frames (a global colour table)"),
             ([_res(K=256), _res(K=256)], {"delta": True},
              "write_gif: delta needs a palette of at most 255 rows (the transparent index is one more entry)"))
    for results, kw, text in cases:
        for call in (container.gif_bytes, container.gif_file, lambda r, **k: container.write_gif(r, os.devnull, **k)):
            with pytest.raises(ValueError) as e:
                call(results, **kw)
            assert str(e.value) == text
    for bad in ({"palette": [[0, 0, 0]]}, [], [1, 2, 3], "x"):
        with pytest.raises(RhccqError):
            container.gif_bytes(bad)


def test_encoder_keywords_are_validated_without_a_device():
    from roibasedimagecompression_amd.image import ImageEncoder
    enc = ImageEncoder.__new__(ImageEncoder)                                  # (no context: the checks come first)
    enc.rh = None
    img, pal = np.zeros((4, 4, 3), np.uint8), np.zeros((1, 3), np.uint8)
    for fn, call in (("encode_with_palette", lambda p: enc.encode_with_palette(img, pal, gif_path=p)),
                     ("quantize", lambda p: enc.quantize(img, 2, gif_path=p)),
                     ("encode", lambda p: enc.encode(img, gif_path=p)),
                     ("quantize_batch", lambda p: enc.quantize_batch([img], 2, gif_path=p)),
                     ("animate", lambda p: enc.animate([img], 2, gif_path=p))):
        with pytest.raises(TypeError) as e:
            call(5)
        assert str(e.value) == f"ImageEncoder.{fn}: gif_path must be a file name, got int"
        with pytest.raises(ValueError) as e:
            call("")
        assert str(e.value) == f"ImageEncoder.{fn}: gif_path must not be empty"
    with pytest.raises(ValueError) as e:
        enc.quantize(img, 257, gif_path="x.gif")
    assert str(e.value) == "ImageEncoder.quantize: gif_path needs colours <= 256 (a GIF colour table has at most 256 rows)"
    with pytest.raises(ValueError) as e:
        enc.quantize_batch([img], 257, gif_path="x.gif")
    assert str(e.value) == "ImageEncoder.quantize_batch: gif_path needs colours <= 256 (a GIF colour table has at most 256 rows)"
    for colours in (0, 257):
        with pytest.raises(ValueError) as e:
            enc.animate([img], colours)
        assert str(e.value) == "ImageEncoder.animate: colours must be 1..256 (a GIF colour table has at most 256 rows)"
    with pytest.raises(ValueError) as e:
        enc.animate([img], 16, refine=65)
    assert str(e.value) == "ImageEncoder.animate: refine must be 0..64"


def test_command_line_arguments():
    from roibasedimagecompression_amd import gif
    args = gif.parser().parse_args(["a.png", "b.png", "o.gif", "--colours", "32", "--delay", "7", "--loop", "2", "--no-delta", "--pattern", "100"])
    assert args.files == ["a.png", "b.png", "o.gif"] and args.colours == 32 and args.delay == 7 and args.loop == 2 and args.no_delta
    assert args.pattern == 100 and args.pattern_size == 4 and args.refine == 0
    for bad in (["o.gif", "--colours", "4"], ["a.png", "o.gif"]):
        with pytest.raises(SystemExit):
            gif.main(bad)


def test_device_entry_point_raises_without_a_gpu():
    """no CPU fallback: container.gif_bytes needs the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError, container
    res = _res()
    if torch.cuda.is_available():
        idx = res["indices"].reshape((1,) + res["shape"])
        assert container.gif_bytes(res) == GC.gif_reference(idx, res["palette"], [4])[0]
    else:
        with pytest.raises(RhccqError):
            container.gif_bytes(res)


def test_step_functions_under_the_host_sanitizers(tmp_path):
    """tests/native/gif_write_host_test.cpp: csrc/gif_write.h needs no HIP.  The corpus is every case; the program encodes each from the
    header's step functions into buffers of exactly the promised sizes and compares with the reference's file."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on this machine")
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    names = GC.write_corpus(str(corpus))
    (corpus / "manifest").write_text("\n".join(names) + "\n")
    exe = tmp_path / "gif_write_host_test"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "roibasedimagecompression_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "gif_write_host_test.cpp"), "-o", str(exe)]
    c = subprocess.run(cmd, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == f"gif_write_host ok {len(names)}", (r.returncode, r.stdout, r.stderr)
