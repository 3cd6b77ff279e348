"""rhccq_png_scanlines_host, rhccq_crc32_host and rhccq_png_encode_host (csrc/png_write.h run serially: csrc/png_write.hip) against the
numpy / struct / zlib reference of tests/png_cases.py, bit for bit; Pillow reads every file; argument errors, limits, the bounds of
rhccq_png_sizes and the keyword's validation in ImageEncoder.  No GPU."""
import ctypes as C
import zlib

import numpy as np
import pytest

import png_cases as PC

_ptr = PC._ptr


def widths(name):
    return [eb for eb in PC.index_widths(len(PC.case(name)[1])) if PC.storable(name, eb)]


@pytest.mark.parametrize("name", PC.names())
def test_host_scanlines_equal_reference(name):
    idx, pal, _, _ = PC.case(name)
    want_scan, want_rows, _ = PC.reference(name)
    assert widths(name)
    for eb in widths(name):
        rc, scan, rows = PC.host_scanlines(idx, pal, PC.flags_of(name, exact=False), eb)
        assert rc == 0, (name, eb)
        assert np.array_equal(scan, want_scan), (name, eb)
        assert np.array_equal(rows, want_rows), (name, eb)


@pytest.mark.parametrize("n", PC.CRC_LENGTHS + (PC.CRC_LONG,))
def test_host_crc32_equals_zlib(n):
    a = PC.crc_bytes(n)
    rc, crc = PC.host_crc32(a)
    assert rc == 0 and crc == zlib.crc32(a.tobytes())


def test_host_crc32_known_values():
    assert PC.host_crc32(np.frombuffer(b"123456789", np.uint8)) == (0, 0xCBF43926)          # the check value of CRC-32
    assert PC.host_crc32(np.frombuffer(b"IEND", np.uint8)) == (0, 0xAE426082)
    assert PC.host_crc32(np.zeros(0, np.uint8)) == (0, 0)


@pytest.mark.parametrize("name", PC.names())
def test_host_file_equals_reference_and_pillow_reads_it(name):
    idx, pal, depth8, flt = PC.case(name)
    K = len(pal)
    scan = PC.reference(name)[0].tobytes()
    want = PC.png_reference(idx, pal, depth8, flt, stream=zlib.compress(scan, 9))         # (zlib compared live)
    for eb in widths(name):
        rc, data = PC.host_png(idx, pal, PC.flags_of(name), eb)
        assert rc == 0 and data == want, (name, eb)
    kinds = [c[0] for c in PC.chunks(want)]
    assert kinds == ([b"IHDR", b"PLTE", b"IDAT", b"IEND"] if K <= 256 else [b"IHDR", b"IDAT", b"IEND"])
    assert all(stored == crc for _, _, stored, crc in PC.chunks(want))
    mode, img, plte = PC.pillow_image(want)
    assert mode == ("P" if K <= 256 else "RGB")
    assert np.array_equal(img, PC.decoded(idx, pal)), name
    if K <= 256:
        assert np.array_equal(plte, pal)                                                    # exactly K entries


def test_rgb_bands_use_every_filter_and_flat_takes_type_0():
    idx, pal, _, _ = PC.case("rgb_bands")
    rc, scan, rows = PC.host_scanlines(idx, pal, 0, 2)
    assert rc == 0 and (rows > 0).all() and rows.sum() == 40
    assert set(scan.reshape(40, -1)[:, 0].tolist()) == {0, 1, 2, 3, 4}
    rc, scan, rows = PC.host_scanlines(idx, pal, PC.NO_FILTER, 2)
    assert rc == 0 and rows.tolist() == [40, 0, 0, 0, 0] and not scan.reshape(40, -1)[:, 0].any()
    idx, pal, _, _ = PC.case("rgb_flat")
    rc, scan, rows = PC.host_scanlines(idx, pal, 0, 2)
    assert rc == 0 and rows.tolist() == [6, 0, 0, 0, 0]


def test_sizes_hold_on_every_case():
    for name in PC.names():
        idx, pal, depth8, _ = PC.case(name)
        H, W = idx.shape
        K = len(pal)
        for exact in (False, True):
            rc, scan, work, bound = PC.sizes(H, W, K, PC.flags_of(name, exact))
            assert rc == 0
            d = PC.depth_of(K, depth8)
            assert scan == len(PC.reference(name)[0]) == H * (1 + ((W * d + 7) // 8 if K <= 256 else 3 * W))
            assert work >= scan and bound >= len(PC.reference_file(name))
            assert bound >= 8 + 25 + (12 + 3 * K if K <= 256 else 0) + 12 + len(zlib.compress(PC.reference(name)[0].tobytes(), 0)) + 12
    lib = PC.lib()
    assert lib.rhccq_png_sizes(3, 5, 7, 0, None, None, None) == 0                           # any of the three may be NULL
    assert lib.rhccq_crc32_bytes(0) >= 4 and lib.rhccq_crc32_bytes(-1) == PC.E_ARG
    assert lib.rhccq_crc32_bytes(1 << 20) >= 4 * ((1 << 20) // PC.CRC_PIECE + 1)


def test_argument_errors_and_limits():
    lib = PC.lib()
    idx = np.zeros((2, 3), np.uint32)
    pal = np.zeros((5, 3), np.uint8)
    scan = np.zeros(64, np.uint8)
    out = np.zeros(4096, np.uint8)
    n = C.c_int64()
    s = C.c_int64()

    def scanlines(i=idx, eb=4, H=2, W=3, p=pal, K=5, flags=0, o=scan):
        return lib.rhccq_png_scanlines_host(_ptr(i), eb, H, W, _ptr(p), K, flags, _ptr(o), None)

    def encode(i=idx, eb=4, H=2, W=3, p=pal, K=5, flags=PC.EXACT, o=out, cap=4096, ln=n):
        return lib.rhccq_png_encode_host(_ptr(i), eb, H, W, _ptr(p), K, flags, _ptr(o), cap, C.byref(ln) if ln is not None else None)

    assert scanlines() == 0 and encode() == 0
    for call in (scanlines, encode):
        assert call(H=0) == PC.E_ARG and call(W=0) == PC.E_ARG and call(H=-1) == PC.E_ARG
        assert call(K=0) == PC.E_ARG and call(K=65537) == PC.E_ARG
        assert call(eb=3) == PC.E_ARG and call(eb=8) == PC.E_ARG
        assert call(flags=8) == PC.E_ARG and call(flags=-1) == PC.E_ARG
        assert call(i=None) == PC.E_ARG and call(p=None) == PC.E_ARG and call(o=None) == PC.E_ARG
    assert encode(flags=0) == PC.E_ARG and encode(flags=PC.DEPTH8) == PC.E_ARG                # the fast encoder has no host form
    assert encode(ln=None) == PC.E_ARG
    rc, _, _, bound = PC.sizes(2, 3, 5, PC.EXACT)
    assert rc == 0 and encode(cap=bound) == 0 and encode(cap=bound - 1) == PC.E_LIMIT
    for flags in (0, PC.EXACT, PC.NO_FILTER):
        assert lib.rhccq_png_sizes(0, 3, 5, flags, C.byref(s), None, None) == PC.E_ARG
        assert lib.rhccq_png_sizes(2, 3, 0, flags, C.byref(s), None, None) == PC.E_ARG
        assert lib.rhccq_png_sizes(2, 3, 5, flags | 8, C.byref(s), None, None) == PC.E_ARG
        # scanlines of 2 GiB or more: both encoders refuse them (colour type 3 at depth 8, colour type 2, a packed depth)
        assert lib.rhccq_png_sizes(1 << 16, 1 << 15, 256, flags, C.byref(s), None, None) == PC.E_LIMIT
        assert lib.rhccq_png_sizes(1 << 15, 1 << 15, 300, flags, C.byref(s), None, None) == PC.E_LIMIT
        assert lib.rhccq_png_sizes(1 << 17, 1 << 17, 2, flags, C.byref(s), None, None) == PC.E_LIMIT
        assert lib.rhccq_png_sizes(1 << 15, 1 << 15, 256, flags, C.byref(s), None, None) == 0 and s.value == (1 << 15) * ((1 << 15) + 1)
    assert lib.rhccq_png_scanlines_host(_ptr(idx), 4, 1 << 16, 1 << 15, _ptr(pal), 5, PC.DEPTH8, _ptr(scan), None) == PC.E_LIMIT
    crc = C.c_uint32()
    assert lib.rhccq_crc32_host(None, 1, C.byref(crc)) == PC.E_ARG and lib.rhccq_crc32_host(_ptr(scan), -1, C.byref(crc)) == PC.E_ARG
    assert lib.rhccq_crc32_host(_ptr(scan), 4, None) == PC.E_ARG
    assert lib.rhccq_abi_version() == 1


def test_device_forms_refuse_a_null_context():
    lib = PC.lib()
    assert lib.rhccq_png_scanlines(None, None, 1, 1, 1, None, 1, 0, None, None) == PC.E_ARG
    assert lib.rhccq_crc32(None, None, 0, None, None, None) == PC.E_ARG
    assert lib.rhccq_png_encode(None, None, 1, 1, 1, None, 1, 0, None, None, 0, None) == PC.E_ARG


def test_index_map_argument_layer():
    """_palette_args.index_map: the dtypes container._index_tensor accepts, no device needed"""
    import torch
    from roibasedimagecompression_amd import _palette_args as A
    fn = "png_encode"
    assert A.index_map(np.zeros((2, 3), np.uint8), 2, 3, "cpu", fn).dtype == torch.uint8
    t = A.index_map(np.array([[65535, 1]], np.uint16), 1, 2, "cpu", fn)
    assert t.dtype == torch.int16 and t.tolist() == [-1, 1]
    assert A.index_map(np.zeros((2, 3), np.int64), 2, 3, "cpu", fn).dtype == torch.int32
    assert A.index_map(torch.zeros(6, dtype=torch.int64), 2, 3, "cpu", fn).dtype == torch.int32
    assert A.index_map([[1, 2, 3]], 1, 3, "cpu", fn).tolist() == [1, 2, 3]
    with pytest.raises(TypeError) as e:
        A.index_map(np.zeros((2, 3), np.float32), 2, 3, "cpu", fn)
    assert str(e.value).startswith("png_encode: indices must be integers")
    with pytest.raises(TypeError):
        A.index_map(torch.zeros(6, dtype=torch.float32), 2, 3, "cpu", fn)
    with pytest.raises(ValueError) as e:
        A.index_map(np.zeros((2, 3), np.uint8), 2, 4, "cpu", fn)
    assert str(e.value) == "png_encode: indices must have H * W elements"


def test_png_path_is_validated_without_a_device():
    from roibasedimagecompression_amd.image import ImageEncoder
    enc = ImageEncoder.__new__(ImageEncoder)                                  # (no context: the checks come first)
    enc.rh = None
    img, pal = np.zeros((4, 4, 3), np.uint8), np.zeros((1, 3), np.uint8)
    for fn, call in (("encode_with_palette", lambda p: enc.encode_with_palette(img, pal, png_path=p)),
                     ("quantize", lambda p: enc.quantize(img, 2, png_path=p)),
                     ("encode", lambda p: enc.encode(img, png_path=p))):
        with pytest.raises(TypeError) as e:
            call(5)
        assert str(e.value) == f"ImageEncoder.{fn}: png_path must be a file name, got int"
        with pytest.raises(ValueError) as e:
            call("")
        assert str(e.value) == f"ImageEncoder.{fn}: png_path must not be empty"
    assert ImageEncoder._png_arg("ImageEncoder.encode", None) is None


def test_write_png_refuses_what_write_frame_refuses():
    from roibasedimagecompression_amd import RhccqError, container
    with pytest.raises(RhccqError) as e:
        container.png_bytes({"palette": [[0, 0, 0]]})
    assert str(e.value) == "write_png: a FrameEncoder result (palette, indices, shape) is required"
    with pytest.raises(RhccqError):
        container.write_png([1, 2, 3], "x.png")


def test_device_entry_point_raises_without_a_gpu():
    """no CPU fallback: container.png_bytes needs the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError, container
    res = {"palette": np.array([[1, 2, 3], [4, 5, 6]], np.uint8), "indices": np.array([0, 1, 1, 0], np.uint8), "shape": (2, 2)}
    if torch.cuda.is_available():
        data = container.png_bytes(res, exact=True)
        assert data == PC.png_reference(np.array([[0, 1], [1, 0]]), res["palette"])
    else:
        with pytest.raises(RhccqError):
            container.png_bytes(res)
