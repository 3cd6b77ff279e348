"""rhccq_palette_pattern_host (the device kernel's step functions run serially: csrc/palette_pattern.h, csrc/palette_pattern.hip) against
the numpy reference of tests/pattern_cases.py, bit for bit: indices in every element width, the three sum columns, the batched host form,
argument errors, the exported constants, the keyword's validation in ImageEncoder, and the value claims from the references alone.
No GPU."""
import numpy as np
import pytest

import dither_cases as DC
import pattern_cases as PC
import remap_cases as RM

host_pattern, _ptr = PC.host_pattern, PC._ptr


def test_constants_are_exported():
    from roibasedimagecompression_amd import _lib, ops
    lib = _lib.load()
    assert ops.PATTERN_MAX == PC.MAX_STRENGTH == 256
    assert ops.PATTERN_SIZES == PC.SIZES == (2, 4, 8)
    assert ops.palette_pattern_max_rows() == lib.rhccq_palette_pattern_max_rows() == PC.MAX_ROWS == 4096
    assert lib.rhccq_abi_version() == 1


def test_bayer_matrices():
    assert PC.bayer(2).tolist() == [[0, 2], [3, 1]]
    assert PC.bayer(4).tolist() == [[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]]
    for n in PC.SIZES:
        assert sorted(PC.bayer(n).reshape(-1).tolist()) == list(range(n * n))


@pytest.mark.parametrize("name", PC.names())
def test_host_equals_reference(name):
    rgb, pal, cls, nc, strength, size, _ = PC.case(name)
    want_out, want_sums, _, _ = PC.reference(name)
    for eb in PC.index_bytes(len(pal)):
        rc, out, sums = host_pattern(rgb, pal, cls, nc, strength, size, eb)
        assert rc == 0, (name, eb)
        assert np.array_equal(out, want_out), (name, eb)
        assert np.array_equal(sums, want_sums), (name, eb)


@pytest.mark.parametrize("name", ["shape1x3", "edge9x9", "luma_tie", "classes2", "classes16", "strength128_n2", "strength128_n8"])
def test_host_properties(name):
    """what the definition implies: the pixel counts are the remap's; moved is the pixels off the remap's index; a pixel of a strength-0
    class keeps the remap's index; strength 0 everywhere is the remap for every size, indices and squared error"""
    rgb, pal, cls, nc, strength, size, _ = PC.case(name)
    table = PC.strength_table(strength, nc)
    rc, out, sums = host_pattern(rgb, pal, cls, nc, strength, size, 4)
    assert rc == 0
    b, base = RM.remap_reference(rgb, pal, cls, nc)
    H, W = rgb.shape[:2]
    b = b.reshape(H, W)
    assert np.array_equal(sums[:, 0], base[:, 0]) and sums[-1, 0] == H * W
    assert sums[-1, 2] == int((out != b).sum())
    c = np.full((H, W), nc, np.int64) if cls is None else np.minimum(np.asarray(cls, np.int64).reshape(H, W), nc)
    still = np.asarray(table)[c] == 0
    assert np.array_equal(out[still], b[still])
    for n in PC.SIZES:
        rc, out0, sums0 = host_pattern(rgb, pal, cls, nc, 0, n, 4)
        assert rc == 0 and np.array_equal(out0, b) and np.array_equal(sums0[:, :2], base) and (sums0[:, 2] == 0).all()


def test_floor_and_tie_cases_by_hand():
    rgb, pal, _, _, strength, size, expect = PC.case("floor")
    rc, out, sums = host_pattern(rgb, pal, None, 0, strength, size, 1)
    assert rc == 0 and out.tolist() == expect == [[1, 0], [0, 1]]
    assert sums.tolist() == [[4, 4 * 4, 2]]


def test_position_only_on_the_host():
    """the same pixels at the same (y mod n, x mod n) in another picture get the same index"""
    rng = np.random.default_rng(5)
    pal = RM._palette(rng, 23)
    for n in PC.SIZES:
        big = PC._image(rng, 3 * n + 1, 4 * n + 3)
        rc, whole, _ = host_pattern(big, pal, None, 0, 256, n, 1)
        part = np.ascontiguousarray(big[n:2 * n + 1, 2 * n:])
        rc2, got, _ = host_pattern(part, pal, None, 0, 256, n, 1)
        assert rc == 0 and rc2 == 0 and np.array_equal(got, whole[n:2 * n + 1, 2 * n:]), n


@pytest.mark.parametrize("what,over,code", PC.ERRORS, ids=[e[0] for e in PC.ERRORS])
def test_host_argument_errors(what, over, code):
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    rgb, pal = np.zeros((4, 3), np.uint8), np.zeros((3, 3), np.uint8)
    cls = np.zeros(4, np.uint8) if over.get("cls") else None
    idx, sums = np.zeros(4, np.uint32), np.zeros((18, 3), np.uint64)
    strength = over.get("strength", [5])
    table = None if strength is None else np.array(strength, np.uint32)
    a = {"rgb": rgb, "palette": pal, "idx_out": idx, "sums": sums}
    a.update({k: v for k, v in over.items() if k in a})
    rc = lib.rhccq_palette_pattern_host(_ptr(a["rgb"]), over.get("H", 2), over.get("W", 2), _ptr(a["palette"]), over.get("K", 3), _ptr(cls),
                                        over.get("n_classes", 0), _ptr(table), over.get("size", 4), _ptr(a["idx_out"]), over.get("idx_elem_bytes", 2),
                                        _ptr(a["sums"]))
    assert rc == code, what


def test_host_accepts_the_valid_call_the_errors_vary():
    """the call every error case changes one argument of succeeds, with and without its class map, for every size; no pixels: zero sums"""
    for n in PC.SIZES:
        rc, out, sums = host_pattern(np.zeros((2, 2, 3), np.uint8), np.zeros((3, 3), np.uint8), None, 0, [5], n, 2)
        assert rc == 0 and out.tolist() == [[0, 0], [0, 0]] and sums.tolist() == [[4, 0, 0]]
    rc, out, sums = host_pattern(np.zeros((2, 2, 3), np.uint8), np.zeros((3, 3), np.uint8), np.array([0, 1, 255, 1], np.uint8), 2, [0, PC.MAX_STRENGTH, 5], 4, 2)
    assert rc == 0 and sums.tolist() == [[1, 0, 0], [2, 0, 0], [4, 0, 0]]
    for h, w in ((0, 0), (0, 5), (5, 0)):
        rc, out, sums = host_pattern(np.zeros((h, w, 3), np.uint8), np.zeros((3, 3), np.uint8), None, 0, [5], 4, 1)
        assert rc == 0 and sums.tolist() == [[0, 0, 0]], (h, w)


def test_host_takes_palettes_above_the_device_cap():
    """the host form has no LDS to fit: 4097 rows (the device form refuses them) against the reference"""
    rng = np.random.default_rng(7)
    pal = RM._palette(rng, 4097)
    rgb = PC._image(rng, 5, 9)
    want, want_sums, _, _ = PC.pattern_reference(rgb, pal, 256, 4)
    rc, out, sums = host_pattern(rgb, pal, None, 0, 256, 4, 2)
    assert rc == 0 and np.array_equal(out, want) and np.array_equal(sums, want_sums)


def _batch_host(frames, pals, rows, cls, nc, strength, size, eb, widths=None):
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    B = len(frames)
    off = np.concatenate([[0], np.cumsum([f.shape[0] * f.shape[1] for f in frames])]).astype(np.int64)
    rgb = np.ascontiguousarray(np.concatenate([f.reshape(-1, 3) for f in frames]))
    wid = np.array([f.shape[1] for f in frames] if widths is None else widths, np.int32)
    stride = max(len(p) for p in pals)
    palettes = np.zeros((B, stride, 3), np.uint8)
    for i, p in enumerate(pals):
        palettes[i, :len(p)] = p
    k_rows = np.array(rows, np.int32)
    table = np.array(PC.strength_table(strength, nc), np.uint32)
    idx = np.full(max(int(off[-1]), 1), 0xAB, PC._DT[eb])
    sums = np.full((B, nc + 1, 3), 0x5555, np.uint64)
    rc = lib.rhccq_palette_pattern_batch_host(_ptr(rgb), _ptr(off), _ptr(wid), B, _ptr(palettes), stride, _ptr(k_rows), _ptr(cls), nc, _ptr(table), size,
                                              _ptr(idx), eb, _ptr(sums))
    return rc, idx[:int(off[-1])].astype(np.int64), sums.astype(np.int64), off


def test_batch_host_equals_the_single_calls():
    """three pictures of different sizes and palettes, one of them without rows: every image is what the single call gives for it alone"""
    rng = np.random.default_rng(11)
    frames = [PC._image(rng, 5, 7), PC._image(rng, 9, 4), PC._image(rng, 3, 11), PC._image(rng, 0, 6)]
    pals = [RM._palette(rng, 5), RM._palette(rng, 17), RM._palette(rng, 9), RM._palette(rng, 3)]
    cls = rng.integers(0, 3, sum(f.shape[0] * f.shape[1] for f in frames)).astype(np.uint8)
    for size in PC.SIZES:
        rc, idx, sums, off = _batch_host(frames, pals, [5, 17, 0, 3], cls, 2, [256, 0, 77], size, 1)
        assert rc == 0
        for i, (f, p) in enumerate(zip(frames, pals)):
            got = idx[off[i]:off[i + 1]].reshape(f.shape[:2])
            if i == 2:                                                       # no rows: index 0 and zero sums
                assert not got.any() and not sums[i].any()
                continue
            want, want_sums, _, _ = PC.pattern_reference(f, p, [256, 0, 77], size, cls[off[i]:off[i + 1]], 2)
            assert np.array_equal(got, want) and np.array_equal(sums[i], want_sums), (size, i)
    # a width that does not divide its image, a negative one, a size that is none of the three
    assert _batch_host(frames, pals, [5, 17, 9, 3], cls, 2, 256, 4, 1, widths=[7, 5, 11, 6])[0] == PC.E_ARG
    assert _batch_host(frames, pals, [5, 17, 9, 3], cls, 2, 256, 4, 1, widths=[7, 4, 11, -1])[0] == PC.E_ARG
    assert _batch_host(frames, pals, [5, 17, 9, 3], cls, 2, 256, 5, 1)[0] == PC.E_ARG
    assert _batch_host(frames, pals, [5, 17, 9, 3], cls, 2, 257, 4, 1)[0] == PC.E_ARG


def test_image_encoder_validates_pattern():
    from roibasedimagecompression_amd.image import ImageEncoder
    fn = "ImageEncoder.encode_with_palette"
    args = ImageEncoder._runs_args
    assert args(fn, None, None, False, None, dither=None, pattern=None) is None
    assert args(fn, None, None, False, pattern=0) == {"pattern": 0, "size": 4, "nonroi": 0, "roi": 0}
    assert args(fn, None, None, False, pattern=256, pattern_size=8) == {"pattern": 256, "size": 8, "nonroi": 256, "roi": 256}
    given = {"roi": 0, "nonroi": 200}
    assert args(fn, None, None, True, pattern=given, pattern_size=2) == {"pattern": given, "size": 2, "nonroi": 200, "roi": 0}
    assert args(fn, 5, None, False) == {"slack": 5, "nonroi": 5, "roi": 5}                # (the positional calls are what they were)
    assert args(fn, None, None, False, dither=7, pattern_size=3) == {"dither": 7, "nonroi": 7, "roi": 7}    # (the size is the pattern's alone)
    for slack, penalty in ((5, None), (None, 5)):
        with pytest.raises(ValueError) as e:
            args(fn, slack, penalty, False, pattern=1)
        assert str(e.value) == f"{fn}: pattern is exclusive with run_slack and run_penalty"
    with pytest.raises(ValueError) as e:
        args(fn, None, None, False, dither=1, pattern=1)
    assert str(e.value) == f"{fn}: pattern and dither are exclusive"
    with pytest.raises(ValueError) as e:
        args(fn, None, None, False, 30.0, pattern=0)
    assert str(e.value) == f"{fn}: pattern cannot be combined with target_psnr"
    for bad in (0, 1, 3, 16, None, True):
        with pytest.raises(ValueError) as e:
            args(fn, None, None, False, pattern=1, pattern_size=bad)
        assert str(e.value) == f"{fn}: pattern_size must be 2, 4 or 8"
    for bad in (-1, 257, {"roi": 257, "nonroi": 0}, {"roi": 0, "nonroi": -1}):
        with pytest.raises(ValueError) as e:
            args(fn, None, None, True, pattern=bad)
        assert str(e.value) == f"{fn}: a pattern must be 0..256"
    with pytest.raises(ValueError) as e:
        args(fn, None, None, False, pattern=given)
    assert str(e.value) == f"{fn}: a roi / nonroi pattern needs roi_mask"
    with pytest.raises(ValueError) as e:
        args(fn, None, None, True, pattern={"roi": 1})
    assert str(e.value) == f'{fn}: pattern is a number or a dict over "roi" and "nonroi"'
    # the messages that were there stay word for word
    with pytest.raises(ValueError) as e:
        args(fn, 5, None, False, dither=1)
    assert str(e.value) == f"{fn}: dither is exclusive with run_slack and run_penalty"
    with pytest.raises(ValueError) as e:
        args(fn, 5, 5, False)
    assert str(e.value) == f"{fn}: run_slack and run_penalty are exclusive"


def test_sequence_refuses_before_it_touches_the_device():
    """the refusals of encode_sequence fire before any device work"""
    from roibasedimagecompression_amd.image import ImageEncoder
    enc = ImageEncoder.__new__(ImageEncoder)                                  # (no context: the checks come first)
    enc.rh = None
    frames = [np.zeros((4, 4, 3), np.uint8)]
    with pytest.raises(ValueError) as e:
        next(enc.encode_sequence(frames, 20, 10, 1.0, pattern={"roi": 1, "nonroi": 2}))
    assert str(e.value) == "ImageEncoder.encode_sequence: pattern is one number (a remapped frame has no region map)"
    with pytest.raises(ValueError) as e:
        next(enc.encode_sequence(frames, 20, 10, 1.0, pattern=5, run_slack=3))
    assert str(e.value) == "ImageEncoder.encode_sequence: pattern is exclusive with run_slack and run_penalty"
    with pytest.raises(ValueError) as e:
        next(enc.encode_sequence(frames, 20, 10, 1.0, pattern=5, pattern_size=5))
    assert str(e.value) == "ImageEncoder.encode_sequence: pattern_size must be 2, 4 or 8"


def test_device_entry_point_raises_without_a_gpu():
    """no CPU fallback: encode_with_palette(pattern=) needs the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError
    from roibasedimagecompression_amd.image import ImageEncoder

    def run():
        return ImageEncoder().encode_with_palette(np.zeros((4, 4, 3), np.uint8), np.zeros((1, 3), np.uint8), pattern=256)
    if torch.cuda.is_available():
        assert run()["stats"]["pattern"] == {"strength": 256, "size": 4, "moved": {"all": 0}, "pixels": 16}
    else:
        with pytest.raises(RhccqError):
            run()


def test_value_claim_on_the_grey_ramp():
    """the references alone: on the 64 x 256 grey ramp with the greys 0, 85, 170, 255, pattern n = 4 at strength 256 brings the error of
    the 8 x 8 block means to at most 2 % of the nearest-row map's (0.37 % in the numpy trial that proposed the rule), and its index map
    deflates (zlib level 9) to at most a quarter of Floyd-Steinberg 256's (167 against 1 994 bytes in the trial); the caps are not
    tuned to the code under test"""
    img, pal = DC.ramp()
    out, _, b = PC.ramp_reference(4, 256)
    fs = DC.dither_reference(img, pal, 256)[0]
    plain, pattern = DC.block_mean_error(img, pal, b), DC.block_mean_error(img, pal, out)
    print(f"grey ramp: block-mean error {plain:.4f} -> {pattern:.4f} ({pattern / plain:.5f}); bytes {PC.map_bytes(b)} nearest, "
          f"{PC.map_bytes(out)} pattern, {PC.map_bytes(fs)} Floyd-Steinberg")
    assert pattern <= PC.RAMP_MAX_BLOCK_RATIO * plain
    assert PC.map_bytes(out) <= PC.RAMP_MAX_BYTES_RATIO * PC.map_bytes(fs)
    rc, got, _ = host_pattern(img, pal, None, 0, 256, 4, 1)
    assert rc == 0 and np.array_equal(got, out)


def test_value_claim_on_the_kodak_crop():
    """the references alone: on kodak_22.png[128:384, 256:512] with the 139 rows of compressed_22.rhccq, pattern n = 4 at strength 128
    brings the error of the 8 x 8 block means to at most 75 % of the nearest-row map's (68.5 % in the numpy trial); the cap is not tuned
    to the code under test"""
    img, pal = DC.kodak_crop()
    n = img.shape[0] * img.shape[1]
    out, sums, b = PC.kodak_reference(4, 128)
    base_sse = int(((img.astype(np.int64) - pal.astype(np.int64)[b]) ** 2).sum())
    plain, pattern = DC.block_mean_error(img, pal, b), DC.block_mean_error(img, pal, out)
    print(f"kodak crop: block-mean error {plain:.4f} -> {pattern:.4f} ({pattern / plain:.4f}); PSNR {RM.psnr(base_sse, n):.2f} -> "
          f"{RM.psnr(int(sums[-1, 1]), n):.2f} dB; bytes {PC.map_bytes(b)} -> {PC.map_bytes(out)}")
    assert pattern <= PC.KODAK_MAX_BLOCK_RATIO * plain
    rc, got, got_sums = host_pattern(img, pal, None, 0, 128, 4, 1)
    assert rc == 0 and np.array_equal(got, out) and np.array_equal(got_sums, sums)


def test_frame_stability_against_error_diffusion():
    """the references alone: on kodak_crop()[64:192, 64:192] with the 139 rows and a copy with fixed-seed noise of -1..1 per channel, the
    share of pixels whose index changes between the two frames is strictly smaller for pattern n = 4, s = 128 than for Floyd-Steinberg
    256.  Two references compared, no numeric margin."""
    near, pattern, fs = PC.stability()
    print(f"changed indices: nearest {near:.4f}, pattern n=4 s=128 {pattern:.4f}, Floyd-Steinberg 256 {fs:.4f}")
    assert pattern < fs
