"""The pattern dither on the device (csrc/palette_pattern.hip, Rhccq.palette_pattern / palette_pattern_batch, the pattern keyword of
ImageEncoder.encode_with_palette / quantize / encode / quantize_batch / encode_sequence) against the numpy reference of
tests/pattern_cases.py, bit for bit, and what the encoder builds on it: the statistics, the last-step rule, the byte target, the batch,
the sequence, the position-only property.  GPU only."""
import ctypes as C

import numpy as np
import pytest

import pattern_cases as PC
import remap_cases as RM
import roimask_cases as RC

pytestmark = pytest.mark.gpu

_TDT = {1: "uint8", 2: "int16", 4: "int32"}


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


@pytest.fixture(scope="module")
def enc(rh):
    from roibasedimagecompression_amd.image import ImageEncoder
    return ImageEncoder(rh)


def _idx64(t):
    a = t.cpu().numpy()
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    elif a.dtype == np.int32:
        a = a.view(np.uint32)
    return a.astype(np.int64)


def _raw_pattern(rh, rgb, pal, cls, n_classes, strength, size, elem_bytes):
    """rhccq_palette_pattern itself, in the element width asked for; buffers pre-filled so that unwritten elements show"""
    import torch
    H, W = rgb.shape[:2]
    d_rgb, d_pal = rh.dev(np.ascontiguousarray(rgb)), rh.dev(np.ascontiguousarray(pal).reshape(-1, 3))
    d_cls = None if cls is None else rh.dev(np.ascontiguousarray(cls).reshape(-1))
    table = PC.strength_table(strength, n_classes)
    tarr = (C.c_uint32 * len(table))(*table)
    idx = torch.full((H, W), 0x2B, dtype=getattr(torch, _TDT[elem_bytes]), device=rh.device)
    sums = torch.full((n_classes + 1, 3), 0x5555, dtype=torch.int64, device=rh.device)
    rc = rh.lib.rhccq_palette_pattern(rh.ctx, rh._p(d_rgb), H, W, rh._p(d_pal), d_pal.shape[0], rh._p(d_cls), n_classes, C.cast(tarr, C.c_void_p),
                                      size, rh._p(idx), elem_bytes, rh._p(sums))
    return rc, _idx64(idx), sums.cpu().numpy()


@pytest.mark.parametrize("name", PC.names())
def test_device_equals_reference(rh, name):
    import torch
    rgb, pal, cls, nc, strength, size, _ = PC.case(name)
    want_out, want_sums, _, _ = PC.reference(name)
    idx, sums = rh.palette_pattern(rgb, pal, strength, size, cls, nc)
    assert idx.dtype == (torch.uint8 if len(pal) <= 256 else torch.int16) and tuple(idx.shape) == tuple(rgb.shape[:2])
    assert sums.dtype == torch.int64 and idx.is_cuda and sums.is_cuda
    assert np.array_equal(_idx64(idx), want_out)
    assert np.array_equal(sums.cpu().numpy(), want_sums)


@pytest.mark.parametrize("name", ["chunks3x701_n4", "K255", "K257", "classes2", "floor", "shape1x1"])
def test_every_index_width(rh, name):
    rgb, pal, cls, nc, strength, size, _ = PC.case(name)
    want_out, want_sums, _, _ = PC.reference(name)
    for eb in PC.index_bytes(len(pal)):
        rc, out, sums = _raw_pattern(rh, rgb, pal, cls, nc, strength, size, eb)
        assert rc == 0, (name, eb)
        assert np.array_equal(out, want_out), (name, eb)
        assert np.array_equal(sums, want_sums), (name, eb)


def test_more_chunks_than_workgroups(rh):
    """a picture of more chunks than the launch has workgroups (16 per compute unit), so that a workgroup takes a second chunk: 700 x 801
    pixels at n = 8 are 4 381 chunks of 128.  Against the host form, which the CPU suite pins to the reference"""
    rng = np.random.default_rng(3)
    rgb = PC._image(rng, 700, 801)
    pal = np.array([[40, 40, 40], [128, 120, 110], [230, 220, 240]], np.uint8)
    rc, want, want_sums = PC.host_pattern(rgb, pal, None, 0, 256, 8, 1)
    idx, sums = rh.palette_pattern(rgb, pal, 256, 8)
    assert rc == 0 and np.array_equal(_idx64(idx), want) and np.array_equal(sums.cpu().numpy(), want_sums)
    assert 0 < want_sums[-1, 2] < want_sums[-1, 0]


def test_python_surface_arguments(rh):
    import torch
    from roibasedimagecompression_amd.ops import RhccqError
    rgb, pal, cls, nc, strength, size, _ = PC.case("classes2")
    want_out, want_sums, _, _ = PC.reference("classes2")
    forms = [(rgb, pal, cls), (torch.from_numpy(rgb.copy()), torch.from_numpy(pal.copy()), torch.from_numpy(cls.copy())),
             (rh.dev(rgb), rh.dev(pal), rh.dev(cls))]
    for r, p, c in forms:                                                          # numpy, CPU tensors, device tensors
        idx, sums = rh.palette_pattern(r, p, strength, size, c, nc)
        assert np.array_equal(_idx64(idx), want_out) and np.array_equal(sums.cpu().numpy(), want_sums)
    idx, sums = rh.palette_pattern(rgb, pal, strength, class_map=cls, n_classes=nc)            # size defaults to 4
    assert size == 4 and np.array_equal(_idx64(idx), want_out)
    idx, sums = rh.palette_pattern(np.zeros((0, 5, 3), np.uint8), pal, 7)
    assert tuple(idx.shape) == (0, 5) and sums.cpu().numpy().tolist() == [[0, 0, 0]]
    with pytest.raises(RhccqError, match="palette_pattern: K must be 1..4096 on the device"):
        rh.palette_pattern(rgb, np.zeros((4097, 3), np.uint8), 256)
    for bad, msg in ((lambda: rh.palette_pattern(rgb, pal, strength, 4, None, 2), "n_classes without a class map"),
                     (lambda: rh.palette_pattern(rgb, pal, [1, 2], 4, cls, 2), r"strength is one integer or n_classes \+ 1 of them"),
                     (lambda: rh.palette_pattern(rgb, pal, 257), r"a strength must be 0\.\.256"),
                     (lambda: rh.palette_pattern(rgb, pal, -1), r"a strength must be 0\.\.256"),
                     (lambda: rh.palette_pattern(rgb, pal, 5, 3), "size must be 2, 4 or 8"),
                     (lambda: rh.palette_pattern(rgb.reshape(-1, 3), pal, 0), r"rgb \[H, W, 3\] and palette \[K, 3\] are expected"),
                     (lambda: rh.palette_pattern(rgb, pal, strength, 4, cls[:-1], 2), "the class map must have one element per pixel")):
        with pytest.raises(ValueError, match="palette_pattern: " + msg):
            bad()


DEVICE_ERRORS = PC.ERRORS + [("K = 4097", {"K": 4097}, PC.E_LIMIT)]


@pytest.mark.parametrize("what,over,code", DEVICE_ERRORS, ids=[e[0] for e in DEVICE_ERRORS])
def test_device_argument_errors(rh, what, over, code):
    """every refusal comes before anything is queued"""
    import torch
    t = {"rgb": rh.zeros((4, 3), torch.uint8), "palette": rh.zeros((3, 3), torch.uint8), "idx_out": rh.zeros((4,), torch.int32),
         "sums": rh.zeros((18, 3), torch.int64)}
    t.update({k: v for k, v in over.items() if k in t})
    cls = rh.zeros((4,), torch.uint8) if over.get("cls") else None
    strength = over.get("strength", [5])
    tarr = None if strength is None else (C.c_uint32 * len(strength))(*strength)
    rc = rh.lib.rhccq_palette_pattern(rh.ctx, rh._p(t["rgb"]), over.get("H", 2), over.get("W", 2), rh._p(t["palette"]), over.get("K", 3), rh._p(cls),
                                      over.get("n_classes", 0), C.cast(tarr, C.c_void_p) if tarr is not None else C.c_void_p(0), over.get("size", 4),
                                      rh._p(t["idx_out"]), over.get("idx_elem_bytes", 2), rh._p(t["sums"]))
    assert rc == code, what
    assert rh._raw.rhccq_last_error(rh.ctx).decode().startswith("palette_pattern:")


def test_kodak_crop_equals_the_reference(rh):
    from dither_cases import kodak_crop
    img, pal = kodak_crop()
    want, want_sums, _ = PC.kodak_reference(4, 128)
    idx, sums = rh.palette_pattern(img, pal, 128, 4)
    assert np.array_equal(_idx64(idx), want) and np.array_equal(sums.cpu().numpy(), want_sums)
    assert 0 < want_sums[-1, 2] < want_sums[-1, 0]


def test_position_only(rh):
    """the same pixels placed at the same (y mod n, x mod n) in two different pictures get the same index"""
    rng = np.random.default_rng(5)
    pal = RM._palette(rng, 23)
    for n in PC.SIZES:
        block = PC._image(rng, 2 * n + 3, 3 * n + 1)
        h, w = block.shape[:2]
        a = PC._image(rng, 5 * n, 6 * n + 5)
        b = PC._image(rng, 5 * n + 3, 7 * n)
        a[n:n + h, 2 * n:2 * n + w] = block
        b[2 * n:2 * n + h, 3 * n:3 * n + w] = block
        ia, ib = _idx64(rh.palette_pattern(a, pal, 256, n)[0]), _idx64(rh.palette_pattern(b, pal, 256, n)[0])
        assert np.array_equal(ia[n:n + h, 2 * n:2 * n + w], ib[2 * n:2 * n + h, 3 * n:3 * n + w]), n
        shifted = _idx64(rh.palette_pattern(np.ascontiguousarray(a[:, 1:]), pal, 256, n)[0])       # another phase: not the same map
        assert not np.array_equal(shifted[n:n + h, 2 * n - 1:2 * n - 1 + w], ia[n:n + h, 2 * n:2 * n + w]), n


# ---- Rhccq.palette_pattern_batch ------------------------------------------------------------------------------------------------------
def test_batch_equals_the_single_calls(rh):
    rng = np.random.default_rng(11)
    frames = [PC._image(rng, 5, 7), PC._image(rng, 37, 41), PC._image(rng, 3, 11), PC._image(rng, 0, 6), PC._image(rng, 9, 130)]
    pals = [RM._palette(rng, 5), RM._palette(rng, 17), RM._palette(rng, 9), RM._palette(rng, 3), RM._palette(rng, 300)]
    rows = [5, 17, 0, 3, 300]
    stride = max(len(p) for p in pals)
    palettes = np.zeros((len(frames), stride, 3), np.uint8)
    for i, p in enumerate(pals):
        palettes[i, :len(p)] = p
    off = np.concatenate([[0], np.cumsum([f.shape[0] * f.shape[1] for f in frames])]).astype(np.int64)
    rgb = np.concatenate([f.reshape(-1, 3) for f in frames])
    cls = rng.integers(0, 3, int(off[-1])).astype(np.uint8)
    table = [256, 0, 77]
    for size in PC.SIZES:
        idx, sums = rh.palette_pattern_batch(rgb, off, [f.shape[1] for f in frames], palettes, np.array(rows, np.int32), table, size, cls, 2)
        idx, sums = _idx64(idx), sums.cpu().numpy()
        for i, (f, p) in enumerate(zip(frames, pals)):
            got = idx[off[i]:off[i + 1]].reshape(f.shape[:2])
            if rows[i] == 0:
                assert not got.any() and not sums[i].any()
                continue
            want, want_sums, _, _ = PC.pattern_reference(f, p, table, size, cls[off[i]:off[i + 1]], 2)
            assert np.array_equal(got, want) and np.array_equal(sums[i], want_sums), (size, i)
    with pytest.raises(ValueError, match="palette_pattern_batch: widths must hold one width per image"):
        rh.palette_pattern_batch(rgb, off, [7, 40, 11, 6, 130], palettes, np.array(rows, np.int32), table, 4, cls, 2)
    with pytest.raises(ValueError, match="palette_pattern_batch: size must be 2, 4 or 8"):
        rh.palette_pattern_batch(rgb, off, [f.shape[1] for f in frames], palettes, np.array(rows, np.int32), table, 6, cls, 2)


# ---- ImageEncoder.encode_with_palette(pattern=) -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def photo():
    """roimask_cases' photo96 (96 x 128), its mask, and 300 of its pixels as the palette (2-byte indices; colours=64 gives 1-byte ones)"""
    _, img, mask = RC.case("photo96")
    flat = img.reshape(-1, 3)
    pal = flat[np.random.default_rng(9).choice(len(flat), 300, replace=False)].copy()
    return img, mask, pal


def _check_result(res, img, mask, pattern, size=4):
    """the result's indices and statistics against the reference over the RETURNED palette -> (out, sums, b)"""
    pal = np.asarray(res["palette"], np.uint8).reshape(-1, 3)
    if mask is None:
        want_out, want_sums, b, _ = PC.pattern_reference(img, pal, pattern, size)
        rows = {"all": want_sums[0]}
    else:
        table = [pattern["nonroi"], pattern["roi"], min(pattern.values())] if isinstance(pattern, dict) else [pattern] * 3
        want_out, want_sums, b, _ = PC.pattern_reference(img, pal, table, size, np.asarray(mask).astype(np.uint8), 2)
        rows = {"nonroi": want_sums[0], "roi": want_sums[1], "all": want_sums[2]}
    assert np.array_equal(_idx64(res["indices"]), want_out)
    assert res["indices_dtype"] == ("uint8" if len(pal) <= 256 else "uint16") and tuple(res["indices"].shape) == img.shape[:2]
    st = res["stats"]
    assert sorted(st["remap"]) == sorted(rows)
    for n, row in rows.items():
        assert (st["remap"][n]["pixels"], st["remap"][n]["sse"]) == (int(row[0]), int(row[1])), n
        assert abs(st["remap"][n]["psnr"] - RM.psnr(int(row[1]), int(row[0]))) < 1e-9
    assert st["pattern"] == {"strength": pattern, "size": size, "moved": {n: int(row[2]) for n, row in rows.items()},
                             "pixels": img.shape[0] * img.shape[1]}
    assert "runs" not in st and "dither" not in st
    return want_out, want_sums, b


@pytest.mark.parametrize("masked,pattern,size", [(False, 256, 4), (True, 128, 8), (True, {"roi": 0, "nonroi": 256}, 2), (False, 0, 4)])
def test_encode_with_palette_pattern(enc, photo, masked, pattern, size):
    img, mask, pal = photo
    mask = mask if masked else None
    res = enc.encode_with_palette(img, pal, roi_mask=mask, pattern=pattern, pattern_size=size)
    want_out, want_sums, b = _check_result(res, img, mask, pattern, size)
    assert np.array_equal(res["palette"], pal)
    plain = enc.encode_with_palette(img, pal, roi_mask=mask)
    assert "pattern" not in plain["stats"] and np.array_equal(_idx64(plain["indices"]), b)
    if pattern == 0:                                                            # 0 is a value: the nearest-row map, with its statistics
        assert np.array_equal(_idx64(res["indices"]), b) and plain["stats"]["remap"] == res["stats"]["remap"]
    else:
        assert want_sums[-1, 2] > 0 and plain["stats"]["remap"]["all"]["sse"] < res["stats"]["remap"]["all"]["sse"]
    if isinstance(pattern, dict):                                               # strength 0 inside the mask: those pixels keep their nearest row
        inside = mask.astype(bool)
        assert np.array_equal(want_out[inside], b[inside]) and want_sums[1, 2] == 0 < want_sums[0, 2]


def test_pattern_arguments(enc, photo):
    img, mask, pal = photo
    for kw in ({"pattern": {"roi": 1, "nonroi": 2}}, {"pattern": {"roi": 1}, "roi_mask": mask}, {"pattern": -1}, {"pattern": 257},
               {"pattern": 5, "run_slack": 5}, {"pattern": 5, "run_penalty": 5}, {"pattern": 5, "dither": 5}, {"pattern": 5, "target_psnr": 30.0},
               {"pattern": 5, "pattern_size": 3}):
        with pytest.raises(ValueError):
            enc.encode_with_palette(img, pal, **kw)
        with pytest.raises(ValueError):
            enc.quantize(img, 16, **kw)
    with pytest.raises(ValueError, match="ImageEncoder.encode: pattern is exclusive with run_slack and run_penalty"):
        enc.encode(img, 20, 10, pattern=5, run_slack=5)
    with pytest.raises(ValueError, match="ImageEncoder.encode: pattern cannot be combined with target_psnr"):
        enc.encode(img, 20, 10, pattern=5, target_psnr=30.0)
    with pytest.raises(ValueError, match="ImageEncoder.quantize_batch: a roi / nonroi pattern needs roi_mask"):
        enc.quantize_batch([img, img], 16, roi_masks=[mask, None], pattern={"roi": 1, "nonroi": 2})
    with pytest.raises(ValueError, match="ImageEncoder.quantize_batch: pattern_size must be 2, 4 or 8"):
        enc.quantize_batch([img], 16, pattern=5, pattern_size=16)


def test_pattern_is_the_last_step(enc, photo):
    """colours= and refine= run first, on the nearest-row assignment; the palette and their statistics are those of the call without pattern"""
    img, mask, pal = photo
    pattern = {"roi": 64, "nonroi": 256}
    res = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=3, colours=64, refine=2, pattern=pattern)
    plain = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=3, colours=64, refine=2)
    assert np.array_equal(res["palette"], plain["palette"]) and len(res["palette"]) == 64
    assert res["stats"]["reduce"] == plain["stats"]["reduce"] and res["stats"]["refine"] == plain["stats"]["refine"]
    _check_result(res, img, mask, pattern)


def test_target_bytes_probes_run_with_the_pattern(rh, enc, photo, tmp_path):
    import os
    from roibasedimagecompression_amd import container
    img, _, pal = photo
    full = len(container.frame_bytes(enc.encode_with_palette(img, pal, pattern=256), rh, exact=True))
    out = str(tmp_path / "t.rhccq")
    res = enc.encode_with_palette(img, pal, target_bytes=int(full * 0.6), pattern=256, exact=True, out_path=out)
    tg = res["stats"]["target"]
    assert tg["kind"] == "bytes" and tg["met"] is True and len(tg["probes"]) > 1 and tg["bound_psnr"] == {"all": None}
    k = tg["colours"]
    again = enc.encode_with_palette(img, pal, colours=k, pattern=256)             # the rung it returns is one it verified
    assert dict(tg["probes"])[k] == len(container.frame_bytes(again, rh, exact=True)) == os.path.getsize(out) <= int(full * 0.6)
    assert np.array_equal(again["palette"], res["palette"]) and np.array_equal(_idx64(again["indices"]), _idx64(res["indices"]))
    assert again["stats"]["pattern"] == res["stats"]["pattern"] and again["stats"]["remap"] == res["stats"]["remap"]
    _check_result(res, img, None, 256)                                           # the returned rung's map is the reference's


# ---- ImageEncoder.quantize(pattern=), quantize_batch(pattern=), encode(pattern=), encode_sequence(pattern=) ------------------------------
def test_quantize_pattern(enc, photo):
    img, mask, _ = photo
    res = enc.quantize(img, 16, pattern=256, pattern_size=8)
    plain = enc.quantize(img, 16)
    assert np.array_equal(res["palette"], plain["palette"]) and res["stats"]["build"] == plain["stats"]["build"]
    _, want_sums, _ = _check_result(res, img, None, 256, 8)                       # over its own palette
    assert want_sums[-1, 2] > 0
    masked = enc.quantize(img, 16, roi_mask=mask, pattern={"roi": 0, "nonroi": 200})
    _check_result(masked, img, mask, {"roi": 0, "nonroi": 200})


def _same_result(a, b):
    assert np.array_equal(a["palette"], b["palette"]) and a["indices"].dtype == b["indices"].dtype
    assert np.array_equal(_idx64(a["indices"]), _idx64(b["indices"])) and a["indices_dtype"] == b["indices_dtype"]
    assert a["shape"] == b["shape"] and a["top_left"] == b["top_left"]
    sa, sb = dict(a["stats"]), dict(b["stats"])
    sa.pop("seconds"), sb.pop("seconds")
    assert sa == sb


@pytest.mark.parametrize("pattern,size,refine,masked", [(256, 4, 0, False), (128, 8, 2, False), ({"roi": 0, "nonroi": 200}, 2, 0, True), (77, 4, 1, True)])
def test_quantize_batch_pattern_equals_the_loop(enc, photo, pattern, size, refine, masked):
    img, mask, _ = photo
    images = [img, np.ascontiguousarray(img[:37, :53]), np.ascontiguousarray(img[40:61, 9:128])]
    masks = [mask, np.ascontiguousarray(mask[:37, :53]), np.ascontiguousarray(mask[40:61, 9:128])]
    if not masked:
        masks = None
    elif not isinstance(pattern, dict):
        masks[1] = None                                                          # a number takes images without a mask beside masked ones
    got = enc.quantize_batch(images, 16, refine=refine, roi_masks=masks, roi_weight=3 if masked else 1, pattern=pattern, pattern_size=size)
    for i, (im, res) in enumerate(zip(images, got)):
        m = None if masks is None else masks[i]
        want = enc.quantize(im, 16, refine=refine, roi_mask=m, roi_weight=3 if m is not None else 1, pattern=pattern, pattern_size=size)
        _same_result(res, want)
        _check_result(res, im, m, pattern, size)
    plain = enc.quantize_batch(images, 16, refine=refine, roi_masks=masks, roi_weight=3 if masked else 1)
    assert all("pattern" not in r["stats"] for r in plain)


def test_encode_pattern(rh, enc, tmp_path):
    from roibasedimagecompression_amd import container
    (q1, q2), img, mask = RC.case("photo96")
    base = enc.encode(img, q1, q2, roi_mask=mask)
    assert "pattern" not in base["stats"] and tuple(base["top_left"]) == (0, 0) and tuple(base["shape"]) == img.shape[:2]
    pal = np.asarray(base["palette"], np.uint8).reshape(-1, 3)
    cls = enc.region_map.cpu().numpy().astype(np.uint8)                          # the map the encoder made of the mask: 1 inside, 0 outside
    pattern = {"roi": 32, "nonroi": 256}
    path = str(tmp_path / "e.rhccq")
    res = enc.encode(img, q1, q2, roi_mask=mask, pattern=pattern, pattern_size=8, out_path=path, exact=True)
    assert np.array_equal(np.asarray(res["palette"], np.uint8).reshape(-1, 3), pal)          # the rewrite goes over its own palette
    want_out, want_sums, _, _ = PC.pattern_reference(img, pal, [256, 32, 32], 8, cls, 2)
    assert np.array_equal(_idx64(res["indices"]).reshape(want_out.shape), want_out)
    assert tuple(res["indices"].shape) == tuple(base["indices"].shape) and res["indices"].dtype == base["indices"].dtype
    assert res["stats"]["pattern"] == {"strength": pattern, "size": 8, "moved": {"all": int(want_sums[2, 2]), "roi": int(want_sums[1, 2]),
                                                                               "nonroi": int(want_sums[0, 2])}, "pixels": img.shape[0] * img.shape[1]}
    assert "runs" not in res["stats"] and "dither" not in res["stats"] and want_sums[2, 2] > 0
    back = container.read_frame(path, rh)
    assert np.array_equal(_idx64(back["indices"]).reshape(want_out.shape), want_out)


def test_encode_sequence_pattern(enc, photo):
    """three small frames, the key frame by quantize: every frame's map is the reference's over the palette it returns, and the PSNR the
    key-frame rule compares is the dithered map's"""
    img, _, _ = photo
    rng = np.random.default_rng(2)
    frames = [np.ascontiguousarray(img[:48, :64])]
    frames.append(np.clip(frames[0].astype(np.int64) + rng.integers(-1, 2, frames[0].shape), 0, 255).astype(np.uint8))
    frames.append(np.ascontiguousarray(img[48:96, 64:128]))                       # other content: a remap that loses, refined or a new key
    out = list(enc.encode_sequence(frames, 20, 10, 1.5, refine=2, key_colours=24, pattern=128, pattern_size=4))
    assert [r["stats"]["key_frame"] for r in out][:2] == [True, False]
    for f, res in zip(frames, out):
        want_out, want_sums, _ = _check_result(res, f, None, 128, 4)
        assert abs(res["stats"]["psnr"] - RM.psnr(int(want_sums[-1, 1]), int(want_sums[-1, 0]))) < 1e-9
    assert np.array_equal(out[1]["palette"], out[0]["palette"])
    plain = list(enc.encode_sequence(frames[:2], 20, 10, 1.5, key_colours=24))
    assert all("pattern" not in r["stats"] for r in plain)
