"""Error diffusion on the device (csrc/palette_dither.hip, Rhccq.palette_dither, the dither keyword of ImageEncoder.encode_with_palette /
quantize / encode) against the numpy reference of tests/dither_cases.py, bit for bit and for every band height, and what the encoder
builds on it: the statistics, the last-step rule, the container round trip, the byte target.  Nothing here tries to make a band give
up its wait: that path is checked by reading the code.  GPU only."""
import ctypes as C

import numpy as np
import pytest

import dither_cases as DC
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


def _raw_dither(rh, rgb, pal, cls, n_classes, strength, elem_bytes):
    """rhccq_palette_dither itself, in the element width asked for; buffers pre-filled so that unwritten elements show"""
    import torch
    H, W = rgb.shape[:2]
    d_rgb, d_pal = rh.dev(np.ascontiguousarray(rgb)), rh.dev(np.ascontiguousarray(pal).reshape(-1, 3))
    d_cls = None if cls is None else rh.dev(np.ascontiguousarray(cls).reshape(-1))
    table = DC.strength_table(strength, n_classes)
    tarr = (C.c_uint32 * len(table))(*table)
    idx = torch.full((H, W), 0x2B, dtype=getattr(torch, _TDT[elem_bytes]), device=rh.device)
    sums = torch.full((n_classes + 1, 3), 0x5555, dtype=torch.int64, device=rh.device)
    status = torch.full((1,), 0x77, dtype=torch.int32, device=rh.device)
    nbytes = int(rh.lib.rhccq_palette_dither_bytes(H, W))
    work = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=rh.device)
    rc = rh.lib.rhccq_palette_dither(rh.ctx, rh._p(d_rgb), H, W, rh._p(d_pal), d_pal.shape[0], rh._p(d_cls), n_classes, C.cast(tarr, C.c_void_p),
                                     rh._p(work), nbytes, rh._p(idx), elem_bytes, rh._p(sums), rh._p(status))
    return rc, _idx64(idx), sums.cpu().numpy(), int(status.cpu()[0])


@pytest.mark.parametrize("rows", (0,) + DC.ROWS)
def test_device_equals_reference_for_every_band_height(rh, rows):
    import torch
    try:
        rh.set_option(rh.OPT_DITHER_ROWS, rows)
        for name in DC.names():
            rgb, pal, cls, nc, strength, _ = DC.case(name)
            want_out, want_sums, _, _ = DC.reference(name)
            idx, sums, status = rh.palette_dither(rgb, pal, strength, cls, nc, with_status=True)
            assert idx.dtype == (torch.uint8 if len(pal) <= 256 else torch.int16) and tuple(idx.shape) == tuple(rgb.shape[:2])
            assert sums.dtype == torch.int64 and idx.is_cuda and sums.is_cuda and status.dtype == torch.int32
            assert int(status.cpu()[0]) == 0, (rows, name)
            assert np.array_equal(_idx64(idx), want_out), (rows, name)
            assert np.array_equal(sums.cpu().numpy(), want_sums), (rows, name)
    finally:
        rh.set_option(rh.OPT_DITHER_ROWS, 0)


@pytest.mark.parametrize("name", ["bands%dx67" % (2 * DC.R + 1), "K255", "K257", "classes2", "tie", "shape1x1"])
def test_every_index_width(rh, name):
    rgb, pal, cls, nc, strength, _ = DC.case(name)
    want_out, want_sums, _, _ = DC.reference(name)
    for eb in DC.index_bytes(len(pal)):
        rc, out, sums, status = _raw_dither(rh, rgb, pal, cls, nc, strength, eb)
        assert rc == 0 and status == 0, (name, eb)
        assert np.array_equal(out, want_out), (name, eb)
        assert np.array_equal(sums, want_sums), (name, eb)


def test_band_height_option_takes_its_values_only(rh):
    from roibasedimagecompression_amd.ops import RhccqError
    try:
        for bad in (1, 2, 3, 12, 64, -4):
            with pytest.raises(RhccqError):
                rh.set_option(rh.OPT_DITHER_ROWS, bad)
    finally:
        rh.set_option(rh.OPT_DITHER_ROWS, 0)


def test_python_surface_arguments(rh):
    import torch
    from roibasedimagecompression_amd.ops import RhccqError
    rgb, pal, cls, nc, strength, _ = DC.case("classes2")
    want_out, want_sums, _, _ = DC.reference("classes2")
    forms = [(rgb, pal, cls), (torch.from_numpy(rgb.copy()), torch.from_numpy(pal.copy()), torch.from_numpy(cls.copy())),
             (rh.dev(rgb), rh.dev(pal), rh.dev(cls))]
    for r, p, c in forms:                                                          # numpy, CPU tensors, device tensors
        idx, sums = rh.palette_dither(r, p, strength, c, nc)
        assert np.array_equal(_idx64(idx), want_out) and np.array_equal(sums.cpu().numpy(), want_sums)
    idx, sums, status = rh.palette_dither(np.zeros((0, 5, 3), np.uint8), pal, 7, with_status=True)
    assert tuple(idx.shape) == (0, 5) and sums.cpu().numpy().tolist() == [[0, 0, 0]] and int(status.cpu()[0]) == 0
    rh.check_dither(status.cpu().numpy())
    with pytest.raises(RhccqError, match="palette_dither: a band gave up waiting"):
        rh.check_dither(np.array([1], np.int32))
    with pytest.raises(RhccqError, match="palette_dither: K must be 1..4096 on the device"):
        rh.palette_dither(rgb, np.zeros((4097, 3), np.uint8), 256)
    for bad, msg in ((lambda: rh.palette_dither(rgb, pal, strength, None, 2), "n_classes without a class map"),
                     (lambda: rh.palette_dither(rgb, pal, [1, 2], cls, 2), r"strength is one integer or n_classes \+ 1 of them"),
                     (lambda: rh.palette_dither(rgb, pal, 257), r"a strength must be 0\.\.256"),
                     (lambda: rh.palette_dither(rgb, pal, -1), r"a strength must be 0\.\.256"),
                     (lambda: rh.palette_dither(rgb.reshape(-1, 3), pal, 0), r"rgb \[H, W, 3\] and palette \[K, 3\] are expected"),
                     (lambda: rh.palette_dither(rgb, pal, strength, cls[:-1], 2), "the class map must have one element per pixel")):
        with pytest.raises(ValueError, match="palette_dither: " + msg):
            bad()


DEVICE_ERRORS = DC.ERRORS + [
    ("null status", {"status": None}, DC.E_ARG),
    ("misaligned status", {"status": 2}, DC.E_ARG),
    ("null workspace", {"work": None}, DC.E_ARG),
    ("misaligned workspace", {"work": 2}, DC.E_ARG),
    ("workspace one byte short", {"short": 1}, DC.E_ARG),
    ("K = 4097", {"K": 4097}, DC.E_LIMIT),
]


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
    nbytes = int(rh.lib.rhccq_palette_dither_bytes(2, 2))
    work, status = rh.zeros((nbytes // 4 + 1,), torch.int32), rh.zeros((2,), torch.int32)

    def ptr(name, tensor):
        v = over.get(name, 0)
        return C.c_void_p(0) if v is None else C.c_void_p(tensor.data_ptr() + v)
    rc = rh.lib.rhccq_palette_dither(rh.ctx, rh._p(t["rgb"]), over.get("H", 2), over.get("W", 2), rh._p(t["palette"]), over.get("K", 3), rh._p(cls),
                                     over.get("n_classes", 0), C.cast(tarr, C.c_void_p) if tarr is not None else C.c_void_p(0), ptr("work", work),
                                     nbytes - over.get("short", 0), rh._p(t["idx_out"]), over.get("idx_elem_bytes", 2), rh._p(t["sums"]),
                                     ptr("status", status))
    assert rc == code, what
    assert rh._raw.rhccq_last_error(rh.ctx).decode().startswith("palette_dither:")


def test_kodak_crop_equals_the_host_form(rh):
    img, pal = DC.kodak_crop()
    for strength in (128, 256):
        rc, want, want_sums = DC.host_dither(img, pal, None, 0, strength, 1)
        idx, sums = rh.palette_dither(img, pal, strength)
        assert rc == 0 and np.array_equal(_idx64(idx), want) and np.array_equal(sums.cpu().numpy(), want_sums), strength
        assert 0 < want_sums[-1, 2] < want_sums[-1, 0]


# ---- ImageEncoder.encode_with_palette(dither=) -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def photo():
    """roimask_cases' photo96 (96 x 128), its mask, and 300 of its pixels as the palette (2-byte indices; colours=64 gives 1-byte ones)"""
    _, img, mask = RC.case("photo96")
    flat = img.reshape(-1, 3)
    pal = flat[np.random.default_rng(9).choice(len(flat), 300, replace=False)].copy()
    return img, mask, pal


def _check_result(res, img, mask, dither):
    """the result's indices and statistics against the reference over the RETURNED palette -> (out, sums, b)"""
    pal = np.asarray(res["palette"], np.uint8).reshape(-1, 3)
    if mask is None:
        want_out, want_sums, b, _ = DC.dither_reference(img, pal, dither)
        rows = {"all": want_sums[0]}
    else:
        table = [dither["nonroi"], dither["roi"], min(dither.values())] if isinstance(dither, dict) else [dither] * 3
        want_out, want_sums, b, _ = DC.dither_reference(img, pal, table, mask.astype(np.uint8), 2)
        rows = {"nonroi": want_sums[0], "roi": want_sums[1], "all": want_sums[2]}
    assert np.array_equal(_idx64(res["indices"]), want_out)
    assert res["indices_dtype"] == ("uint8" if len(pal) <= 256 else "uint16") and tuple(res["indices"].shape) == img.shape[:2]
    st = res["stats"]
    assert sorted(st["remap"]) == sorted(rows)
    for n, row in rows.items():
        assert (st["remap"][n]["pixels"], st["remap"][n]["sse"]) == (int(row[0]), int(row[1])), n
        assert abs(st["remap"][n]["psnr"] - RM.psnr(int(row[1]), int(row[0]))) < 1e-9
    assert st["dither"] == {"strength": dither, "moved": {n: int(row[2]) for n, row in rows.items()}, "pixels": img.shape[0] * img.shape[1]}
    assert "runs" not in st
    return want_out, want_sums, b


@pytest.mark.parametrize("masked,dither", [(False, 256), (True, 128), (True, {"roi": 0, "nonroi": 256}), (False, 0)])
def test_encode_with_palette_dither(enc, photo, masked, dither):
    img, mask, pal = photo
    mask = mask if masked else None
    res = enc.encode_with_palette(img, pal, roi_mask=mask, dither=dither)
    want_out, want_sums, b = _check_result(res, img, mask, dither)
    assert np.array_equal(res["palette"], pal)
    plain = enc.encode_with_palette(img, pal, roi_mask=mask)
    assert "dither" not in plain["stats"] and np.array_equal(_idx64(plain["indices"]), b)
    if dither == 0:                                                             # 0 is a value: the nearest-row map, with its statistics
        assert np.array_equal(_idx64(res["indices"]), b) and plain["stats"]["remap"] == res["stats"]["remap"]
    else:
        assert want_sums[-1, 2] > 0 and plain["stats"]["remap"]["all"]["sse"] < res["stats"]["remap"]["all"]["sse"]
    if isinstance(dither, dict):                                                # strength 0 inside the mask: those pixels keep their nearest row
        inside = mask.astype(bool)
        assert np.array_equal(want_out[inside], b[inside]) and want_sums[1, 2] == 0 < want_sums[0, 2]


def test_dither_arguments(enc, photo):
    img, mask, pal = photo
    for kw in ({"dither": {"roi": 1, "nonroi": 2}}, {"dither": {"roi": 1}, "roi_mask": mask}, {"dither": -1}, {"dither": 257},
               {"dither": 5, "run_slack": 5}, {"dither": 5, "run_penalty": 5}, {"dither": 5, "target_psnr": 30.0}):
        with pytest.raises(ValueError):
            enc.encode_with_palette(img, pal, **kw)
        with pytest.raises(ValueError):
            enc.quantize(img, 16, **kw)
    with pytest.raises(ValueError, match="ImageEncoder.encode: dither is exclusive with run_slack and run_penalty"):
        enc.encode(img, 20, 10, dither=5, run_slack=5)


def test_dither_is_the_last_step(enc, photo):
    """colours= and refine= run first, on the nearest-row assignment; the palette and their statistics are those of the call without dither"""
    img, mask, pal = photo
    dither = {"roi": 64, "nonroi": 256}
    res = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=3, colours=64, refine=2, dither=dither)
    plain = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=3, colours=64, refine=2)
    assert np.array_equal(res["palette"], plain["palette"]) and len(res["palette"]) == 64
    assert res["stats"]["reduce"] == plain["stats"]["reduce"] and res["stats"]["refine"] == plain["stats"]["refine"]
    _check_result(res, img, mask, dither)


def test_container_round_trip(rh, enc, photo, tmp_path):
    from roibasedimagecompression_amd import container
    img, _, pal = photo
    path = str(tmp_path / "dither.rhccq")
    res = enc.encode_with_palette(img, pal, dither=256, out_path=path, exact=True)
    want_out, _, _ = _check_result(res, img, None, 256)
    back = container.read_frame(path, rh)
    assert np.array_equal(_idx64(back["indices"]).reshape(want_out.shape), want_out) and np.array_equal(back["palette"].cpu().numpy(), pal)
    assert np.array_equal(back["image"].cpu().numpy().reshape(img.shape), pal[want_out])


def test_target_bytes_probes_run_with_the_dither(rh, enc, photo, tmp_path):
    import os
    from roibasedimagecompression_amd import container
    img, _, pal = photo
    full = len(container.frame_bytes(enc.encode_with_palette(img, pal, dither=256), rh, exact=True))
    out = str(tmp_path / "t.rhccq")
    res = enc.encode_with_palette(img, pal, target_bytes=int(full * 0.6), dither=256, exact=True, out_path=out)
    tg = res["stats"]["target"]
    assert tg["kind"] == "bytes" and tg["met"] is True and len(tg["probes"]) > 1 and tg["bound_psnr"] == {"all": None}
    k = tg["colours"]
    again = enc.encode_with_palette(img, pal, colours=k, dither=256)              # the rung it returns is one it verified
    assert dict(tg["probes"])[k] == len(container.frame_bytes(again, rh, exact=True)) == os.path.getsize(out) <= int(full * 0.6)
    assert np.array_equal(again["palette"], res["palette"]) and np.array_equal(_idx64(again["indices"]), _idx64(res["indices"]))
    assert again["stats"]["dither"] == res["stats"]["dither"] and again["stats"]["remap"] == res["stats"]["remap"]
    _check_result(res, img, None, 256)


# ---- ImageEncoder.quantize(dither=) and encode(dither=) -----------------------------------------------------------------------------
def test_quantize_dither(enc, photo):
    img, mask, _ = photo
    res = enc.quantize(img, 16, dither=256)
    plain = enc.quantize(img, 16)
    assert np.array_equal(res["palette"], plain["palette"]) and res["stats"]["build"] == plain["stats"]["build"]
    _, want_sums, _ = _check_result(res, img, None, 256)                          # over its own palette
    assert want_sums[-1, 2] > 0
    masked = enc.quantize(img, 16, roi_mask=mask, dither={"roi": 0, "nonroi": 200})
    _check_result(masked, img, mask, {"roi": 0, "nonroi": 200})


def test_encode_dither(rh, enc, tmp_path):
    from roibasedimagecompression_amd import container
    (q1, q2), img, mask = RC.case("photo96")
    base = enc.encode(img, q1, q2, roi_mask=mask)
    assert "dither" not in base["stats"] and tuple(base["top_left"]) == (0, 0) and tuple(base["shape"]) == img.shape[:2]
    pal = np.asarray(base["palette"], np.uint8).reshape(-1, 3)
    cls = enc.region_map.cpu().numpy().astype(np.uint8)                          # the map the encoder made of the mask: 1 inside, 0 outside
    dither = {"roi": 32, "nonroi": 256}
    path = str(tmp_path / "e.rhccq")
    res = enc.encode(img, q1, q2, roi_mask=mask, dither=dither, out_path=path, exact=True)
    assert np.array_equal(np.asarray(res["palette"], np.uint8).reshape(-1, 3), pal)          # the rewrite goes over its own palette
    want_out, want_sums, _, _ = DC.dither_reference(img, pal, [256, 32, 32], cls, 2)
    assert np.array_equal(_idx64(res["indices"]).reshape(want_out.shape), want_out)
    assert tuple(res["indices"].shape) == tuple(base["indices"].shape) and res["indices"].dtype == base["indices"].dtype
    assert res["stats"]["dither"] == {"strength": dither, "moved": {"all": int(want_sums[2, 2]), "roi": int(want_sums[1, 2]),
                                                                    "nonroi": int(want_sums[0, 2])}, "pixels": img.shape[0] * img.shape[1]}
    assert "runs" not in res["stats"] and want_sums[2, 2] > 0
    back = container.read_frame(path, rh)
    assert np.array_equal(_idx64(back["indices"]).reshape(want_out.shape), want_out)
