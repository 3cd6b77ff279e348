"""The nearest-colour remap on the device (csrc/palette_remap.hip, Rhccq.palette_remap, ImageEncoder.encode_with_palette /
encode_sequence) against the numpy reference of tests/remap_cases.py, bit for bit, and the properties that follow from it:
a remap onto the encoder's own palette never has a larger squared error, a decoded picture remaps onto itself, the container
round trip, the per-class rows, the key-frame rule of a sequence.  GPU only."""
import numpy as np
import pytest

import remap_cases as RM
import roimask_cases as RC

pytestmark = pytest.mark.gpu

_TDT = {1: "uint8", 2: "int16", 4: "int32"}
_NDT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


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
    return a.reshape(-1).astype(np.int64)


def _raw_remap(rh, rgb, pal, cls, n_classes, elem_bytes):
    """rhccq_palette_remap itself, in the element width asked for; buffers pre-filled so that unwritten elements show"""
    import torch
    d_rgb, d_pal = rh.dev(np.ascontiguousarray(rgb).reshape(-1, 3)), rh.dev(np.ascontiguousarray(pal).reshape(-1, 3))
    d_cls = None if cls is None else rh.dev(np.ascontiguousarray(cls).reshape(-1))
    n = d_rgb.shape[0]
    if n == 0:                                           # (an empty tensor has a null pointer: the C entry wants real buffers)
        d_rgb = rh.zeros((1, 3), torch.uint8)
    idx = torch.full((max(n, 1),), 0x2B, dtype=getattr(torch, _TDT[elem_bytes]), device=rh.device)
    sums = torch.full((n_classes + 1, 2), 0x5555, dtype=torch.int64, device=rh.device)
    rc = rh.lib.rhccq_palette_remap(rh.ctx, rh._p(d_rgb), n, rh._p(d_pal), d_pal.shape[0], rh._p(d_cls), n_classes, rh._p(idx), elem_bytes,
                                    rh._p(sums))
    return rc, _idx64(idx)[:n], sums.cpu().numpy()


@pytest.mark.parametrize("name", RM.names())
def test_device_equals_reference(rh, name):
    import torch
    rgb, pal, cls, nc, _ = RM.case(name)
    want_idx, want_sums = RM.reference(name)
    for eb in RM.index_bytes(len(pal)):
        rc, idx, sums = _raw_remap(rh, rgb, pal, cls, nc, eb)
        assert rc == 0, (name, eb)
        assert np.array_equal(idx, want_idx), (name, eb)
        assert np.array_equal(sums, want_sums), (name, eb)
    # the Python surface: numpy arguments, the repository's index storage, the pixel shape kept
    idx, sums = rh.palette_remap(rgb, pal, cls, nc)
    assert idx.dtype == (torch.uint8 if len(pal) <= 256 else torch.int16) and tuple(idx.shape) == tuple(rgb.shape[:-1])
    assert sums.dtype == torch.int64 and idx.is_cuda and sums.is_cuda
    assert np.array_equal(_idx64(idx), want_idx) and np.array_equal(sums.cpu().numpy(), want_sums), name


@pytest.mark.parametrize("name", RM.GRID_CASES)
def test_more_chunks_than_workgroups(rh, name):
    """4.5 M pixels: more chunks of 2048 pixels than the grid has workgroups, so a workgroup runs its chunk loop twice (the sums
    accumulate across chunks; a palette of one tile stays staged, a larger one is staged again per chunk)."""
    import torch
    rgb, pal, cls, nc, want_idx, want_sums = RM.grid_case(name)
    chunks = -(-rgb.shape[0] * rgb.shape[1] // 2048)
    assert chunks > 8 * torch.cuda.get_device_properties(rh.device).multi_processor_count
    for eb in RM.index_bytes(len(pal)):
        rc, idx, sums = _raw_remap(rh, rgb, pal, cls, nc, eb)
        assert rc == 0, (name, eb)
        assert np.array_equal(idx, want_idx), (name, eb)
        assert np.array_equal(sums, want_sums), (name, eb)


def test_device_tensor_arguments(rh):
    rgb, pal, cls, nc, _ = RM.case("classes2")
    want_idx, want_sums = RM.reference("classes2")
    idx, sums = rh.palette_remap(rh.dev(rgb), rh.dev(pal), rh.dev(cls), nc)
    assert np.array_equal(_idx64(idx), want_idx) and np.array_equal(sums.cpu().numpy(), want_sums)
    idx, sums = rh.palette_remap(rh.dev(rgb), pal, rh.dev(cls == 1), 2)            # a bool map: classes 0 / 1
    _, want = RM.remap_reference(rgb, pal, (cls == 1).astype(np.uint8), 2)
    assert np.array_equal(sums.cpu().numpy(), want)
    with pytest.raises(ValueError, match="palette_remap: n_classes without a class map"):
        rh.palette_remap(rgb, pal, None, 2)
    with pytest.raises(ValueError, match="palette_remap: the class map must have one element per pixel"):
        rh.palette_remap(rgb, pal, cls[:-1], 2)
    with pytest.raises(TypeError, match=r"palette_remap: rgb must be uint8, got torch\.int32"):
        rh.palette_remap(rgb.astype(np.int32), pal)


@pytest.mark.parametrize("what,over,code", RM.ERRORS, ids=[e[0] for e in RM.ERRORS])
def test_device_argument_errors(rh, what, over, code):
    import torch
    t = {"rgb": rh.zeros((4, 3), torch.uint8), "palette": rh.zeros((3, 3), torch.uint8), "idx_out": rh.zeros((4,), torch.int32),
         "sums": rh.zeros((17, 2), torch.int64)}
    t.update({k: v for k, v in over.items() if k in t})
    cls = rh.zeros((4,), torch.uint8) if over.get("cls") else None
    rc = rh.lib.rhccq_palette_remap(rh.ctx, rh._p(t["rgb"]), over.get("n_pixels", 4), rh._p(t["palette"]), over.get("K", 3), rh._p(cls),
                                    over.get("n_classes", 0), rh._p(t["idx_out"]), over.get("idx_elem_bytes", 2), rh._p(t["sums"]))
    assert rc == code, what
    assert rh._raw.rhccq_last_error(rh.ctx).decode().startswith("palette_remap:")


def test_device_equals_host_form(rh):
    import ctypes as C
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (300, 301, 3)).astype(np.uint8)
    pal = rng.integers(0, 256, (1000, 3)).astype(np.uint8)
    cls = rng.integers(0, 3, (300, 301)).astype(np.uint8)
    h_idx, h_sums = np.zeros(300 * 301, np.uint16), np.zeros((3, 2), np.uint64)
    rc = rh._raw.rhccq_palette_remap_host(C.c_void_p(rgb.ctypes.data), rgb.size // 3, C.c_void_p(pal.ctypes.data), 1000,
                                          C.c_void_p(cls.ctypes.data), 2, C.c_void_p(h_idx.ctypes.data), 2, C.c_void_p(h_sums.ctypes.data))
    assert rc == 0
    idx, sums = rh.palette_remap(rgb, pal, cls, 2)
    assert np.array_equal(_idx64(idx), h_idx.astype(np.int64)) and np.array_equal(sums.cpu().numpy(), h_sums.astype(np.int64))
    assert h_sums[2, 0] == 300 * 301 and h_sums[0, 0] + h_sums[1, 0] < h_sums[2, 0]     # class 2 is in no row


# ---- a result of the encoder as the palette ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoded(enc, tmp_path_factory):
    """photo96 (96 x 128, synth.photo) encoded once: (image, result, the result's .rhccq file)"""
    (q1, q2), img, _ = RC.case("photo96")
    path = str(tmp_path_factory.mktemp("remap") / "key.rhccq")
    res = enc.encode(img, q1, q2, out_path=path, exact=True)
    assert tuple(res["top_left"]) == (0, 0) and tuple(res["shape"]) == img.shape[:2]
    return img, res, path


def _encoder_sse(rh, img, res):
    import torch
    every = rh.zeros(img.shape[:2], torch.uint8)
    row = rh.class_error_sums_indexed(rh.dev(img), res["indices"].reshape(-1), rh.dev(np.asarray(res["palette"], np.uint8).reshape(-1, 3)),
                                      every, 1)[0]
    assert int(row[5]) == img.shape[0] * img.shape[1]
    return int(row[0]) + int(row[1]) + int(row[2])


def test_remap_onto_own_palette_is_optimal(rh, enc, encoded):
    img, res, _ = encoded
    pal = np.asarray(res["palette"], np.uint8).reshape(-1, 3)
    want_idx, want_sums = RM.remap_reference(img, pal)
    out = enc.encode_with_palette(img, res)                                  # (a dict with "palette": the earlier result)
    row = out["stats"]["remap"]["all"]
    sse_encode = _encoder_sse(rh, img, res)
    assert row["sse"] == int(want_sums[-1, 1]) and row["pixels"] == img.shape[0] * img.shape[1]
    assert row["sse"] <= sse_encode
    assert row["psnr"] >= RM.psnr(sse_encode, row["pixels"]) and abs(row["psnr"] - RM.psnr(row["sse"], row["pixels"])) < 1e-9
    assert row["mse"] == row["sse"] / (3.0 * row["pixels"])
    assert np.array_equal(_idx64(out["indices"]), want_idx)
    assert tuple(out["indices"].shape) == img.shape[:2] and out["shape"] == img.shape[:2] and out["top_left"] == (0, 0)
    assert out["indices_dtype"] == ("uint8" if len(pal) <= 256 else "uint16") and np.array_equal(out["palette"], pal)
    assert list(out["stats"]["remap"]) == ["all"] and "quality" not in out["stats"] and list(out["stats"]["seconds"]) == ["remap"]
    decoded = rh.decode(out["indices"].reshape(-1), rh.dev(pal)).cpu().numpy().reshape(img.shape)
    assert np.array_equal(decoded, pal[want_idx].reshape(img.shape))


def test_decoded_picture_remaps_onto_itself(rh, enc, encoded):
    img, res, _ = encoded
    pal = np.asarray(res["palette"], np.uint8).reshape(-1, 3)
    decoded = pal[_idx64(res["indices"])].reshape(img.shape)
    out = enc.encode_with_palette(decoded, pal)
    assert out["stats"]["remap"]["all"]["sse"] == 0 and out["stats"]["remap"]["all"]["psnr"] == float("inf")
    idx = _idx64(out["indices"])
    assert np.array_equal(pal[idx].reshape(img.shape), decoded)
    keys = (pal[:, 0].astype(np.int64) << 16) | (pal[:, 1].astype(np.int64) << 8) | pal[:, 2]
    first = {}
    for j, k in enumerate(keys.tolist()):
        first.setdefault(k, j)
    px = decoded.reshape(-1, 3).astype(np.int64)
    assert idx.tolist() == [first[k] for k in ((px[:, 0] << 16) | (px[:, 1] << 8) | px[:, 2]).tolist()]


def test_container_round_trip(rh, enc, encoded, tmp_path):
    from decoder.uncompression.uncompression import decompress_color_quantization, load_compressed
    from encoder.compression.compression import lossless_compress_optimized, save_compressed
    from roibasedimagecompression_amd import container
    img, res, key_path = encoded
    frame = container.read_frame(key_path, rh)                               # device palette, as read from the key frame's file
    pal = frame["palette"].cpu().numpy()
    assert np.array_equal(pal, np.asarray(res["palette"], np.uint8).reshape(-1, 3))
    want_idx, _ = RM.remap_reference(img, pal)
    want_img = pal[want_idx].reshape(img.shape)
    path = str(tmp_path / "remap.rhccq")
    out = enc.encode_with_palette(img, frame, out_path=path, exact=True)
    assert "container" in out["stats"]["seconds"]
    back = container.read_frame(path, rh)
    assert np.array_equal(back["image"].cpu().numpy(), want_img) and np.array_equal(_idx64(back["indices"]), want_idx)
    assert np.array_equal(np.asarray(decompress_color_quantization(load_compressed(path))["image"], np.uint8).reshape(img.shape), want_img)
    host = str(tmp_path / "host.rhccq")
    save_compressed(lossless_compress_optimized(out["palette"], want_idx.astype(_NDT[out["indices"].element_size()]), out["shape"]), host)
    assert open(path, "rb").read() == open(host, "rb").read()


def test_roi_mask_rows_and_report(rh, enc, encoded):
    img, res, _ = encoded
    _, _, m = RC.case("photo96")
    pal = np.asarray(res["palette"], np.uint8).reshape(-1, 3)
    _, want = RM.remap_reference(img, pal, m.astype(np.uint8), 2)
    out = enc.encode_with_palette(img, pal, roi_mask=m, report=True)
    remap = out["stats"]["remap"]
    assert sorted(remap) == ["all", "nonroi", "roi"]
    for key, row in (("nonroi", want[0]), ("roi", want[1]), ("all", want[2])):
        assert (remap[key]["pixels"], remap[key]["sse"]) == (int(row[0]), int(row[1])), key
        assert abs(remap[key]["psnr"] - RM.psnr(int(row[1]), int(row[0]))) < 1e-9
    assert remap["roi"]["pixels"] == int(m.sum()) and remap["roi"]["pixels"] + remap["nonroi"]["pixels"] == remap["all"]["pixels"]
    quality = out["stats"]["quality"]
    assert list(quality) == ["nonroi", "roi", "all"] and out["stats"]["roi_source"] == "caller"
    for key in quality:
        assert quality[key]["pixel_count"] == remap[key]["pixels"]
        assert quality[key]["mse"] == np.float32(remap[key]["sse"] / (3.0 * remap[key]["pixels"])), key
        assert abs(float(quality[key]["psnr"]) - remap[key]["psnr"]) < 1e-9
    # a device mask gives the same rows; without a mask only "all", and the report uses the detector's map
    import torch
    again = enc.encode_with_palette(torch.from_numpy(np.array(img)).to(rh.device), rh.dev(pal), roi_mask=rh.dev(m.astype(np.uint8) * 255))
    assert again["stats"]["remap"] == remap and "quality" not in again["stats"]
    with pytest.raises(ValueError):
        enc.encode_with_palette(img, pal, roi_mask=m[:-1])
    with pytest.raises(ValueError):
        enc.encode_with_palette(img, np.zeros((0, 3), np.uint8))


# ---- sequences ----------------------------------------------------------------------------------------------------------------------
def _same_result(a, b):
    return (np.array_equal(np.asarray(a["palette"]), np.asarray(b["palette"])) and a["indices"].dtype == b["indices"].dtype
            and np.array_equal(a["indices"].cpu().numpy(), b["indices"].cpu().numpy()) and tuple(a["shape"]) == tuple(b["shape"])
            and tuple(a["top_left"]) == tuple(b["top_left"]) and a["indices_dtype"] == b["indices_dtype"])


def test_encode_sequence(rh, enc, tmp_path):
    """Frames [A, A with a 6 x 6 patch brightened by 1, B, B] (tests/remap_cases.py: A red only, B green and blue only), qualities
    (20, 10), max_drop_db = 3.  The choice was confirmed with oracle.rhccq_oracle.script_flow on the CPU before the inputs were
    fixed: encode(A) has 85 colours and 52.81 dB; the reference remap onto that palette gives 56.61 dB for A, 56.62 dB for frame 1
    (kept: 6.8 dB above the bound) and 6.50 dB for B, 43.3 dB under the bound of 49.81 dB, so frame 2 re-keys; encode(B) has 98
    colours and 39.40 dB, the remap of frame 3 onto it 40.51 dB (kept, as the optimality property guarantees)."""
    frames = RM.sequence_frames()
    q1, q2 = RM.SEQ_QUALITIES
    drop = RM.SEQ_MAX_DROP_DB
    paths = [str(tmp_path / f"f{i}.rhccq") for i in range(4)]
    gen = enc.encode_sequence(frames, q1, q2, drop, out_paths=paths, exact=True)
    assert iter(gen) is gen                                                    # a generator: nothing is encoded before it is asked
    results = list(gen)
    assert len(results) == 4
    with pytest.raises(TypeError):
        enc.encode_sequence(frames, q1, q2)                                    # max_drop_db has no default
    first = results[0]
    assert first["stats"]["key_frame"] is True and first["stats"]["key_index"] == 0
    assert _same_result(first, enc.encode(frames[0], q1, q2))
    key, key_psnr, key_index = first, RM.psnr(_encoder_sse(rh, frames[0], first), 96 * 128), 0
    remaps = rekeys = 0
    for i in range(1, 4):
        res, st = results[i], results[i]["stats"]
        pal = np.asarray(key["palette"], np.uint8).reshape(-1, 3)
        want_idx, want_sums = RM.remap_reference(frames[i], pal)
        ref_psnr = RM.psnr(int(want_sums[-1, 1]), int(want_sums[-1, 0]))
        assert abs(ref_psnr - (key_psnr - drop)) > 1e-6                        # (not a tie of the rule itself)
        if st["key_frame"]:
            rekeys += 1
            assert ref_psnr < key_psnr - drop, i
            assert st["key_index"] == i and _same_result(res, enc.encode(frames[i], q1, q2)), i
            assert tuple(res["top_left"]) == (0, 0) and tuple(res["shape"]) == (96, 128)
            key, key_psnr, key_index = res, RM.psnr(_encoder_sse(rh, frames[i], res), 96 * 128), i
        else:
            remaps += 1
            assert ref_psnr >= key_psnr - drop, i
            assert st["key_index"] == key_index and np.array_equal(_idx64(res["indices"]), want_idx), i
            assert np.array_equal(res["palette"], pal) and st["remap"]["all"]["sse"] == int(want_sums[-1, 1])
            assert abs(st["psnr"] - ref_psnr) < 1e-9 and abs(st["key_psnr"] - key_psnr) < 1e-9
    assert remaps >= 1 and rekeys >= 1
    assert [r["stats"]["key_frame"] for r in results] == [True, False, True, False]
    assert [r["stats"]["key_index"] for r in results] == [0, 0, 2, 2]
    # every frame's file decodes to the frame's own result
    from roibasedimagecompression_amd import container
    for res, path in zip(results, paths):
        back = container.read_frame(path, rh)
        assert np.array_equal(_idx64(back["indices"]), _idx64(res["indices"])) and np.array_equal(back["palette"].cpu().numpy(), res["palette"])
