"""The exact row segmentation on the device (csrc/palette_segment.hip, Rhccq.palette_segment, the run_penalty keyword of
ImageEncoder.encode_with_palette / encode / encode_sequence) against the numpy reference of tests/segment_cases.py, bit for bit, and what
the encoder builds on it: the statistics, the last-step rule, the container round trip, the byte target.  GPU only."""
import numpy as np
import pytest

import remap_cases as RM
import roimask_cases as RC
import segment_cases as SG

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


def _raw_segment(rh, rgb, pal, cls, n_classes, penalty, elem_bytes, work="garbage", K=None):
    """rhccq_palette_segment itself, in the element width asked for; the outputs and the workspace are pre-filled, so that unwritten
    elements show and nothing depends on what the workspace held.  work: "garbage", None (NULL), "odd" (off its alignment) or "short"."""
    import ctypes as C
    import torch
    H, W = rgb.shape[:2]
    d_rgb, d_pal = rh.dev(np.ascontiguousarray(rgb)), rh.dev(np.ascontiguousarray(pal).reshape(-1, 3))
    d_cls = None if cls is None else rh.dev(np.ascontiguousarray(cls).reshape(-1))
    table = SG.penalty_table(penalty, n_classes)
    tarr = (C.c_uint32 * len(table))(*table)
    K = int(d_pal.shape[0]) if K is None else K
    nbytes = int(rh.lib.rhccq_palette_segment_bytes(H, W, min(K, SG.CAP)))
    buf = torch.full((nbytes + 16,), 0xA7, dtype=torch.uint8, device=rh.device)
    assert buf.data_ptr() % 8 == 0
    ptr, given = buf.data_ptr(), nbytes
    if work is None:
        ptr = 0
    elif work == "odd":
        ptr += 4
    elif work == "short":
        given = nbytes - 1
    idx = torch.full((H, W), 0x2B, dtype=getattr(torch, _TDT[elem_bytes]), device=rh.device)
    sums = torch.full((n_classes + 1, 4), 0x5555, dtype=torch.int64, device=rh.device)
    rc = rh.lib.rhccq_palette_segment(rh.ctx, rh._p(d_rgb), H, W, rh._p(d_pal), K, rh._p(d_cls), n_classes, C.cast(tarr, C.c_void_p),
                                      C.c_void_p(ptr), given, rh._p(idx), elem_bytes, rh._p(sums))
    return rc, _idx64(idx), sums.cpu().numpy()


@pytest.mark.parametrize("name", SG.names())
def test_device_equals_reference(rh, name):
    import torch
    rgb, pal, cls, nc, penalty, _ = SG.case(name)
    want_out, want_sums, _ = SG.reference(name)
    for eb in SG.index_bytes(len(pal)):
        rc, out, sums = _raw_segment(rh, rgb, pal, cls, nc, penalty, eb)
        assert rc == 0, (name, eb)
        assert np.array_equal(out, want_out), (name, eb)
        assert np.array_equal(sums, want_sums), (name, eb)
    # the Python surface: numpy arguments, the repository's index storage, the picture's shape kept
    idx, sums = rh.palette_segment(rgb, pal, penalty, cls, nc)
    assert idx.dtype == (torch.uint8 if len(pal) <= 256 else torch.int16) and tuple(idx.shape) == tuple(rgb.shape[:2])
    assert sums.dtype == torch.int64 and idx.is_cuda and sums.is_cuda
    assert np.array_equal(_idx64(idx), want_out) and np.array_equal(sums.cpu().numpy(), want_sums), name


def test_the_cap_is_accepted_and_one_more_is_not(rh):
    from roibasedimagecompression_amd import ops
    from roibasedimagecompression_amd.ops import RhccqError
    assert ops.palette_segment_max_rows() == SG.CAP and len(SG.case(f"K{SG.CAP}")[1]) == SG.CAP      # (test_device_equals_reference runs it)
    rng = np.random.default_rng(2)
    pal = RM._palette(rng, SG.CAP + 1)
    rgb = SG.RN._image(rng, pal, 2, 9)
    rc, _, _ = _raw_segment(rh, rgb, pal, None, 0, 5, 2)
    assert rc == SG.E_LIMIT and rh._raw.rhccq_last_error(rh.ctx).decode().startswith("palette_segment:")
    with pytest.raises(RhccqError):
        rh.palette_segment(rgb, pal, 5)


def test_larger_penalty_never_more_breaks_nor_less_error(rh):
    SG.check_monotone(lambda rgb, pal, p: _idx64(rh.palette_segment(rgb, pal, p)[0]))


def test_python_surface_arguments(rh):
    rgb, pal, cls, nc, penalty, _ = SG.case("classes2")
    want_out, want_sums, _ = SG.reference("classes2")
    idx, sums = rh.palette_segment(rh.dev(rgb), rh.dev(pal), penalty, rh.dev(cls), nc)
    assert np.array_equal(_idx64(idx), want_out) and np.array_equal(sums.cpu().numpy(), want_sums)
    idx, sums = rh.palette_segment(np.zeros((0, 5, 3), np.uint8), pal, 7)
    assert tuple(idx.shape) == (0, 5) and sums.cpu().numpy().tolist() == [[0, 0, 0, 0]]
    for bad, msg in ((lambda: rh.palette_segment(rgb, pal, penalty, None, 2), "n_classes without a class map"),
                     (lambda: rh.palette_segment(rgb, pal, [1, 2], cls, 2), r"penalty is one integer or n_classes \+ 1 of them"),
                     (lambda: rh.palette_segment(rgb, pal, SG.MAX_PENALTY + 1), r"a penalty must be 0\.\.16777215"),
                     (lambda: rh.palette_segment(rgb, pal, -1), r"a penalty must be 0\.\.16777215"),
                     (lambda: rh.palette_segment(rgb.reshape(-1, 3), pal, 0), r"rgb \[H, W, 3\] and palette \[K, 3\] are expected"),
                     (lambda: rh.palette_segment(rgb, pal, penalty, cls[:-1], 2), "the class map must have one element per pixel")):
        with pytest.raises(ValueError, match="palette_segment: " + msg):
            bad()
    with pytest.raises(TypeError, match=r"palette_segment: rgb must be uint8, got torch\.int32"):
        rh.palette_segment(rgb.astype(np.int32), pal, 0)


@pytest.mark.parametrize("what,over,code", SG.ERRORS + SG.DEVICE_ERRORS, ids=[e[0] for e in SG.ERRORS + SG.DEVICE_ERRORS])
def test_device_argument_errors(rh, what, over, code):
    import ctypes as C
    import torch
    t = {"rgb": rh.zeros((4, 3), torch.uint8), "palette": rh.zeros((3, 3), torch.uint8), "idx_out": rh.zeros((4,), torch.int32),
         "sums": rh.zeros((18, 4), torch.int64)}
    t.update({k: v for k, v in over.items() if k in t})
    cls = rh.zeros((4,), torch.uint8) if over.get("cls") else None
    penalty = over.get("penalty", [5])
    tarr = None if penalty is None else (C.c_uint32 * len(penalty))(*penalty)
    nbytes = int(rh.lib.rhccq_palette_segment_bytes(2, 2, 3))
    buf = rh.zeros((nbytes + 16,), torch.uint8)
    work = over.get("work", "ok")
    ptr = 0 if work is None else buf.data_ptr() + (4 if work == "odd" else 0)
    rc = rh.lib.rhccq_palette_segment(rh.ctx, rh._p(t["rgb"]), over.get("H", 2), over.get("W", 2), rh._p(t["palette"]), over.get("K", 3), rh._p(cls),
                                      over.get("n_classes", 0), C.cast(tarr, C.c_void_p) if tarr is not None else C.c_void_p(0), C.c_void_p(ptr),
                                      nbytes - (1 if work == "short" else 0), rh._p(t["idx_out"]), over.get("idx_elem_bytes", 2), rh._p(t["sums"]))
    assert rc == code, what
    assert rh._raw.rhccq_last_error(rh.ctx).decode().startswith("palette_segment:")


def test_the_valid_call_the_errors_vary_succeeds(rh):
    rc, out, sums = _raw_segment(rh, np.zeros((2, 2, 3), np.uint8), np.zeros((3, 3), np.uint8), None, 0, [5], 2)
    assert rc == 0 and out.tolist() == [[0, 0], [0, 0]] and sums.tolist() == [[4, 0, 0, 0]]


# ---- ImageEncoder.encode_with_palette(run_penalty=) -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def photo():
    """roimask_cases' photo96 (96 x 128), its mask, and 300 of its pixels as the palette (2-byte indices; colours=64 gives 1-byte ones)"""
    _, img, mask = RC.case("photo96")
    flat = img.reshape(-1, 3)
    pal = flat[np.random.default_rng(9).choice(len(flat), 300, replace=False)].copy()
    return img, mask, pal


def _check_result(res, img, mask, run_penalty):
    """the result's indices and statistics against the reference over the RETURNED palette"""
    pal = np.asarray(res["palette"], np.uint8).reshape(-1, 3)
    if mask is None:
        want_out, want_sums, _ = SG.segment_reference(img, pal, run_penalty)
        rows = {"all": want_sums[0]}
    else:
        table = [run_penalty["nonroi"], run_penalty["roi"], min(run_penalty.values())] if isinstance(run_penalty, dict) else [run_penalty] * 3
        want_out, want_sums, _ = SG.segment_reference(img, pal, table, mask.astype(np.uint8), 2)
        rows = {"nonroi": want_sums[0], "roi": want_sums[1], "all": want_sums[2]}
    assert np.array_equal(_idx64(res["indices"]), want_out)
    assert res["indices_dtype"] == ("uint8" if len(pal) <= 256 else "uint16") and tuple(res["indices"].shape) == img.shape[:2]
    st = res["stats"]
    assert sorted(st["remap"]) == sorted(rows)
    for n, row in rows.items():
        assert (st["remap"][n]["pixels"], st["remap"][n]["sse"]) == (int(row[0]), int(row[1])), n
        assert abs(st["remap"][n]["psnr"] - RM.psnr(int(row[1]), int(row[0]))) < 1e-9
    assert st["runs"] == {"penalty": run_penalty, "carried": {n: int(row[2]) for n, row in rows.items()},
                          "breaks": {n: int(row[3]) for n, row in rows.items()}, "pixels": img.shape[0] * img.shape[1]}
    return want_out, want_sums


@pytest.mark.parametrize("masked,run_penalty", [(False, 150), (True, 150), (True, {"roi": 20, "nonroi": 900}), (False, 0)])
def test_encode_with_palette_run_penalty(enc, photo, masked, run_penalty):
    img, mask, pal = photo
    mask = mask if masked else None
    res = enc.encode_with_palette(img, pal, roi_mask=mask, run_penalty=run_penalty)
    _, want_sums = _check_result(res, img, mask, run_penalty)
    assert np.array_equal(res["palette"], pal)
    plain = enc.encode_with_palette(img, pal, roi_mask=mask)
    assert "runs" not in plain["stats"] and plain["stats"]["remap"]["all"]["sse"] <= res["stats"]["remap"]["all"]["sse"]
    if run_penalty == 0:
        assert plain["stats"]["remap"] == res["stats"]["remap"]                 # penalty 0 keeps the squared error, ties aside the indices too
    else:
        assert want_sums[-1, 2] > 0 and not np.array_equal(_idx64(plain["indices"]), _idx64(res["indices"]))


def test_run_penalty_arguments(enc, photo):
    img, mask, pal = photo
    for kw in ({"run_penalty": {"roi": 1, "nonroi": 2}}, {"run_penalty": {"roi": 1}, "roi_mask": mask}, {"run_penalty": -1},
               {"run_penalty": SG.MAX_PENALTY + 1}, {"run_penalty": {"roi": 1, "nonroi": SG.MAX_PENALTY + 1}, "roi_mask": mask},
               {"run_penalty": 5, "run_slack": 5}, {"run_penalty": 0, "run_slack": 0}, {"run_penalty": 5, "target_psnr": 30.0},
               {"run_penalty": 5, "target_psnr": {"roi": 30.0}, "roi_mask": mask}):
        with pytest.raises(ValueError):
            enc.encode_with_palette(img, pal, **kw)
    (q1, q2), _, _ = RC.case("photo96")
    for kw in ({"run_penalty": 5, "run_slack": 5}, {"run_penalty": 5, "target_psnr": 30.0}):
        with pytest.raises(ValueError):
            enc.encode(img, q1, q2, **kw)
    for kw in ({"run_penalty": {"roi": 1, "nonroi": 2}}, {"run_penalty": 5, "run_slack": 5}, {"run_penalty": 5, "target_psnr": 30.0}):
        with pytest.raises(ValueError):
            next(enc.encode_sequence([img, img], 20, 10, 3.0, **kw))


def test_a_palette_above_the_cap_raises(enc, photo):
    from roibasedimagecompression_amd.ops import RhccqError
    img, _, _ = photo
    pal = RM._palette(np.random.default_rng(4), SG.CAP + 1)
    with pytest.raises(RhccqError):
        enc.encode_with_palette(img, pal, run_penalty=10)


def test_segmentation_is_the_last_step(enc, photo):
    """colours= and refine= run first, on the nearest-row assignment; the palette and their statistics are those of the call without a penalty"""
    img, mask, pal = photo
    penalty = {"roi": 60, "nonroi": 600}
    res = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=3, colours=64, refine=2, run_penalty=penalty)
    plain = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=3, colours=64, refine=2)
    assert np.array_equal(res["palette"], plain["palette"]) and len(res["palette"]) == 64
    assert res["stats"]["reduce"] == plain["stats"]["reduce"] and res["stats"]["refine"] == plain["stats"]["refine"]
    _check_result(res, img, mask, penalty)


def test_container_round_trip(rh, enc, photo, tmp_path):
    import os
    from roibasedimagecompression_amd import container
    img, mask, pal = photo
    path = str(tmp_path / "segment.rhccq")
    res = enc.encode_with_palette(img, pal, run_penalty=200, out_path=path, exact=True)
    want_out, _ = _check_result(res, img, None, 200)
    back = container.read_frame(path, rh)
    assert np.array_equal(_idx64(back["indices"]).reshape(want_out.shape), want_out) and np.array_equal(back["palette"].cpu().numpy(), pal)
    assert np.array_equal(back["image"].cpu().numpy().reshape(img.shape), pal[want_out])
    plain = str(tmp_path / "plain.rhccq")
    enc.encode_with_palette(img, pal, out_path=plain, exact=True)
    print("bytes", os.path.getsize(plain), "->", os.path.getsize(path))
    assert os.path.getsize(path) < os.path.getsize(plain)


@pytest.mark.parametrize("exact", [True, False])
def test_target_bytes_probes_run_with_the_penalty(rh, enc, photo, tmp_path, exact):
    import os
    from roibasedimagecompression_amd import container
    img, _, pal = photo
    penalty = 120
    full = len(container.frame_bytes(enc.encode_with_palette(img, pal, run_penalty=penalty), rh, exact=exact))
    out = str(tmp_path / "t.rhccq")
    res = enc.encode_with_palette(img, pal, target_bytes=int(full * 0.6), run_penalty=penalty, exact=exact, out_path=out)
    tg = res["stats"]["target"]
    assert tg["kind"] == "bytes" and tg["met"] is True and len(tg["probes"]) > 1
    for k, size in tg["probes"]:
        again = enc.encode_with_palette(img, pal, colours=k, run_penalty=penalty)
        assert size == len(container.frame_bytes(again, rh, exact=exact)), k
        if k == tg["colours"]:
            assert np.array_equal(again["palette"], res["palette"]) and np.array_equal(_idx64(again["indices"]), _idx64(res["indices"]))
            assert again["stats"]["runs"] == res["stats"]["runs"] and again["stats"]["remap"] == res["stats"]["remap"]
    assert os.path.getsize(out) == dict(tg["probes"])[tg["colours"]] <= int(full * 0.6)
    # the recorded bound is a valid one: two penalties a pixel on top of the rung's curve
    assert res["stats"]["remap"]["all"]["psnr"] >= tg["bound_psnr"]["all"]
    _check_result(res, img, None, penalty)


# ---- ImageEncoder.encode(run_penalty=) and encode_sequence ------------------------------------------------------------------------------
def _same_result(a, b):
    return (np.array_equal(np.asarray(a["palette"]), np.asarray(b["palette"])) and a["indices"].dtype == b["indices"].dtype
            and np.array_equal(a["indices"].cpu().numpy(), b["indices"].cpu().numpy()) and tuple(a["shape"]) == tuple(b["shape"])
            and tuple(a["top_left"]) == tuple(b["top_left"]) and a["indices_dtype"] == b["indices_dtype"])


def test_encode_run_penalty(rh, enc, tmp_path):
    from roibasedimagecompression_amd import container
    (q1, q2), img, mask = RC.case("photo96")
    base = enc.encode(img, q1, q2, roi_mask=mask)
    none = enc.encode(img, q1, q2, roi_mask=mask, run_penalty=None)
    assert _same_result(base, none) and "runs" not in none["stats"]
    assert tuple(base["top_left"]) == (0, 0) and tuple(base["shape"]) == img.shape[:2]
    pal = np.asarray(base["palette"], np.uint8).reshape(-1, 3)
    cls = enc.region_map.cpu().numpy().astype(np.uint8)                        # the map the encoder made of the mask: 1 inside, 0 outside
    for run_penalty in (90, {"roi": 10, "nonroi": 400}):
        path = str(tmp_path / "e.rhccq")
        res = enc.encode(img, q1, q2, roi_mask=mask, run_penalty=run_penalty, out_path=path, exact=True)
        assert np.array_equal(np.asarray(res["palette"], np.uint8).reshape(-1, 3), pal)
        table = [run_penalty["nonroi"], run_penalty["roi"], min(run_penalty.values())] if isinstance(run_penalty, dict) else [run_penalty] * 3
        want_out, want_sums, _ = SG.segment_reference(img, pal, table, cls, 2)
        assert np.array_equal(_idx64(res["indices"]).reshape(want_out.shape), want_out)
        assert tuple(res["indices"].shape) == tuple(base["indices"].shape) and res["indices"].dtype == base["indices"].dtype
        assert res["stats"]["runs"] == {"penalty": run_penalty,
                                        "carried": {"all": int(want_sums[2, 2]), "roi": int(want_sums[1, 2]), "nonroi": int(want_sums[0, 2])},
                                        "breaks": {"all": int(want_sums[2, 3]), "roi": int(want_sums[1, 3]), "nonroi": int(want_sums[0, 3])},
                                        "pixels": img.shape[0] * img.shape[1]}
        assert want_sums[2, 2] > 0
        back = container.read_frame(path, rh)
        assert np.array_equal(_idx64(back["indices"]).reshape(want_out.shape), want_out)


def test_encode_sequence_forwards_the_penalty(enc):
    frames = RM.sequence_frames()[:2]                                          # a key frame and a frame that is remapped onto it
    q1, q2 = RM.SEQ_QUALITIES
    results = list(enc.encode_sequence(frames, q1, q2, RM.SEQ_MAX_DROP_DB, run_penalty=50))
    assert [r["stats"]["key_frame"] for r in results] == [True, False]
    assert _same_result(results[0], enc.encode(frames[0], q1, q2, run_penalty=50)) and results[0]["stats"]["runs"]["penalty"] == 50
    pal = np.asarray(results[0]["palette"], np.uint8).reshape(-1, 3)
    want_out, want_sums, _ = SG.segment_reference(frames[1], pal, 50)
    assert np.array_equal(_idx64(results[1]["indices"]), want_out)
    assert results[1]["stats"]["runs"] == {"penalty": 50, "carried": {"all": int(want_sums[0, 2])}, "breaks": {"all": int(want_sums[0, 3])},
                                           "pixels": 96 * 128}


# ---- the value claim on the device path ---------------------------------------------------------------------------------------------------
def test_kodak_22_equals_reference(rh):
    """the device index map is the reference's, so the 0.93 x bytes / no-more-error condition of tests/test_palette_segment_cpu.py holds for it"""
    img, pal, b, out, sums, greedy, greedy_sums = SG.kodak()
    idx, got = rh.palette_segment(img, pal, SG.KODAK_PENALTY)
    assert np.array_equal(_idx64(idx), out) and np.array_equal(got.cpu().numpy(), sums)
    assert SG.index_bytes_zlib9(_idx64(idx)) <= SG.KODAK_MAX_BYTES_RATIO * SG.index_bytes_zlib9(greedy)
    assert int(got[-1, 1]) <= int(greedy_sums[-1, 1])
