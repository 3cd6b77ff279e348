"""The palette reduction on the device (csrc/palette_reduce.hip, Rhccq.palette_reduce) against the numpy reference of
tests/reduce_cases.py, bit for bit (palette, counts, map, merges, k_out), and what is built on it:
ImageEncoder.encode_with_palette(colours=N), ImageEncoder.encode(max_colours=N), encode_sequence(max_colours=N) and
container.reduce_frame.  GPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import reduce_cases as RD
import refine_cases as RF
import remap_cases as RM

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


@pytest.fixture(scope="module")
def enc(rh):
    from roibasedimagecompression_amd.image import ImageEncoder
    return ImageEncoder(rh)


class _Raw:
    """one call of rhccq_palette_reduce itself: output buffers and the workspace pre-filled so that unwritten elements show; nothing
    is read back before `read`"""

    def __init__(self, rh, pal, counts, target, work=None, merges=True):
        import torch
        self.rh = rh
        self.pal = rh.dev(np.ascontiguousarray(pal, np.uint8).reshape(-1, 3))
        self.counts = rh.dev(np.ascontiguousarray(counts, np.uint64).view(np.int64))
        self.K, self.target = int(self.pal.shape[0]), int(target)
        self.wbytes = int(rh._raw.rhccq_palette_reduce_bytes(self.K))
        self.work = work if work is not None else torch.full((self.wbytes // 8,), 0x3333, dtype=torch.int64, device=rh.device)
        self.pal_out = torch.full((self.target, 3), 0x55, dtype=torch.uint8, device=rh.device)
        self.cnt_out = torch.full((self.target,), 0x5555, dtype=torch.int64, device=rh.device)
        self.map = torch.full((self.K,), -7, dtype=torch.int32, device=rh.device)
        self.merges = torch.full((max(self.K - 1, 1), 2), -7, dtype=torch.int32, device=rh.device) if merges else None
        self.k_out = torch.full((1,), -7, dtype=torch.int32, device=rh.device)

    def launch(self):
        rh = self.rh
        return rh.lib.rhccq_palette_reduce(rh.ctx, rh._p(self.pal), rh._p(self.counts), self.K, self.target, rh._p(self.work), self.wbytes,
                                           rh._p(self.pal_out), rh._p(self.cnt_out), rh._p(self.map), rh._p(self.merges), rh._p(self.k_out))

    def read(self):
        merges = None if self.merges is None else self.merges.cpu().numpy()[:self.K - 1]
        return self.pal_out.cpu().numpy(), self.cnt_out.cpu().numpy(), self.map.cpu().numpy(), merges, int(self.k_out.item())


def _same(got, want, what):
    pal, cnt, map_, merges, k = got
    want_pal, want_cnt, want_map, want_merges, want_k = want
    assert k == want_k, (what, k, want_k)
    if merges is not None:
        assert np.array_equal(merges, want_merges), (what, merges[:8].tolist(), want_merges[:8].tolist())
    assert np.array_equal(pal, want_pal) and np.array_equal(cnt, want_cnt) and np.array_equal(map_, want_map), what


@pytest.mark.parametrize("name", RD.names(device=True))
def test_device_equals_reference(rh, name):
    c, want = RD.case(name), RD.reference(name)
    raw = _Raw(rh, c["pal"], c["counts"], c["target"])
    assert raw.launch() == 0, name
    _same(raw.read(), want, name)                                              # the whole buffers: zero rows and -1 steps behind the result
    pal, cnt, map_, merges = rh.palette_reduce(c["pal"], c["counts"], c["target"])
    k, steps = want[4], int((want[3][:, 0] >= 0).sum())
    assert pal.shape == (k, 3) and cnt.shape == (k,) and merges.shape == (steps, 2) and map_.shape == (len(c["pal"]),)
    _same((pal.cpu().numpy(), cnt.cpu().numpy(), map_.cpu().numpy(), None, k), (want[0][:k], want[1][:k], want[2], None, k), name)
    assert np.array_equal(merges.cpu().numpy(), want[3][:steps]), name


def test_without_merges(rh):
    c, want = RD.case("K257"), RD.reference("K257")
    raw = _Raw(rh, c["pal"], c["counts"], c["target"], merges=False)
    assert raw.launch() == 0
    _same(raw.read(), want, "merges == NULL")


def test_back_to_back_without_a_sync(rh):
    """three reductions queued on the stream and nothing read in between: the second has buffers of its own, the third runs in the
    first one's workspace (stream order is what keeps it from the first)"""
    a, b, c = RD.case("K300_to_16"), RD.case("K1025_distinct"), RD.case("K257")
    ra = _Raw(rh, a["pal"], a["counts"], a["target"])
    rb = _Raw(rh, b["pal"], b["counts"], b["target"])
    rc = _Raw(rh, c["pal"], c["counts"], c["target"], work=ra.work)
    assert rc.wbytes <= ra.wbytes
    assert ra.launch() == 0 and rb.launch() == 0 and rc.launch() == 0
    _same(ra.read(), RD.reference("K300_to_16"), "first")
    _same(rb.read(), RD.reference("K1025_distinct"), "second")
    _same(rc.read(), RD.reference("K257"), "third")


def _error_call(rh, over):
    """the valid call of reduce_cases.ERRORS with `over` applied, on device buffers -> (return code, the _Raw)"""
    import torch
    K = RD.ERROR_K
    raw = _Raw(rh, np.arange(3 * K, dtype=np.uint8).reshape(K, 3), over.get("counts", [1, 2, 3]), 4)    # room for K_target = K + 1
    raw.work = torch.full((raw.wbytes // 8 + 1,), 0x3333, dtype=torch.int64, device=rh.device)
    raw.cnt_out = torch.full((6,), 0x5555, dtype=torch.int64, device=rh.device)
    raw.map = torch.full((K + 1,), -7, dtype=torch.int32, device=rh.device)
    raw.merges = torch.full((K, 2), -7, dtype=torch.int32, device=rh.device)
    raw.k_out = torch.full((2,), -7, dtype=torch.int32, device=rh.device)
    raw.counts = torch.cat([raw.counts, torch.zeros(1, dtype=torch.int64, device=rh.device)])
    names = {"palette": "pal", "counts_buf": "counts", "palette_out": "pal_out", "counts_out": "cnt_out", "map": "map", "merges": "merges",
             "k_out": "k_out", "work": "work"}
    ptr = {}
    for key, attr in names.items():
        t = getattr(raw, attr)
        off = 0
        if over.get("misalign") == key:
            off = 1 if key in ("counts_buf", "counts_out", "work") else 2
        ptr[key] = C.c_void_p(0) if key in over and over[key] is None else C.c_void_p(t.data_ptr() + off)
    raw.target = over.get("K_target", 2)
    code = rh.lib.rhccq_palette_reduce(rh.ctx, ptr["palette"], ptr["counts_buf"], over.get("K", K), raw.target, ptr["work"],
                                       raw.wbytes - (1 if over.get("work_short") else 0), ptr["palette_out"], ptr["counts_out"], ptr["map"],
                                       ptr["merges"], ptr["k_out"])
    return code, raw


_ARG_ERRORS = [e for e in RD.ERRORS if e[3] != "data"]
_DATA_ERRORS = [e for e in RD.ERRORS if e[3] == "data"]


@pytest.mark.parametrize("what,over,code", [e[:3] for e in _ARG_ERRORS], ids=[e[0] for e in _ARG_ERRORS])
def test_device_argument_errors(rh, what, over, code):
    from roibasedimagecompression_amd import RhccqError
    got, raw = _error_call(rh, over)
    assert got == code, what
    rh.sync()
    assert int(raw.k_out[0].item()) == -7 and (raw.map.cpu().numpy() == -7).all(), what      # nothing was launched
    with pytest.raises(RhccqError):
        rh._check(got, "palette_reduce")


@pytest.mark.parametrize("what,over,code", [e[:3] for e in _DATA_ERRORS], ids=[e[0] for e in _DATA_ERRORS])
def test_device_data_errors_come_back_through_k_out(rh, what, over, code):
    """all counts zero, or their sum above 2^32 - 1: the host never reads the counts, so the call returns 0, *k_out holds the code
    and the outputs are zero (map and merges -1); Rhccq.palette_reduce raises from it"""
    from roibasedimagecompression_amd import RhccqError
    got, raw = _error_call(rh, over)
    assert got == 0, what
    rh.sync()
    K = RD.ERROR_K
    assert int(raw.k_out[0].item()) == code and int(raw.k_out[1].item()) == -7, what
    assert not raw.pal_out.cpu().numpy()[:raw.target].any() and not raw.cnt_out.cpu().numpy()[:raw.target].any(), what
    assert (raw.map.cpu().numpy()[:K] == -1).all() and (raw.merges.cpu().numpy()[:K - 1] == -1).all(), what
    with pytest.raises(RhccqError):
        rh.palette_reduce(np.zeros((K, 3), np.uint8), np.array(over["counts"], np.uint64), 2)


@pytest.mark.parametrize("what,over", RD.ACCEPTED, ids=[a[0] for a in RD.ACCEPTED])
def test_device_accepts(rh, what, over):
    got, raw = _error_call(rh, over)
    assert got == 0, what
    rh.sync()
    assert int(raw.k_out[0].item()) == over.get("K_target", 2), what


def test_more_rows_than_the_cap_raise_and_name_it(rh):
    from roibasedimagecompression_amd import RhccqError, ops
    assert ops.palette_reduce_max_rows() == RD.CAP
    with pytest.raises(RhccqError, match=str(RD.CAP)):
        rh.palette_reduce(np.zeros((RD.CAP + 1, 3), np.uint8), np.ones(RD.CAP + 1, np.int64), 2)


# ---- encode_with_palette(colours=N) ---------------------------------------------------------------------------------------------------
def _photo_case():
    from roibasedimagecompression_amd import synth
    img = synth.photo(96, 128, 7)
    flat = img.reshape(-1, 3)
    pal = flat[np.random.default_rng(5).choice(len(flat), 300, replace=False)].copy()
    pal[17] = pal[3]                                                           # a duplicate row: no pixel goes to it
    mask = np.zeros((96, 128), bool)
    mask[20:70, 30:100] = True
    return img, pal, mask


def _composition(img, pal, mask, roi_weight, colours, refine):
    """remap_reference -> bincount -> reduce_reference -> refine_reference -> remap_reference"""
    first, _ = RM.remap_reference(img, pal)
    w = np.ones(first.shape, np.int64) if mask is None else np.where(mask.reshape(-1), roi_weight, 1).astype(np.int64)
    counts = np.bincount(first, weights=w, minlength=len(pal)).astype(np.int64)
    red, _, _, merges, k = RD.reduce_reference(pal, counts, min(colours, len(pal)))
    red = red[:k]
    hist, nit = None, 0
    if refine:
        cls = None if mask is None else mask.astype(np.uint8)
        red, hist, nit = RF.refine_reference(img, red, cls, None if mask is None else [1, roi_weight, 1], max_iter=refine)
    idx, sums = RM.remap_reference(img, red)
    row = {"from": len(pal), "to": k, "empty": int((counts == 0).sum()), "steps": int((merges[:, 0] >= 0).sum())}
    return red, idx, sums, row, hist, nit


@pytest.mark.parametrize("masked,refine,colours", [(False, 0, 256), (False, 2, 256), (True, 0, 256), (True, 2, 256), (True, 2, 16)])
def test_encode_with_palette_colours(enc, masked, refine, colours):
    img, pal, mask = _photo_case()
    mask = mask if masked else None
    roi_weight = 7 if masked else 1
    want_pal, want_idx, want_sums, want_row, want_hist, want_nit = _composition(img, pal, mask, roi_weight, colours, refine)
    res = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=roi_weight, refine=refine, colours=colours)
    assert res["stats"]["reduce"] == want_row and want_row["to"] == colours and want_row["empty"] >= 1, (res["stats"]["reduce"], want_row)
    assert np.array_equal(np.asarray(res["palette"]), want_pal)
    assert res["indices"].shape == (96, 128) and np.array_equal(res["indices"].cpu().numpy().astype(np.int64).reshape(-1) & 0xFFFF, want_idx)
    assert res["stats"]["remap"]["all"]["sse"] == int(want_sums[-1, 1])
    if refine:
        assert res["stats"]["refine"]["iterations"] == want_nit and res["stats"]["refine"]["sse"] == [int(v) for v in want_hist[:want_nit, 0]]
    plain = enc.encode_with_palette(img, pal, roi_mask=mask)
    assert plain["indices_dtype"] == "uint16" and res["indices_dtype"] == "uint8" and "reduce" not in plain["stats"]


def test_encode_with_palette_without_colours_is_unchanged(enc):
    img, pal, mask = _photo_case()
    for kw in ({}, {"roi_mask": mask}, {"roi_mask": mask, "refine": 2, "roi_weight": 3}):
        a, b = enc.encode_with_palette(img, pal, **kw), enc.encode_with_palette(img, pal, colours=None, **kw)
        assert np.array_equal(a["palette"], b["palette"]) and np.array_equal(a["indices"].cpu().numpy(), b["indices"].cpu().numpy())
        assert a["indices_dtype"] == b["indices_dtype"] and {k: v for k, v in a["stats"].items() if k != "seconds"} == \
            {k: v for k, v in b["stats"].items() if k != "seconds"}
    with pytest.raises(ValueError):
        enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=3)          # still needs refine (or colours)
    with pytest.raises(ValueError):
        enc.encode_with_palette(img, pal, roi_weight=3, colours=64)             # and always a mask


# ---- encode(max_colours=N) --------------------------------------------------------------------------------------------------------------
def test_encode_max_colours(enc):
    frame = RF.drift_frames()[0]
    full = enc.encode(frame, *RM.SEQ_QUALITIES)
    K = len(full["palette"])
    N = max(2, K // 2)
    assert K > N
    res = enc.encode(frame, *RM.SEQ_QUALITIES, max_colours=N)
    assert res["top_left"] == full["top_left"] and res["shape"] == full["shape"] and res["indices"].shape == full["indices"].shape
    (top, left), (h, w) = res["top_left"], res["shape"]
    idx0 = full["indices"].cpu().numpy().astype(np.int64).reshape(-1) & 0xFFFF
    counts = np.bincount(idx0, minlength=K)
    want_pal, _, _, merges, k = RD.reduce_reference(np.asarray(full["palette"], np.uint8), counts, N)
    pal = np.asarray(res["palette"], np.uint8)
    assert len(pal) == k <= N and np.array_equal(pal, want_pal[:k])
    want_idx, _ = RM.remap_reference(frame[top:top + h, left:left + w], pal)
    assert np.array_equal(res["indices"].cpu().numpy().astype(np.int64).reshape(-1) & 0xFFFF, want_idx)
    assert res["stats"]["reduce"] == {"from": K, "to": k, "empty": int((counts == 0).sum()), "steps": int((merges[:, 0] >= 0).sum())}
    assert "reduce" not in full["stats"]
    same = enc.encode(frame, *RM.SEQ_QUALITIES, max_colours=K)                  # not above the bound: nothing runs
    assert "reduce" not in same["stats"] and np.array_equal(same["palette"], full["palette"])
    assert np.array_equal(same["indices"].cpu().numpy(), full["indices"].cpu().numpy())


def test_encode_sequence_passes_max_colours_to_its_key_frames(enc):
    A, A2, B = RF.drift_frames()
    q1, q2 = RM.SEQ_QUALITIES
    plain = list(enc.encode_sequence([A, B], q1, q2, RM.SEQ_MAX_DROP_DB))
    assert [r["stats"]["key_frame"] for r in plain] == [True, True] and min(len(r["palette"]) for r in plain) > 16
    assert all("reduce" not in r["stats"] for r in plain)
    out = list(enc.encode_sequence([A, B], q1, q2, RM.SEQ_MAX_DROP_DB, max_colours=16))
    for r, p in zip(out, plain):
        assert r["stats"]["key_frame"] is True and len(r["palette"]) <= 16
        assert r["stats"]["reduce"]["from"] == len(p["palette"]) and r["stats"]["reduce"]["to"] == len(r["palette"])


# ---- container.reduce_frame ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colours", [256, 32])
def test_reduce_frame(rh, tmp_path, colours):
    from roibasedimagecompression_amd import container
    from roibasedimagecompression_amd.api import uncompression as U
    src, dst = os.path.join(G, "g7_lenna64.rhccq"), str(tmp_path / "reduced.rhccq")
    pal0, idx0, (h, w) = U.lossless_decompress(U.load_compressed(src))           # the host decoder
    pal0, idx0 = np.array(pal0, np.uint8), np.array(idx0, np.int64)
    counts = np.bincount(idx0, minlength=len(pal0))
    want_pal, _, map_, _, k = RD.reduce_reference(pal0, counts, min(colours, len(pal0)))
    out = container.reduce_frame(src, dst, colours, rh)
    pkg = U.load_compressed(dst)
    pal1, idx1, shape1 = U.lossless_decompress(pkg)
    assert tuple(shape1) == (h, w) and pkg["d"] == "uint8" and os.path.getsize(dst) == out["bytes"] + 1
    assert np.array_equal(np.array(pal1, np.uint8), want_pal[:k]) and np.array_equal(np.array(idx1, np.int64), map_[idx0])
    assert out["from"] == len(pal0) and out["to"] == k <= colours
    old, new = pal0[idx0].astype(np.int64), want_pal[map_[idx0]].astype(np.int64)
    sse = int(((old - new) ** 2).sum())
    if sse == 0:
        assert colours >= len(pal0) and out["psnr"] == float("inf")
    else:
        assert out["psnr"] == pytest.approx(RM.psnr(sse, h * w), rel=1e-12)
