"""The palette ladder on the device (csrc/palette_ladder.hip: Rhccq.palette_moments, palette_curve, palette_rung) against its host
forms and the numpy references of tests/ladder_cases.py, bit for bit, and what is built on it: ImageEncoder.ladder and the
target_bytes / target_psnr keywords of encode_with_palette, encode and encode_sequence.  GPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import ladder_cases as LD
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


def _np(t):
    return t.cpu().numpy()


def _idx(t):
    return _np(t).astype(np.int64).reshape(-1) & 0xFFFF


# ---- the three kernels against their host forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LD.names(pixels=False))
def test_device_moments_equal_host(rh, name):
    """every case, on both sides of the LDS threshold: the wrapper's index width, four-byte indices and no indices at all"""
    import torch
    c = LD.case(name)
    want_idx, want_mom, _ = LD.reference(name)                                  # (equal to the host form's: tests/test_palette_ladder_cpu.py)
    idx, mom = rh.palette_moments(c["rgb"], c["pal"], c["cls"], c["n_classes"])
    assert idx.shape == c["rgb"].shape[:-1] and np.array_equal(_idx(idx), want_idx) and np.array_equal(_np(mom), want_mom), name
    none, mom = rh.palette_moments(c["rgb"], c["pal"], c["cls"], c["n_classes"], want_indices=False)
    assert none is None and np.array_equal(_np(mom), want_mom), name
    n, K = len(want_idx), len(c["pal"])
    if n:
        rgb, pal = rh.dev(np.ascontiguousarray(c["rgb"])), rh.dev(np.ascontiguousarray(c["pal"]))
        cls = None if c["cls"] is None else rh.dev(np.ascontiguousarray(c["cls"]))
        wide = torch.full((n,), 0x55555555, dtype=torch.int32, device=rh.device)
        mom = torch.full(want_mom.shape, 0x5555, dtype=torch.int64, device=rh.device)          # (the call zeroes it)
        assert rh.lib.rhccq_palette_moments(rh.ctx, rh._p(rgb), n, rh._p(pal), K, rh._p(cls), c["n_classes"], rh._p(wide), 4, rh._p(mom)) == 0
        assert np.array_equal(_np(wide).astype(np.int64), want_idx) and np.array_equal(_np(mom), want_mom), name


@pytest.mark.parametrize("name", LD.TIE_NAMES)
def test_device_moments_keep_the_lowest_row_on_a_tie(rh, name):
    """the search's constructed ties, inside a tile and across a tile boundary: every legal index width and no index buffer"""
    import torch
    c = LD.case(name)
    want_idx, want_mom, _ = LD.reference(name)
    assert want_idx.tolist() == c["expect"]
    n, K = len(want_idx), len(c["pal"])
    rgb, pal = rh.dev(np.ascontiguousarray(c["rgb"])), rh.dev(np.ascontiguousarray(c["pal"]))
    for width in (None,) + RM.index_bytes(K):
        idx = None if width is None else torch.full((n,), 0x55, dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[width], device=rh.device)
        mom = torch.full(want_mom.shape, 0x5555, dtype=torch.int64, device=rh.device)          # (the call zeroes it)
        assert rh.lib.rhccq_palette_moments(rh.ctx, rh._p(rgb), n, rh._p(pal), K, rh._p(None), 0, rh._p(idx), width or 0, rh._p(mom)) == 0, (name, width)
        assert np.array_equal(_np(mom), want_mom), (name, width)
        assert idx is None or (_np(idx).astype(np.int64) & ((1 << 8 * width) - 1)).tolist() == c["expect"], (name, width)


def test_the_lds_threshold_is_where_the_cases_say(rh):
    from roibasedimagecompression_amd import ops
    assert (LD.LDS0, LD.LDS2) == (ops.palette_moments_lds_rows(0), ops.palette_moments_lds_rows(2))
    ks = sorted(len(LD.case(n)["pal"]) for n in LD.names() if n.startswith("37x53_K") and len(LD.case(n)["pal"]) > 300)
    assert ks == sorted([LD.LDS2, LD.LDS2 + 1, LD.LDS0, LD.LDS0 + 1])


@pytest.mark.parametrize("name", LD.names())
def test_device_curve_and_rung_equal_host(rh, name):
    c = LD.case(name)
    K = len(c["pal"])
    _, mom, _ = LD.reference(name)
    counts, merges, want_curve, live = LD.host_ladder(name)
    curve = rh.palette_curve(c["pal"], counts, merges[:live - 1], mom)
    assert np.array_equal(_np(curve), want_curve), name
    for k in sorted({1, 2, 3, live - 1, live, min(live + 1, K), K}):
        if not 1 <= k <= K:
            continue
        _, want_pal, want_cnt, want_map, want_k = LD.host_rung(c["pal"], counts, merges, k)
        pal, cnt, map_ = rh.palette_rung(c["pal"], counts, merges[:live - 1], k)
        assert pal.shape == (want_k, 3) and np.array_equal(_np(pal), want_pal[:want_k]) and np.array_equal(_np(cnt), want_cnt[:want_k]), (name, k)
        assert np.array_equal(_np(map_), want_map), (name, k)


def test_the_cap_with_the_device_chain(rh):
    """4 096 rows, all in use: the device chain to one row, then the curve and rungs from its log against the host forms"""
    import torch
    rng = np.random.default_rng(77)
    pal = RM._palette(rng, LD.CAP)
    rgb = RM._near(rng, pal, 37 * 53, spread=5)
    cls = (rng.random(37 * 53) < 0.3).astype(np.uint8)
    rc, _, mom = LD.host_moments(rgb, pal, cls, 2)
    assert rc == 0
    counts = 1 + LD.combine_counts(mom, [1, 7, 1])                              # every row has weight: 4 095 steps
    _, _, _, merges = rh.palette_reduce(pal, counts, 1)
    merges_h = _np(merges)
    assert merges_h.shape == (LD.CAP - 1, 2)
    rc, want_curve = LD.host_curve(pal, counts, merges_h, mom)
    assert rc == 0
    curve = rh.palette_curve(pal, counts, merges, mom)
    assert np.array_equal(_np(curve), want_curve) and (want_curve[:, -1] > 0).all()
    for k in (1, 2, 16, 1000, LD.CAP - 1, LD.CAP):
        _, want_pal, want_cnt, want_map, want_k = LD.host_rung(pal, counts, merges_h, k)
        got_pal, got_cnt, got_map = rh.palette_rung(pal, counts, merges, k)
        assert want_k == k and np.array_equal(_np(got_pal), want_pal) and np.array_equal(_np(got_cnt), want_cnt) and np.array_equal(_np(got_map), want_map), k
    # the whole output buffers of one raw call: zero rows behind k_out
    short = merges_h.copy()
    short[5:] = -1
    d = {k: rh.dev(v) for k, v in (("pal", pal), ("counts", counts.astype(np.int64)), ("merges", short))}
    pal_out = torch.full((64, 3), 0x55, dtype=torch.uint8, device=rh.device)
    cnt_out = torch.full((64,), 0x5555, dtype=torch.int64, device=rh.device)
    map_ = torch.full((LD.CAP,), -7, dtype=torch.int32, device=rh.device)
    k_out = torch.full((2,), -7, dtype=torch.int32, device=rh.device)
    assert rh.lib.rhccq_palette_rung(rh.ctx, rh._p(d["pal"]), rh._p(d["counts"]), LD.CAP, rh._p(d["merges"]), 64, rh._p(pal_out), rh._p(cnt_out),
                                     rh._p(map_), rh._p(k_out)) == 0
    _, want_pal, want_cnt, want_map, want_k = LD.host_rung(pal, counts, short, 64)
    assert _np(k_out).tolist() == [want_k, -7] and want_k == LD.CAP - 5          # the log ended early: the clusters it has
    assert np.array_equal(_np(pal_out), want_pal) and np.array_equal(_np(cnt_out), want_cnt) and np.array_equal(_np(map_), want_map)


def _device_pointers(rh, bufs, over):
    import torch
    dev = {k: rh.dev(a.view(np.int64) if a.dtype == np.uint64 else a) for k, a in bufs.items()}
    out = {}
    for k, t in dev.items():
        off = (1 if t.element_size() in (8, 2) else 2) if over.get("misalign") == k else 0
        out[k] = C.c_void_p(0) if k in over and over[k] is None else C.c_void_p(t.data_ptr() + off)
    return dev, out


def _chain_bufs():
    return {"palette": np.arange(9, dtype=np.uint8).reshape(3, 3), "counts": np.array([1, 2, 3, 0], np.uint64),
            "merges": np.array([[0, 1], [-1, -1], [-1, -1]], np.int32), "moments": np.ones(3 * 5 + 1, np.uint64), "curve": np.full(4, 77, np.uint64),
            "palette_out": np.full((4, 3), 0x55, np.uint8), "counts_out": np.full(5, 77, np.uint64), "map": np.full(4, -7, np.int32),
            "k_out": np.full(2, -7, np.int32), "work": np.zeros(64, np.uint64)}


@pytest.mark.parametrize("what,over,code", [e[:3] for e in LD.CURVE_ERRORS], ids=[e[0] for e in LD.CURVE_ERRORS])
def test_device_curve_argument_errors(rh, what, over, code):
    dev, p = _device_pointers(rh, _chain_bufs(), over)
    wb = int(rh._raw.rhccq_palette_curve_bytes(3, 1))
    got = rh.lib.rhccq_palette_curve(rh.ctx, p["palette"], p["counts"], over.get("K", 3), p["merges"], p["moments"], over.get("n_tables", 1), p["work"],
                                     wb - (1 if over.get("work_short") else 0), p["curve"])
    rh.sync()
    assert got == code and (_np(dev["curve"]) == 77).all(), what                # nothing was launched


@pytest.mark.parametrize("what,over,code", [e[:3] for e in LD.RUNG_ERRORS], ids=[e[0] for e in LD.RUNG_ERRORS])
def test_device_rung_argument_errors(rh, what, over, code):
    dev, p = _device_pointers(rh, _chain_bufs(), over)
    got = rh.lib.rhccq_palette_rung(rh.ctx, p["palette"], p["counts"], over.get("K", 3), p["merges"], over.get("K_target", 2), p["palette_out"],
                                    p["counts_out"], p["map"], p["k_out"])
    rh.sync()
    assert got == code and (_np(dev["k_out"]) == -7).all() and (_np(dev["map"]) == -7).all(), what


def test_device_valid_calls_and_data_errors(rh):
    from roibasedimagecompression_amd import RhccqError
    dev, p = _device_pointers(rh, _chain_bufs(), {})
    wb = int(rh._raw.rhccq_palette_curve_bytes(3, 1))
    assert rh.lib.rhccq_palette_curve(rh.ctx, p["palette"], p["counts"], 3, p["merges"], p["moments"], 1, p["work"], wb, p["curve"]) == 0
    assert rh.lib.rhccq_palette_rung(rh.ctx, p["palette"], p["counts"], 3, p["merges"], 2, p["palette_out"], p["counts_out"], p["map"], p["k_out"]) == 0
    b = _chain_bufs()
    rc, want = LD.host_curve(b["palette"], b["counts"][:3], b["merges"][:2], b["moments"][:15].reshape(1, 3, 5))
    assert rc == 0 and _np(dev["curve"]).tolist() == want[0].tolist() + [77]
    assert _np(dev["k_out"]).tolist() == [2, -7] and _np(dev["map"]).tolist() == [0, 0, 1, -7] and _np(dev["counts_out"]).tolist() == [3, 3, 77, 77, 77]
    for what, counts, code in LD.RUNG_DATA_ERRORS:                              # they come back through k_out, as the reduction's do
        b = _chain_bufs()
        b["counts"][:3] = np.array(counts, np.uint64)
        dev, p = _device_pointers(rh, b, {})
        assert rh.lib.rhccq_palette_rung(rh.ctx, p["palette"], p["counts"], 3, p["merges"], 2, p["palette_out"], p["counts_out"], p["map"], p["k_out"]) == 0
        assert _np(dev["k_out"]).tolist() == [code, -7] and _np(dev["map"]).tolist() == [-1, -1, -1, -7] and not _np(dev["palette_out"])[:2].any(), what
        with pytest.raises(RhccqError):
            rh.palette_rung(np.zeros((3, 3), np.uint8), np.array(counts, np.uint64), b["merges"][:2], 2)
    with pytest.raises(RhccqError, match=str(LD.CAP)):
        rh.palette_rung(np.zeros((LD.CAP + 1, 3), np.uint8), np.ones(LD.CAP + 1, np.int64), np.zeros((0, 2), np.int32), 2)
    with pytest.raises(RhccqError, match=str(LD.CAP)):
        rh.palette_curve(np.zeros((LD.CAP + 1, 3), np.uint8), np.ones(LD.CAP + 1, np.int64), np.zeros((0, 2), np.int32), np.zeros((1, LD.CAP + 1, 5), np.int64))


@pytest.mark.parametrize("what,over,code", LD.MOMENTS_ERRORS, ids=[e[0] for e in LD.MOMENTS_ERRORS])
def test_device_moments_argument_errors(rh, what, over, code):
    bufs = {"rgb": np.zeros((4, 3), np.uint8), "palette": np.arange(9, dtype=np.uint8).reshape(3, 3), "idx_out": np.full(6, 0x5555, np.uint16).view(np.int16),
            "moments": np.full(2 * 3 * 5 + 1, 77, np.uint64), "cls": np.zeros(4, np.uint8)}
    dev, p = _device_pointers(rh, bufs, over)
    got = rh.lib.rhccq_palette_moments(rh.ctx, p["rgb"], over.get("n_pixels", 4), p["palette"], over.get("K", 3), p["cls"] if over.get("cls") else C.c_void_p(0),
                                       over.get("n_classes", 0), p["idx_out"], over.get("idx_elem_bytes", 2), p["moments"])
    rh.sync()
    assert got == code and (_np(dev["moments"]) == 77).all(), what


# ---- ImageEncoder.ladder ---------------------------------------------------------------------------------------------------------------
def _photo_case():
    from roibasedimagecompression_amd import synth
    img = synth.photo(96, 128, 7)
    flat = img.reshape(-1, 3)
    pal = flat[np.random.default_rng(5).choice(len(flat), 300, replace=False)].copy()
    pal[17] = pal[3]                                                           # a duplicate row: no pixel goes to it
    mask = np.zeros((96, 128), bool)
    mask[20:70, 30:100] = True
    return img, pal, mask


def _cpu_ladder(img, pal, mask, roi_weight):
    """the host forms end to end -> (counts, merges, curve int64[T, K], live, moments)"""
    rc, _, mom = LD.host_moments(img, pal, None if mask is None else mask.astype(np.uint8), 0 if mask is None else 2)
    assert rc == 0
    counts = LD.combine_counts(mom, [1] if mask is None else [1, roi_weight, 1])
    rc, _, _, _, merges, k = LD.host_reduce(pal, counts, 1)
    assert rc == 0 and k == 1
    rc, curve = LD.host_curve(pal, counts, merges, mom)
    assert rc == 0
    return counts, merges, curve, int((counts > 0).sum()), mom


@pytest.mark.parametrize("masked", [False, True])
def test_ladder(rh, enc, masked):
    img, pal, mask = _photo_case()
    mask, w = (mask, 7) if masked else (None, 1)
    counts, merges, curve, live, mom = _cpu_ladder(img, pal, mask, w)
    L = enc.ladder(img, pal, roi_mask=mask, roi_weight=w)
    names = ("nonroi", "roi", "all") if masked else ("all",)
    assert L["colours"] == list(range(live, 0, -1)) and sorted(L["sse"]) == sorted(names) == sorted(L["psnr_bound"])
    assert np.array_equal(L["merges"], merges[:live - 1])
    for t, n in enumerate(names):
        pixels = int(mom[t, :, 0].sum())
        assert L["pixels"][n] == pixels and L["sse"][n] == curve[t, :live].tolist(), n
        assert L["psnr_bound"][n] == pytest.approx([RM.psnr(v, pixels) for v in curve[t, :live]], rel=1e-12), n
    assert L["sse"]["all"][0] == int(RM.remap_reference(img, pal)[1][-1, 1])     # no merge yet: the remap's own error
    st = L["state"]
    assert np.array_equal(_np(st["counts"]), counts) and np.array_equal(_idx(st["indices"]), RM.remap_reference(img, pal)[0])
    for k in (1, 2, 16, 64, live - 1, live):                                    # every rung is the palette colours=k would use
        pal_k, cnt_k, map_k = rh.palette_rung(st["palette"], st["counts"], st["merges"], k)
        want_pal, want_cnt, want_map, _ = rh.palette_reduce(pal, counts, k)
        assert np.array_equal(_np(pal_k), _np(want_pal)) and np.array_equal(_np(cnt_k), _np(want_cnt)) and np.array_equal(_np(map_k), _np(want_map)), k
    with pytest.raises(ValueError):
        enc.ladder(img, pal, roi_weight=3)                                      # a weight needs a mask


# ---- the targets of encode_with_palette -----------------------------------------------------------------------------------------------
def _png(name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(G, name + ".png")).convert("RGB"), dtype=np.uint8)


_KODAK = {}


def _kodak(enc, shape):
    """a crop of a golden Kodak image and the palette ImageEncoder.encode gives the 96 x 128 crop (computed once)"""
    if not _KODAK:
        big = np.ascontiguousarray(_png("kodak_5")[200:296, 300:428])
        _KODAK["pal"] = np.asarray(enc.encode(big, 20, 10)["palette"], np.uint8).reshape(-1, 3).copy()
        _KODAK[(96, 128)] = big
        _KODAK[(37, 53)] = np.ascontiguousarray(big[:37, :53])
    return _KODAK[shape], _KODAK["pal"]


def _host_file(pal, idx, shape, path):
    from roibasedimagecompression_amd.api import compression as CP
    CP.save_compressed(CP.lossless_compress_optimized(np.asarray(pal, np.uint8), np.asarray(idx, np.int64), shape), path)
    with open(path, "rb") as f:
        return f.read()


def _cpu_byte_search(img, pal, B, refine, colours, path):
    """the search of encode_with_palette(target_bytes=B, exact=True) with the host forms, the numpy references and zlib level 9
    -> (k, met, probes, palette, indices, file bytes)"""
    counts, merges, _, live, _ = _cpu_ladder(img, pal, None, 1)
    k0 = min(colours or len(pal), live)
    probes, done = [], {}

    def probe(k):
        rc, p, _, _, k_out = LD.host_rung(pal, counts, merges, k)
        assert rc == 0 and k_out == k
        if refine:
            p, _, _ = RF.refine_reference(img, p, None, None, max_iter=refine)
        idx, _ = RM.remap_reference(img, p)
        data = _host_file(p, idx, img.shape[:2], path)
        probes.append((k, len(data)))
        done[k] = (np.asarray(p, np.uint8), idx, data)
        return len(data) <= B
    if probe(k0):
        return (k0, True, probes) + done[k0]
    lo, hi = 0, k0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if probe(mid):
            lo = mid
        else:
            hi = mid
    return (max(lo, 1), lo > 0, probes) + done[max(lo, 1)]


@pytest.mark.parametrize("shape,refine,frac", [((37, 53), 0, 0.7), ((37, 53), 2, 0.5), ((96, 128), 0, 0.6), ((96, 128), 2, 0.8), ((37, 53), 0, 2.0),
                                               ((37, 53), 0, 0.0)])
def test_target_bytes_exact(enc, tmp_path, shape, refine, frac):
    """the same k, the same probes and the same file as the search run on the CPU; the result is colours=k's"""
    img, pal = _kodak(enc, shape)
    top = _cpu_byte_search(img, pal, 1 << 40, refine, None, str(tmp_path / "cpu.rhccq"))
    B = max(1, int(top[2][0][1] * frac))                                        # a fraction of the top rung's file
    want_k, want_met, want_probes, want_pal, want_idx, want_file = _cpu_byte_search(img, pal, B, refine, None, str(tmp_path / "cpu.rhccq"))
    out = str(tmp_path / "gpu.rhccq")
    res = enc.encode_with_palette(img, pal, target_bytes=B, exact=True, refine=refine, out_path=out)
    tg = res["stats"]["target"]
    print(shape, refine, B, tg)
    assert (tg["kind"], tg["target"], tg["colours"], tg["met"], tg["refine_dropped"]) == ("bytes", B, want_k, want_met, False)
    assert [tuple(p) for p in tg["probes"]] == want_probes
    assert want_met == (frac > 0) and (len(want_probes) > 1) == (frac < 1) and (not want_met or want_probes[-1][1] <= B or want_k != want_probes[-1][0])
    with open(out, "rb") as f:
        data = f.read()
    assert data == want_file and dict(want_probes)[want_k] == len(data)
    assert np.array_equal(np.asarray(res["palette"]), want_pal) and np.array_equal(_idx(res["indices"]), want_idx)
    same = enc.encode_with_palette(img, pal, colours=want_k, exact=True, refine=refine, out_path=str(tmp_path / "colours.rhccq"))
    with open(str(tmp_path / "colours.rhccq"), "rb") as f:
        assert f.read() == data
    assert np.array_equal(same["palette"], res["palette"]) and np.array_equal(_np(same["indices"]), _np(res["indices"]))
    for key in ("reduce", "remap", "refine"):
        assert res["stats"].get(key) == same["stats"].get(key), key


def test_target_bytes_fast_encoder_and_colours_cap(enc, tmp_path):
    """exact=False: the file is no larger than the target, or met is False at rung 1; colours=N caps the rungs"""
    img, pal = _kodak(enc, (96, 128))
    full = enc.encode_with_palette(img, pal, out_path=str(tmp_path / "full.rhccq"))
    size = os.path.getsize(str(tmp_path / "full.rhccq"))
    for B, cap in ((int(size * 0.7), None), (int(size * 0.7), 12), (size * 4, 12), (10, None)):
        out = str(tmp_path / "t.rhccq")
        res = enc.encode_with_palette(img, pal, target_bytes=B, colours=cap, out_path=out)
        tg = res["stats"]["target"]
        k = tg["colours"]
        assert os.path.getsize(out) == dict(tg["probes"])[k] and (os.path.getsize(out) <= B if tg["met"] else k == 1), (B, cap, tg)
        assert tg["met"] == (B > 10) and (cap is None or k <= cap) and tg["probes"][0][0] == (cap or res["stats"]["reduce"]["from"] - res["stats"]["reduce"]["empty"])
        same = enc.encode_with_palette(img, pal, colours=k)
        assert np.array_equal(same["palette"], res["palette"]) and np.array_equal(_np(same["indices"]), _np(res["indices"]))
        assert same["stats"]["reduce"] == res["stats"]["reduce"] and same["stats"]["remap"] == res["stats"]["remap"]
    assert "target" not in full["stats"]
    with pytest.raises(ValueError):
        enc.encode_with_palette(img, pal, target_bytes=1000, target_psnr=30.0)
    with pytest.raises(ValueError):
        enc.encode_with_palette(img, pal, target_psnr={"roi": 30.0})            # needs roi_mask
    with pytest.raises(ValueError):
        enc.encode_with_palette(img, pal, target_bytes=0)


def _cpu_rung_psnr(img, pal, mask, roi_weight):
    """-> (live, names, bound[name][k]: the CPU curve's PSNR of rung k, None for a table without pixels)"""
    counts, merges, curve, live, mom = _cpu_ladder(img, pal, mask, roi_weight)
    names = ("all",) if mask is None else ("nonroi", "roi", "all")
    bound = {}
    for t, n in enumerate(names):
        pixels = int(mom[t, :, 0].sum())
        bound[n] = {live - s: (RM.psnr(curve[t, s], pixels) if pixels else None) for s in range(live)}
    return live, names, bound


@pytest.mark.parametrize("masked,refine,target", [(False, 0, 32.0), (False, 2, 30.0), (True, 0, {"roi": 34.0, "nonroi": 27.0}),
                                                   (True, 0, {"all": 29.0, "roi": 31.0}), (True, 2, {"roi": 33.0})])
def test_target_psnr(enc, masked, refine, target):
    img, pal, mask = _photo_case()
    mask, w = (mask, 7) if masked else (None, 1)
    live, names, bound = _cpu_rung_psnr(img, pal, mask, w)
    cons = target if isinstance(target, dict) else {"all": target}

    def ok(k):
        return all(bound[n][k] is None or bound[n][k] >= v for n, v in cons.items())
    res = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=w, refine=refine, target_psnr=target)
    tg = res["stats"]["target"]
    k = tg["colours"]
    print(masked, refine, target, tg, {n: res["stats"]["remap"][n]["psnr"] for n in names})
    assert tg["kind"] == "psnr" and tg["probes"] == [] and tg["met"] is True and tg["target"] == cons
    assert 1 < k < live and ok(k) and not ok(k - 1)                              # the smallest rung whose bound meets every constraint
    assert all(not ok(j) for j in range(1, k))
    assert sorted(tg["bound_psnr"]) == sorted(names) and all(tg["bound_psnr"][n] == pytest.approx(bound[n][k], rel=1e-12) for n in names)
    for n, v in cons.items():                                                   # the final remap's own sums meet every constraint
        assert res["stats"]["remap"][n]["psnr"] >= v, n
    if not refine:
        assert all(res["stats"]["remap"][n]["psnr"] >= bound[n][k] for n in names)
    kw = {} if tg["refine_dropped"] else {"refine": refine}
    same = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=w, colours=k, **kw)
    assert np.array_equal(same["palette"], res["palette"]) and np.array_equal(_np(same["indices"]), _np(res["indices"]))
    for key in ("reduce", "remap", "refine"):
        assert res["stats"].get(key) == same["stats"].get(key), key


def test_target_psnr_out_of_reach(enc):
    img, pal, mask = _photo_case()
    live, _, bound = _cpu_rung_psnr(img, pal, None, 1)
    assert bound["all"][live] < 90.0
    res = enc.encode_with_palette(img, pal, target_psnr=90.0)
    assert res["stats"]["target"]["colours"] == live and res["stats"]["target"]["met"] is False and len(res["palette"]) == live
    res = enc.encode_with_palette(img, pal, target_psnr=90.0, colours=40)       # colours caps the rungs
    assert res["stats"]["target"]["colours"] == 40 and res["stats"]["target"]["met"] is False and len(res["palette"]) == 40
    res = enc.encode_with_palette(img, pal, target_psnr=1.0)                    # any rung will do: the lowest
    assert res["stats"]["target"]["colours"] == 1 and res["stats"]["target"]["met"] is True


def _dropped_case():
    """three rows far apart; the non-ROI pixels sit exactly on rows 0 and 1, the ROI pixels 40 off row 0 and on row 2.  Rung 3 is
    the palette itself and shows the non-ROI pixels without error; rung 2 does not.  The refinement with roi_weight 7 pulls row 0
    towards the ROI pixels and the non-ROI figure falls far below 60 dB."""
    pal = np.array([[100, 0, 0], [0, 200, 0], [0, 0, 250]], np.uint8)
    img = np.zeros((8, 16, 3), np.uint8)
    mask = np.zeros((8, 16), bool)
    mask[:, 8:] = True
    img[:, :4], img[:, 4:8] = (100, 0, 0), (0, 200, 0)
    img[:, 8:12], img[:, 12:] = (140, 0, 0), (0, 0, 250)
    return img, pal, mask


def test_refine_dropped(enc):
    img, pal, mask = _dropped_case()
    # the case does what it is built for, by the numpy references alone
    live, _, bound = _cpu_rung_psnr(img, pal, mask, 7)
    assert live == 3 and bound["nonroi"][3] == float("inf") and bound["nonroi"][2] < 60.0
    cls = mask.astype(np.uint8)
    refined, _, _ = RF.refine_reference(img, pal, cls, [1, 7, 1], max_iter=4)
    _, s_ref = RM.remap_reference(img, refined, cls, 2)
    _, s_plain = RM.remap_reference(img, pal, cls, 2)
    assert s_plain[0, 1] == 0 and RM.psnr(s_ref[0, 1], s_ref[0, 0]) < 60.0 and s_ref[1, 1] < s_plain[1, 1]
    res = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=7, refine=4, target_psnr={"nonroi": 60.0})
    tg = res["stats"]["target"]
    assert tg["colours"] == 3 and tg["refine_dropped"] is True and tg["met"] is True and "refine" not in res["stats"]
    assert np.array_equal(np.asarray(res["palette"]), pal) and res["stats"]["remap"]["nonroi"]["sse"] == 0
    kept = enc.encode_with_palette(img, pal, roi_mask=mask, roi_weight=7, refine=4, target_psnr={"roi": 20.0})     # the ROI only gains
    assert kept["stats"]["target"]["refine_dropped"] is False and "refine" in kept["stats"]


# ---- encode and encode_sequence --------------------------------------------------------------------------------------------------------
def test_encode_targets(enc, tmp_path):
    frame = RF.drift_frames()[0]
    full = enc.encode(frame, *RM.SEQ_QUALITIES)
    (top, left), (h, w) = full["top_left"], full["shape"]
    window = np.ascontiguousarray(frame[top:top + h, left:left + w])
    live, _, bound = _cpu_rung_psnr(window, np.asarray(full["palette"], np.uint8), None, 1)
    P = (bound["all"][live] + bound["all"][max(1, live // 4)]) / 2              # between the top rung and a low one
    res = enc.encode(frame, *RM.SEQ_QUALITIES, target_psnr=P)
    tg = res["stats"]["target"]
    assert tg["kind"] == "psnr" and 1 <= tg["colours"] < live and bound["all"][tg["colours"]] >= P > bound["all"][tg["colours"] - 1]
    assert res["top_left"] == full["top_left"] and res["shape"] == full["shape"] and res["indices"].shape == full["indices"].shape
    same = enc.encode_with_palette(window, np.asarray(full["palette"], np.uint8), colours=tg["colours"])
    assert np.array_equal(same["palette"], res["palette"]) and np.array_equal(_idx(same["indices"]), _idx(res["indices"]))
    assert res["stats"]["reduce"] == same["stats"]["reduce"]
    out = str(tmp_path / "t.rhccq")
    enc.encode(frame, *RM.SEQ_QUALITIES, out_path=str(tmp_path / "full.rhccq"))
    B = int(os.path.getsize(str(tmp_path / "full.rhccq")) * 0.8)
    res = enc.encode(frame, *RM.SEQ_QUALITIES, target_bytes=B, out_path=out)
    tg = res["stats"]["target"]
    assert tg["kind"] == "bytes" and tg["met"] is True and os.path.getsize(out) == dict(tg["probes"])[tg["colours"]] <= B
    for kw in ({"target_bytes": B, "max_colours": 16}, {"target_psnr": 30.0, "max_colours": 16}, {"target_bytes": B, "target_psnr": 30.0}):
        with pytest.raises(ValueError):
            enc.encode(frame, *RM.SEQ_QUALITIES, **kw)


def test_encode_sequence_passes_the_target_to_its_key_frames(enc):
    A, A2, B = RF.drift_frames()
    q1, q2 = RM.SEQ_QUALITIES
    out = list(enc.encode_sequence([A, B], q1, q2, RM.SEQ_MAX_DROP_DB, target_psnr=25.0))
    assert [r["stats"]["key_frame"] for r in out] == [True, True]
    for r in out:
        assert r["stats"]["target"]["kind"] == "psnr" and r["stats"]["target"]["colours"] == len(r["palette"]) == r["stats"]["reduce"]["to"]
    with pytest.raises(ValueError):
        list(enc.encode_sequence([A], q1, q2, RM.SEQ_MAX_DROP_DB, target_psnr=25.0, max_colours=16))
