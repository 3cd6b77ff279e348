"""Per-class quality metrics on the device (csrc/region_metrics.hip: Rhccq.class_error_sums, class_error_sums_indexed, class_ssim7;
api.comparison.region_metrics_from_device) against numpy.  GPU only.

The error sums are integers: identical or wrong.  The SSIM sums are compared with a window-by-window float64 statement
(tests/roimask_cases.py window_ssim, the formula of O.structural_similarity_win7 with S kept per centre): the counts identical,
the per-class means within the 1e-9 absolute of the existing SSIM tests against the oracle."""
import numpy as np
import pytest

import roimask_cases as RC

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 3), (7, 9), (38, 38), (233, 40)]          # 1 px, tail only, 63 px (tail of 3), one SSIM tile, several blocks


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


def _pair(H, W, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return a, b


def _dev(rh, *arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(x)).to(rh.device) for x in arrays]
    return out[0] if len(out) == 1 else out


@pytest.mark.parametrize("n_classes", [1, 2, 16])
@pytest.mark.parametrize("shape", SHAPES)
def test_class_error_sums_equal_numpy(rh, shape, n_classes):
    H, W = shape
    a, b = _pair(H, W, H * 1000 + W)
    cls = np.random.default_rng(5).choice(np.array([0, 1, 255], np.uint8), (H, W))
    got = rh.class_error_sums(*_dev(rh, a, b, cls), n_classes)
    assert got.dtype == np.int64 and got.shape == (n_classes, 6)
    assert np.array_equal(got, RC.class_sums(a, b, cls, n_classes))


def test_class_error_sums_many_classes_absent_class_single_class(rh):
    a, b = _pair(233, 40, 7)
    d_a, d_b = _dev(rh, a, b)
    rng = np.random.default_rng(8)
    cls = rng.choice(np.array(list(range(16)) + [16, 200, 255], np.uint8), (233, 40))
    for n in (3, 5, 16):
        assert np.array_equal(rh.class_error_sums(d_a, d_b, _dev(rh, cls), n), RC.class_sums(a, b, cls, n)), n
    absent = rng.choice(np.array([0, 255], np.uint8), (233, 40))                 # class 1 has no pixel
    got = rh.class_error_sums(d_a, d_b, _dev(rh, absent), 2)
    assert np.array_equal(got, RC.class_sums(a, b, absent, 2)) and not got[1].any() and got[0, 5] > 0
    for n, k in ((2, 0), (2, 1), (16, 9)):                                       # all pixels in one class
        one = np.full((233, 40), k, np.uint8)
        got = rh.class_error_sums(d_a, d_b, _dev(rh, one), n)
        assert np.array_equal(got, RC.class_sums(a, b, one, n)) and got[k, 5] == 233 * 40 and got[:, 5].sum() == 233 * 40
    assert np.array_equal(rh.class_error_sums(d_a, d_b, _dev(rh, cls % 2) != 0, 2), RC.class_sums(a, b, cls % 2, 2))   # a bool map


@pytest.mark.parametrize("n_classes", [2, 16])
def test_class_map_at_an_odd_byte_offset(rh, n_classes):
    import torch
    H, W = 233, 40
    a, b = _pair(H, W, 11)
    cls = np.random.default_rng(12).integers(0, 3, (H, W)).astype(np.uint8)
    buf = torch.zeros(H * W + 8, dtype=torch.uint8, device=rh.device)
    for off in (1, 3):
        view = buf[off:off + H * W].view(H, W)
        view.copy_(_dev(rh, cls))
        assert view.data_ptr() % 4 == off and view.is_contiguous()
        assert np.array_equal(rh.class_error_sums(*_dev(rh, a, b), view, n_classes), RC.class_sums(a, b, cls, n_classes))


def test_class_error_sums_past_32_bits(rh):
    """a = 0, b = 255 in class 1 only: 90 000 px * 65 025 = 5.85e9 per channel, past 2^32 (reached at 66 052 px)"""
    H = W = 300
    a, b = np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8)
    cls = np.ones((H, W), np.uint8)
    got = rh.class_error_sums(*_dev(rh, a, b, cls), 2)
    want = np.array([[0] * 6, [90000 * 65025] * 3 + [90000 * 3 * 255, 255, 90000]], np.int64)
    assert want[1, 0] > 2 ** 32 and np.array_equal(got, want)
    cls[::2] = 0                                                                  # and split over two classes
    assert np.array_equal(rh.class_error_sums(*_dev(rh, a, b, cls), 2), RC.class_sums(a, b, cls, 2))


@pytest.mark.parametrize("shape", SHAPES)
def test_column_sums_equal_error_sums(rh, shape):
    H, W = shape
    a, b = _pair(H, W, 21)
    cls = np.random.default_rng(22).integers(0, 5, (H, W)).astype(np.uint8)
    d_a, d_b, d_c = _dev(rh, a, b, cls)
    rows, whole = rh.class_error_sums(d_a, d_b, d_c, 5), rh.error_sums(d_a, d_b)
    assert np.array_equal(rows[:, :4].sum(axis=0), whole[:4]) and rows[:, 4].max() == whole[4]


@pytest.mark.parametrize("dtype,pal_n", [(np.uint8, 3), (np.uint16, 300), (np.int32, 70000)])
@pytest.mark.parametrize("shape", [(7, 9), (233, 40)])
def test_indexed_equals_plain_on_decoded(rh, shape, dtype, pal_n):
    import torch
    H, W = shape
    rng = np.random.default_rng(pal_n + H)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    pal = rng.integers(0, 256, (pal_n, 3), dtype=np.uint8)
    hi = 256 if dtype == np.uint8 else pal_n                                     # uint8 indices past a 3-colour palette read entry 0
    idx = rng.integers(0, hi, H * W).astype(dtype)
    cls = rng.integers(0, 3, (H, W)).astype(np.uint8)
    d_a, d_pal, d_cls = _dev(rh, a, pal, cls)
    d_idx = _dev(rh, idx.view(np.int16) if dtype == np.uint16 else idx)
    recon = rh.decode(d_idx, d_pal).reshape(H, W, 3)
    want_rec = pal[np.where(idx.astype(np.int64) >= pal_n, 0, idx.astype(np.int64))].reshape(H, W, 3)
    assert np.array_equal(recon.cpu().numpy(), want_rec)
    for n in (2, 16):
        got = rh.class_error_sums_indexed(d_a, d_idx, d_pal, d_cls, n)
        assert np.array_equal(got, rh.class_error_sums(d_a, recon, d_cls, n)), n
        assert np.array_equal(got, RC.class_sums(a, want_rec, cls, n)), n
    # indices from a view that is element- but not vector-aligned
    buf = torch.zeros(H * W + 4, dtype=d_idx.dtype, device=rh.device)
    view = buf[1:1 + H * W]
    view.copy_(d_idx)
    assert np.array_equal(rh.class_error_sums_indexed(d_a, view, d_pal, d_cls, 2), RC.class_sums(a, want_rec, cls, 2))


def test_bad_class_counts_raise(rh):
    from roibasedimagecompression_amd import RhccqError
    a, b = _pair(9, 9, 1)
    d_a, d_b, d_c = _dev(rh, a, b, np.zeros((9, 9), np.uint8))
    d_idx, d_pal = _dev(rh, np.zeros(81, np.uint8), np.zeros((2, 3), np.uint8))
    for n in (0, 17):
        with pytest.raises(RhccqError):
            rh.class_error_sums(d_a, d_b, d_c, n)
        with pytest.raises(RhccqError):
            rh.class_error_sums_indexed(d_a, d_idx, d_pal, d_c, n)
        with pytest.raises(RhccqError):
            rh.class_ssim7(d_a, d_b, d_c, n)
    assert rh.class_error_sums(d_a, d_b, d_c, 1).shape == (1, 6)                 # the context is still usable


def _class_maps(H, W):
    y, x = np.mgrid[:H, :W]
    split = (x >= W // 2).astype(np.uint8)                                       # a boundary through a tile
    diag = (x * H > y * W).astype(np.uint8)                                      # a diagonal one
    border = np.zeros((H, W), np.uint8)                                          # class 2 lives in the 3-px border only: no centre
    border[:3], border[-3:], border[:, :3], border[:, -3:] = 2, 2, 2, 2
    border[3:-3, 3:-3] = split[3:-3, 3:-3]
    ignore = diag.copy()
    ignore[H // 3:H // 2] = 255                                                  # windows centred on an ignored pixel count nowhere
    return {"split": (split, 2), "diag": (diag, 2), "border": (border, 3), "ignore": (ignore, 2), "sixteen": ((x % 16).astype(np.uint8), 16)}


@pytest.mark.parametrize("shape", [(7, 7), (38, 38), (39, 45), (70, 33)])       # one window, one full tile, 2 x 2 tiles, 2 x 1 tiles
def test_class_ssim7_equals_window_statement(rh, shape):
    H, W = shape
    a, _ = _pair(H, W, 31)
    b = np.clip(a.astype(np.int64) + np.random.default_rng(32).integers(-30, 31, a.shape), 0, 255).astype(np.uint8)
    d_a, d_b = _dev(rh, a, b)
    for name, (cls, n) in _class_maps(H, W).items():
        sums, counts = rh.class_ssim7(d_a, d_b, _dev(rh, cls), n)
        want_sums, want_counts = RC.class_ssim(a, b, cls, n)
        assert counts.dtype == np.int64 and np.array_equal(counts, want_counts), name
        for k in range(n):
            if want_counts[k]:
                assert np.all(np.abs(sums[k] / counts[k] - want_sums[k] / want_counts[k]) <= 1e-9), (name, k)
            else:
                assert not sums[k].any(), (name, k)
        if name == "border":
            assert counts[2] == 0 and (cls == 2).sum() > 0
        if name in ("split", "diag", "border", "sixteen"):                       # every centre has a class: the counts add up
            assert counts.sum() == (H - 6) * (W - 6)
    # all windows in one class = the whole-picture kernel (same per-window arithmetic; the order of the float64 additions
    # differs: fewer than 2 000 terms of at most 1 in magnitude, each addition within 2^-53 relative: far below 1e-12 on the mean)
    sums, counts = rh.class_ssim7(d_a, d_b, _dev(rh, np.zeros((H, W), np.uint8)), 1)
    assert np.all(np.abs(sums[0] / counts[0] - rh.ssim7(d_a, d_b)) <= 1e-12)


def test_region_metrics_from_device(rh):
    from roibasedimagecompression_amd.api.comparison import (calculate_region_quality_metrics, metrics_from_device, region_metrics_from_device,
                                                             region_metrics_from_sums)
    H, W = 70, 33
    a, _ = _pair(H, W, 41)
    b = np.clip(a.astype(np.int64) + np.random.default_rng(42).integers(-25, 26, a.shape), 0, 255).astype(np.uint8)
    cls = _class_maps(H, W)["diag"][0]
    d_a, d_b, d_c = _dev(rh, a, b, cls)
    got = region_metrics_from_device(rh, d_a, d_b, d_c)
    want = region_metrics_from_sums(RC.class_sums(a, b, cls, 2), RC.class_ssim(a, b, cls, 2), ("nonroi", "roi"))
    assert list(got) == ["nonroi", "roi", "all"]
    whole = metrics_from_device(rh, d_a, d_b)
    assert list(got["all"]) == list(whole) + ["pixel_count"] and got["all"]["pixel_count"] == H * W
    for name in got:
        for k, v in want[name].items():
            assert type(got[name][k]) is type(v), (name, k)
            if k == "ssim":
                assert abs(got[name][k] - v) <= 1e-9, (name, k)
            else:
                assert got[name][k] == v, (name, k)                              # integer sums, the same host arithmetic
    for k, v in whole.items():                                                   # "all" = the whole-picture metrics, key for key
        assert type(got["all"][k]) is type(v), k
        if k == "ssim":
            assert abs(got["all"][k] - v) <= 1e-12, k                            # reordered float64 additions only (see above)
        else:
            assert got["all"][k] == v, k
    host = calculate_region_quality_metrics(a, b, cls.astype(bool))
    assert all(host[n][k] == got[n][k] for n in got for k in got[n])
    three = calculate_region_quality_metrics(a, b, np.full((H, W), 2, np.uint8), names=("x", "y", "z"))
    assert three["x"] is None and three["y"] is None and three["z"] == three["all"]
    with pytest.raises(ValueError):
        calculate_region_quality_metrics(a, b, cls[:, :-1])
    # 6 x 40: no window fits, 0 blocks, ssim None (the error statistics as usual)
    a6, b6 = _pair(6, 40, 43)
    assert rh.lib.rhccq_class_ssim7_blocks(6, 40) == 0 and rh.lib.rhccq_class_ssim7_blocks(7, 7) == 1
    small = calculate_region_quality_metrics(a6, b6, _class_maps(6, 40)["split"][0])
    assert all(small[n]["ssim"] is None for n in small) and small["all"]["pixel_count"] == 240
    assert np.isfinite(small["all"]["psnr"])
