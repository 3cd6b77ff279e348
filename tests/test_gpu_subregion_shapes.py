"""The sub-region stage (csrc/split_score.hip, csrc/slic.hip through ops.Rhccq, api/split_score.py, api/slic.py and ImageEncoder's
batched launches) on tile-edge and degenerate shapes: device against the oracle or a literal loop, never against another device path.
GPU only.

The shapes, contents and the reference side of every comparison come from tests/test_subregion_shapes_cpu.py, which also pins the
oracle itself to scipy / literal definitions on the same shapes and asserts that the comparisons are not vacuous.

  split statistics   all 12 raw sums, not the clipped scores: histograms and count identical, every float sum within
                     1e-9 x max(count, sum |term|) (the 1e-9 of test_split_score_vs_oracle per masked pixel; on these <= 1105-pixel shapes
                     one wrong halo pixel moves a mean by ~1e-6).  The largest observed error / bound is printed per shape.
  everything else    exact: LBP codes of flat patches (decided by float rounding), label maps, centroid tables (bytes), resizes."""
import numpy as np
import pytest

import test_subregion_shapes_cpu as S
from test_subregion_shapes_cpu import O

pytestmark = pytest.mark.gpu


def _ctx():
    import torch
    from roibasedimagecompression_amd.ops import default_context
    rh = default_context()
    return rh, (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rh.device))


def _up_mask(up, m):
    return None if m is None else up(np.ascontiguousarray(m).view(np.uint8))


def check_stats(got, ref, what):
    """test 1's rule -> the largest |device - reference| / bound over the float sums"""
    sums, lbp, gray = got
    want, want_lbp, want_gray, _ = ref
    assert np.array_equal(lbp, want_lbp), (what, "lbp", lbp, want_lbp)
    assert np.array_equal(gray, want_gray), (what, "gray", gray, want_gray)
    assert sums[0] == want[0], (what, "count")
    err, bound = np.abs(sums - want), S.stats_tolerance(ref)
    assert (err <= bound).all(), (what, [(q, sums[q], want[q], err[q] / bound[q]) for q in np.nonzero(err > bound)[0]])
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ---- 1. raw split statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", S.ALL_SPLIT_SHAPES, ids=S.ids(S.ALL_SPLIT_SHAPES))
def test_split_stats_on_shape(shape):
    rh, up = _ctx()
    worst = 0.0
    for iname, img in S.split_images(*shape):
        t = up(img)
        for mname, m in S.split_masks(*shape):
            worst = max(worst, check_stats(rh.split_stats(t, _up_mask(up, m)), O.split_stats(img, m), (iname, mname)))
    print(f"split_stats {shape[0]}x{shape[1]}: largest error / bound = {worst:.3g}")


def _boxes_frame():
    """a 70 x 210 frame holding several split shapes as boxes at offsets that are no multiple of the 32 x 8 tile, in two label maps;
    a later box may paint over an earlier one's pixels, which makes the earlier mask ragged"""
    from roibasedimagecompression_amd import synth
    from roibasedimagecompression_amd.image import Region
    rng = np.random.default_rng(12)
    H, W = 70, 210
    img = synth.photo(H, W, 12, sigma=3.0)
    img[:, 100:] = img[:, 100:] // 8 + 100                                       # low contrast: unclipped colour scores
    places = [((9, 33), (3, 5)), ((17, 65), (1, 37)), ((8, 32), (21, 3)), ((1, 65), (31, 9)), ((17, 1), (33, 1)), ((7, 31), (35, 77)),
              ((16, 64), (19, 101)), ((2, 2), (67, 207)), ((1, 1), (69, 0)), ((15, 63), (45, 113)), ((17, 65), (50, 41)), ((9, 33), (37, 170)),
              ((2, 64), (66, 100)), ((1, 128), (0, 70))]
    maps, regions = [np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)], []
    for i, ((h, w), (y, x)) in enumerate(places):
        m = i % 2
        blob = np.ones((h, w), bool) if i % 3 == 0 else rng.random((h, w)) < 0.8
        maps[m][y:y + h, x:x + w][blob] = i + 1
        regions.append(Region(m, m, i + 1, (y, x, y + h, x + w), 0))
    return img, maps, regions


def test_batched_split_stats_vs_oracle():
    """ImageEncoder.split_stats (one launch over all boxes) against O.split_stats of every crop and mask"""
    from roibasedimagecompression_amd.image import ImageEncoder
    rh, up = _ctx()
    img, maps, regions = _boxes_frame()
    got = ImageEncoder(rh).split_stats(up(img), [up(m) for m in maps], regions)
    assert len(got) == len(regions)
    worst, counts = 0.0, []
    for r, g in zip(regions, got):
        y0, x0, y1, x1 = r.bbox
        ref = O.split_stats(img[y0:y1, x0:x1], maps[r.map][y0:y1, x0:x1] == r.label)
        counts.append(ref[0][0])
        worst = max(worst, check_stats(g, ref, r.bbox))
    assert min(counts) >= 1 and max(counts) >= 1000
    print(f"batched split_stats: largest error / bound = {worst:.3g}")


# ---- 2. the LBP rounding probe -------------------------------------------------------------------------------------------------------
def test_lbp_code_of_flat_patches():
    """the code of a flat neighbourhood is 8 or 9 by the rounding of the bilinear sample alone: the device rounds as the oracle does on
    all 256 gray levels and on 256 random colours, in one frame and level by level"""
    rh, up = _ctx()
    gray, colour, inner = S.lbp_probe_frames()
    for name, frame in (("gray", gray), ("colour", colour)):
        for mname, m in (("inner", inner), ("all", np.ones_like(inner))):
            _, lbp, gh = rh.split_stats(up(frame), _up_mask(up, m))
            want = O.split_stats(frame, m)
            assert np.array_equal(lbp, want[1]) and np.array_equal(gh, want[2]), (name, mname, lbp, want[1])
    assert O.split_stats(gray, inner)[1][9] == 9 * len(S.flat_levels_with_code_9()) > 0
    bad = []
    ones = up(np.ones((9, 33), np.uint8))
    for v in range(256):
        _, lbp, _ = rh.split_stats(up(S.flat_level(v)), ones)
        if not np.array_equal(lbp, O.split_stats(S.flat_level(v), np.ones((9, 33), bool))[1]):
            bad.append(v)
    assert not bad, bad


# ---- 3. score boundaries -----------------------------------------------------------------------------------------------------------
def test_score_boundaries():
    from roibasedimagecompression_amd.api.split_score import calculate_split_score
    contents = dict(S.split_images(17, 65))
    img, low = contents["photo"], contents["low"]                                # low: its colour score is not clipped
    cases = [(img, S.score_mask(17, 65, n)) for n in (99, 100, 101)] + [(S.dark_frame(n), None) for n in (99, 100)]
    cases += [(low, S.score_mask(17, 65, n)) for n in (100, 101)]
    kinds = []
    for im, m in cases:
        want, got = S.outcome(O.split_score, im, m), S.outcome(calculate_split_score, im, m)
        assert got[0] == want[0], (got, want)
        if want[0] == "raised":
            assert got[1] is want[1]
        else:
            assert np.allclose(got[1], want[1], rtol=0, atol=1e-9), (got, want)
        kinds.append(want[0] == "ok" and want[1][0] > 0)
    assert kinds == [False, True, True, False, True, True, True]
    assert 0.0 < O.split_score(low, S.score_mask(17, 65, 100))[1] < 1.0


# ---- 4. rhccq_slic_assign with chosen centroids ----------------------------------------------------------------------------------------
def _assign(rh, up, img, mask, seg, step, ignore_color, fill=-7):
    import torch
    H, W = mask.shape
    d_img, d_mask, d_seg = up(img), up(mask.view(np.uint8)), up(seg)
    d_lab = torch.full((H, W), fill, dtype=torch.int32, device=rh.device)
    rh._check(rh.lib.rhccq_slic_assign(rh.ctx, rh._p(d_img), rh._p(d_mask), rh._p(d_seg), H, W, len(seg), float(step), int(ignore_color), rh._p(d_lab)),
              "slic_assign")
    return d_lab.cpu().numpy()


ASSIGN_GROUPS = S.ids(S.SLIC_SHAPES) + ["chosen"]


@pytest.mark.parametrize("group", ASSIGN_GROUPS)
def test_slic_assign_vs_literal_loop(group):
    rh, up = _ctx()
    n = 0
    for i, (name, img, mask, seg, step) in enumerate(S.assign_cases()):
        grid = name.split("_")[0] in ASSIGN_GROUPS                              # "16x32_K255_step2.5"; the chosen cases start with a word
        if (name.split("_")[0] if grid else "chosen") != group:
            continue
        for ic in (True, False):
            want = S.assign_reference(i, ic)[0]
            got = _assign(rh, up, img, mask, seg, step, ic)
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, ic, int((got != want).sum()))
        n += 1
    assert n >= 6


def test_slic_assign_refuses_more_centroids_than_fit():
    from roibasedimagecompression_amd._lib import RhccqError
    rh, up = _ctx()
    rng = np.random.default_rng(1)
    K = S.K_LDS_MAX + 1
    seg = np.concatenate([rng.uniform(0, 16, (K, 1)), rng.uniform(0, 32, (K, 1)), np.zeros((K, 3))], axis=1)
    with pytest.raises(RhccqError, match="centroids"):
        _assign(rh, up, np.zeros((16, 32, 3)), S.full_mask(16, 32), seg, 2.0, True)
    # nothing was launched: run it again by hand and look at the label buffer
    import torch
    d_img, d_mask, d_seg = up(np.zeros((16, 32, 3))), up(np.ones((16, 32), np.uint8)), up(seg)
    d_lab = torch.full((16, 32), -7, dtype=torch.int32, device=rh.device)
    rc = rh.lib.rhccq_slic_assign(rh.ctx, rh._p(d_img), rh._p(d_mask), rh._p(d_seg), 16, 32, K, 2.0, 1, rh._p(d_lab))
    torch.cuda.synchronize()
    assert rc != 0 and (d_lab.cpu().numpy() == -7).all()
    assert (_assign(rh, up, np.zeros((16, 32, 3)), S.full_mask(16, 32), seg[:-1], 2.0, True) > 0).any()      # K = 1097 runs


# ---- 5. rhccq_slic_sweeps_regions called directly --------------------------------------------------------------------------------------
def test_slic_sweeps_regions_vs_oracle():
    """several regions of different sizes and K in one call, the 256-pixel padding between them: labels identical and the final centroid
    table bit-identical (bytes: -0.0 and NaN count) to O.slic_sweeps run twice per region -- the centroid means add in raster order as
    np.bincount does; the region with no masked pixel in any window stops after its first sweep and keeps its seeds"""
    import torch
    from roibasedimagecompression_amd.image import _block_tables
    rh, up = _ctx()
    regions, ref = S.sweep_regions(), S.sweep_reference()
    px_off, seg_off, tab = 0, 0, []
    for img, mask, seg, step in regions:
        tab.append((px_off, mask.shape[0], mask.shape[1], len(seg), seg_off))
        px_off += (mask.size + 255) // 256 * 256
        seg_off += len(seg)
    rng = np.random.default_rng(2)
    img_all = rng.normal(0, 3, (px_off, 3))                                      # the padding holds values and set mask bytes: never read
    mask_all = np.ones(px_off, np.uint8)
    for (o, h, w, K, so), (img, mask, seg, step) in zip(tab, regions):
        img_all[o:o + h * w] = img.reshape(-1, 3)
        mask_all[o:o + h * w] = mask.reshape(-1)
    tab = np.array(tab, np.int32)
    item, first = _block_tables(tab[:, 1].astype(np.int64) * tab[:, 2])
    seg_region = np.repeat(np.arange(len(tab), dtype=np.int32), tab[:, 3])
    assert len(seg_region) % 4 != 0
    wb = int(rh.lib.rhccq_slic_regions_work_bytes(len(tab), S.SWEEP_ITERS))
    d = [up(a) for a in (img_all, mask_all, np.concatenate([r[2] for r in regions]), tab, np.array([r[3] for r in regions]), item, first, seg_region)]
    work = torch.empty((wb,), dtype=torch.uint8, device=rh.device)
    labels = torch.full((px_off,), -7, dtype=torch.int32, device=rh.device)
    rh._check(rh.lib.rhccq_slic_sweeps_regions(rh.ctx, rh._p(d[0]), rh._p(d[1]), rh._p(d[2]), rh._p(d[3]), rh._p(d[4]), len(tab), int(tab[:, 3].max()),
                                               rh._p(d[5]), rh._p(d[6]), len(item), rh._p(d[7]), len(seg_region), S.SWEEP_ITERS, rh._p(work), wb,
                                               rh._p(labels)), "slic_sweeps_regions")
    labels, seg = labels.cpu().numpy(), d[2].cpu().numpy()
    inside = np.zeros(px_off, bool)
    for r, ((o, h, w, K, so), (want_lab, want_seg)) in enumerate(zip(tab, ref)):
        inside[o:o + h * w] = True
        got = labels[o:o + h * w].reshape(h, w)
        assert np.array_equal(got, want_lab), (r, int((got != want_lab).sum()))
        assert seg[so:so + K].tobytes() == want_seg.tobytes(), (r, seg[so:so + K], want_seg)
    assert (labels[~inside] == -7).all()                                         # the padding between the regions is not written


# ---- 6. resize at thin shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", S.RESIZE_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}->{s[1][0]}x{s[1][1]}")
def test_resize_thin_shapes(shapes):
    """gauss1d_kernel with a radius beyond the axis length (its mirror index wraps several times) and axes of length 1, the two zoom
    kernels at one row / one column: bit-identical to scipy"""
    from roibasedimagecompression_amd.api.slic import _resize
    (h, w), (oh, ow) = shapes
    rng = np.random.default_rng(h * 7 + w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for aa in (True, False):
        got, want = _resize(img, (oh, ow), 1, aa), O.sk_resize(img, (oh, ow), 1, aa)
        assert got.dtype == want.dtype == np.float64 and got.shape == want.shape and got.tobytes() == want.tobytes(), (aa, np.abs(got - want).max())
    mask = rng.random((h, w)) < 0.6
    got, want = _resize(mask, (oh, ow), 0, False), O.sk_resize(mask, (oh, ow), 0, False)
    assert got.shape == want.shape and np.array_equal(got, want)
    lab = rng.integers(0, 90, (oh, ow)).astype(np.int32)
    got, want = _resize(lab, (h, w), 0, False), O.sk_resize(lab, (h, w), 0, False)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


# ---- 7. whole masked SLIC at degenerate regions ------------------------------------------------------------------------------------------
def test_enhanced_slic_on_degenerate_regions():
    from roibasedimagecompression_amd.api.slic import enhanced_slic_with_texture
    for ragged in (False, True):
        for img, mask, n in S.slic_region_inputs(ragged):
            want = O.enhanced_slic(img, mask, n_segments=n)
            got, _ = enhanced_slic_with_texture(img, mask, n_segments=n)
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (img.shape, n, ragged)


def _slic_frame(inputs):
    """every region as a box of one frame, stacked on shelves -> (frame, label map, regions)"""
    from roibasedimagecompression_amd.image import Region
    W = max(i[0].shape[1] for i in inputs) + 7
    y, x, shelf, boxes = 1, 3, 0, []
    for img, mask, n in inputs:
        h, w = mask.shape
        if x + w > W:
            y, x, shelf = y + shelf + 1, 3, 0
        boxes.append((y, x))
        x, shelf = x + w + 2, max(shelf, h)
    H = y + shelf + 2
    frame = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    lab, regions = np.zeros((H, W), np.int32), []
    for i, ((img, mask, n), (y, x)) in enumerate(zip(inputs, boxes)):
        h, w = mask.shape
        frame[y:y + h, x:x + w] = img
        lab[y:y + h, x:x + w][mask] = i + 1
        regions.append(Region(0, 0, i + 1, (y, x, y + h, x + w), int(mask.sum())))
    return frame, lab, regions


def test_batched_slic_on_degenerate_regions():
    """ImageEncoder.slic, one call over all the regions (full and ragged masks), against O.enhanced_slic: its small label maps, upscaled
    by the oracle's nearest-neighbour resize, are the oracle's label maps"""
    from roibasedimagecompression_amd.image import ImageEncoder
    rh, up = _ctx()
    inputs = S.slic_region_inputs(False) + S.slic_region_inputs(True)
    frame, lab, regions = _slic_frame(inputs)
    small = ImageEncoder(rh).slic(frame, up(frame), [up(lab), up(np.zeros_like(lab))], regions, [n for _, _, n in inputs])
    assert len(small) == len(inputs)
    for (img, mask, n), s in zip(inputs, small):
        want = O.enhanced_slic(img, mask, n_segments=n)
        got = O.sk_resize(s, mask.shape, 0, False).astype(np.int32)
        assert np.array_equal(got, want), (img.shape, n)


def test_downscale_to_no_rows_raises_like_the_oracle():
    """(1, 600): scale 0.8 gives 0 rows; scipy's Gaussian raises OverflowError on the infinite sigma, and so do both device paths"""
    from roibasedimagecompression_amd.api.slic import enhanced_slic_with_texture
    from roibasedimagecompression_amd.image import ImageEncoder
    rh, up = _ctx()
    h, w, n = S.SLIC_RAISING
    img, mask = np.random.default_rng(6).integers(0, 256, (h, w, 3), dtype=np.uint8), S.full_mask(h, w)
    with np.errstate(divide="ignore"):
        want = S.outcome(O.enhanced_slic, img, mask, n_segments=n)
    frame, lab, regions = _slic_frame([(img, mask, n)])
    per_region = S.outcome(enhanced_slic_with_texture, img, mask, n_segments=n)
    batched = S.outcome(ImageEncoder(rh).slic, frame, up(frame), [up(lab), up(np.zeros_like(lab))], regions, [n])
    print("oracle", want, "enhanced_slic_with_texture", per_region, "ImageEncoder.slic", batched)
    assert want == ("raised", OverflowError)
    assert per_region[0] == batched[0] == "raised" and per_region[1] is want[1] and batched[1] is want[1]
