"""ImageEncoder (roibasedimagecompression_amd/image.py): image -> .rhccq in one device-resident flow, checked against flow.script_flow,
the reference-shaped chain it replaces.  GPU only.

Per image: the final palette, indices, dtype, shape and top_left are equal; the label layers (ClassSpecs) equal the ones
subregion_quantization hands to FrameEncoder.prepare; the exact=True files have the same sha256.  Intermediate stages: the batched
split statistics equal Rhccq.split_stats per region, the batched SLIC equals enhanced_slic_with_texture per region.  Residency: on the
4K mosaic the flow reads back less than one frame's H x W x 3 bytes (script_flow: six frames from the ROI stage alone)."""
import hashlib
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _png(name):
    return np.asarray(Image.open(os.path.join(G, name + ".png")).convert("RGB"), dtype=np.uint8)


def _mosaic():
    from roibasedimagecompression_amd import synth
    return synth.kodak_mosaic([_png(f"kodak_{i}") for i in range(1, 21)])


def _script_flow_with_specs(img, q1, q2, out_path):
    """script_flow(...) and the ClassSpecs its subregion_quantization calls pass to FrameEncoder.prepare (ROI call first)"""
    from roibasedimagecompression_amd.flow import script_flow
    from roibasedimagecompression_amd.frame import FrameEncoder
    seen, orig = [], FrameEncoder.prepare

    def prepare(self, rgb, classes):
        seen.extend((c.labels.cpu().numpy(), c.seg_region.copy(), c.region_bbox.copy(), c.quality) for c in classes)
        return orig(self, rgb, classes)
    FrameEncoder.prepare = prepare
    try:
        final, _, info = script_flow(img, q1, q2, out_path=out_path)
    finally:
        FrameEncoder.prepare = orig
    return final, info, seen


def _indices(res):
    idx = res["indices"].cpu().numpy()
    if res["indices_dtype"] == "uint16":
        idx = idx.view(np.uint16)
    return idx.reshape(-1).astype(np.int64)


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def _check_parity(img, tmp_path, q1=20, q2=10):
    from roibasedimagecompression_amd.image import ImageEncoder
    from roibasedimagecompression_amd.segment import as_index_array
    ref_path, my_path = str(tmp_path / "ref.rhccq"), str(tmp_path / "mine.rhccq")
    final, info, specs = _script_flow_with_specs(img, q1, q2, ref_path)
    res = ImageEncoder().encode(img, q1, q2, out_path=my_path, exact=True)
    assert np.array_equal(res["palette"], np.asarray(final["palette"], np.uint8).reshape(-1, 3))
    assert np.array_equal(_indices(res), np.asarray(as_index_array(final["indices"])).reshape(-1).astype(np.int64))
    assert res["indices_dtype"] == final["indices_dtype"]
    assert tuple(res["shape"]) == tuple(final["shape"]) and tuple(res["top_left"]) == tuple(final["top_left"])
    assert len(res["classes"]) == len(specs)
    for (call, spec), (labels, seg_region, bbox, quality) in zip(res["classes"], specs):
        assert np.array_equal(spec.labels.cpu().numpy(), labels)
        assert np.array_equal(spec.seg_region, seg_region) and np.array_equal(spec.region_bbox, bbox) and spec.quality == quality
    st = res["stats"]
    for k in ("roi_regions", "nonroi_regions", "roi_segments", "nonroi_segments", "segments_dropped"):
        assert st[k] == info[k], k
    assert st["region_map_roi_fraction"] == info["region_map_roi_fraction"] and st["edge_fraction"] == info["edge_fraction"]
    assert _sha(my_path) == _sha(ref_path)
    print(f"branches: regions {st['roi_regions']}/{st['nonroi_regions']}, layers {st['roi_layers']}/{st['nonroi_layers']}, "
          f"segments {st['roi_segments']}/{st['nonroi_segments']}, dropped {st['segments_dropped']}, "
          f"single component {tuple(res['shape']) != img.shape[:2]}")
    return res


@pytest.mark.parametrize("name", ["Lenna", "kodak_1", "kodak_3", "kodak_8", "kodak_13", "kodak_19", "kodak_23"])
def test_equal_to_script_flow(name, tmp_path):
    _check_parity(_png(name), tmp_path)


def test_equal_to_script_flow_tiny_crop(tmp_path):
    """no non-ROI region: script_flow's region_quantization of that call raises and is caught (`except: []`)"""
    res = _check_parity(np.ascontiguousarray(_png("kodak_5")[200:248, 300:364]), tmp_path)
    assert res["stats"]["nonroi_segments"] == 0 and res["stats"]["roi_segments"] > 0


def test_flat_image_raises_like_script_flow(tmp_path):
    """a flat image has no ROI; whatever script_flow does with it (a result or an exception), ImageEncoder does the same"""
    from roibasedimagecompression_amd.flow import script_flow
    from roibasedimagecompression_amd.image import ImageEncoder
    img = np.full((96, 128, 3), 120, np.uint8)
    try:
        script_flow(img, 20, 10, container=False)
    except Exception as e:                                                   # noqa: BLE001
        with pytest.raises(type(e)):
            ImageEncoder().encode(img, 20, 10)
        return
    _check_parity(img, tmp_path)


def test_equal_to_script_flow_4k_mosaic_and_resident(tmp_path):
    from roibasedimagecompression_amd.ops import Rhccq
    from roibasedimagecompression_amd.image import ImageEncoder
    img = _mosaic()
    assert img.shape == (2160, 3840, 3)
    st = _check_parity(img, tmp_path)["stats"]
    assert st["nonroi_layers"] > 1                                           # overlapping regions in separate layers
    # device-to-host bytes of the flow without the container
    moved = [0]
    o_cpu, o_to, o_host = torch.Tensor.cpu, torch.Tensor.to, Rhccq.to_host

    def cpu(self, *a, **k):
        if self.is_cuda:
            moved[0] += self.numel() * self.element_size()
        return o_cpu(self, *a, **k)

    def to(self, *a, **k):
        out = o_to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            moved[0] += self.numel() * self.element_size()
        return out

    def to_host(self, *ts):
        moved[0] += sum(t.numel() * t.element_size() for t in ts)
        return o_host(self, *ts)
    from roibasedimagecompression_amd.flow import script_flow
    enc = ImageEncoder()
    torch.Tensor.cpu, torch.Tensor.to, Rhccq.to_host = cpu, to, to_host
    try:
        script_flow(img, 20, 10, container=False)
        reference = moved[0]
        moved[0] = 0
        # the stages up to the label layers: what script_flow moves through the host (six frames from the ROI stage alone)
        regions, maps, rgb, _ = enc.regions(img)
        small = enc.slic(img, rgb, maps, regions, enc.split_segments(rgb, maps, regions))
        enc.layers(maps, regions, small, (20, 10))
        upstream = moved[0]
        enc.encode(img, 20, 10)
    finally:
        torch.Tensor.cpu, torch.Tensor.to, Rhccq.to_host = o_cpu, o_to, o_host
    total = moved[0] - upstream
    print("device-to-host bytes: script_flow", reference, "regions -> layers", upstream, "whole encode", total)
    assert 0 < upstream < total < img.size < reference


def test_round_trip(tmp_path):
    from roibasedimagecompression_amd import container
    from roibasedimagecompression_amd.image import ImageEncoder
    path = str(tmp_path / "x.rhccq")
    res = ImageEncoder().encode(_png("Lenna"), 20, 10, out_path=path)
    back = container.read_frame(path)
    pal, got = back["palette"], back["indices"]
    pal, got = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (pal, got))
    assert np.array_equal(pal.astype(np.uint8).reshape(-1, 3), res["palette"])
    if res["indices_dtype"] == "uint16":
        got = got.view(np.uint16)
    assert np.array_equal(got.reshape(-1).astype(np.int64), _indices(res))


def _random_regions(rng, H, W, n):
    """two label maps of random blobs and the Region list over them"""
    from roibasedimagecompression_amd.image import Region
    maps, regions = [], []
    for m in range(2):
        lab = np.zeros((H, W), np.int32)
        for k in range(1, n + 1):
            y0, x0 = rng.integers(0, H - 8), rng.integers(0, W - 8)
            h, w = rng.integers(2, min(H - y0, 120) + 1), rng.integers(2, min(W - x0, 160) + 1)
            blob = rng.random((h, w)) < rng.uniform(0.3, 1.0)
            sub = lab[y0:y0 + h, x0:x0 + w]
            sub[blob] = k
        maps.append(lab)
    for m, lab in enumerate(maps):
        for k in range(1, n + 1):
            ys, xs = np.nonzero(lab == k)
            if len(ys):
                regions.append(Region(m, m, k, (int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1), len(ys)))
    return maps, regions


def test_batched_split_stats_equal_per_region():
    from roibasedimagecompression_amd.image import ImageEncoder
    enc = ImageEncoder()
    rh = enc.rh
    rng = np.random.default_rng(7)
    img = _png("kodak_7")
    H, W = img.shape[:2]
    maps, regions = _random_regions(rng, H, W, 6)
    rgb = torch.from_numpy(img).to(rh.device)
    d_maps = [torch.from_numpy(m).to(rh.device) for m in maps]
    got = enc.split_stats(rgb, d_maps, regions)
    for r, (sums, lbp, gray) in zip(regions, got):
        y0, x0, y1, x1 = r.bbox
        crop = torch.from_numpy(np.ascontiguousarray(img[y0:y1, x0:x1])).to(rh.device)
        mask = torch.from_numpy(np.ascontiguousarray(maps[r.map][y0:y1, x0:x1] == r.label).view(np.uint8)).to(rh.device)
        s2, l2, g2 = rh.split_stats(crop, mask)
        assert sums.tobytes() == s2.tobytes() and np.array_equal(lbp, l2) and np.array_equal(gray, g2)


def test_batched_slic_equal_per_region():
    """K = 1, masks under 100 pixels and large regions that are downscaled, against enhanced_slic_with_texture"""
    from roibasedimagecompression_amd.api.slic import enhanced_slic_with_texture
    from roibasedimagecompression_amd.image import ImageEncoder, Region
    enc = ImageEncoder()
    rh = enc.rh
    img = _png("kodak_11")
    H, W = img.shape[:2]
    rng = np.random.default_rng(3)
    maps, regions = _random_regions(rng, H, W, 4)
    maps[1][:] = 0
    maps[1][20:500, 10:700] = (rng.random((480, 690)) < 0.9) * 1                # a region wider than 500 px: downscaled
    ys, xs = np.nonzero(maps[1])
    regions = [r for r in regions if r.map == 0] + [Region(1, 1, 1, (int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1), len(ys))]
    n_seg = [1, 3, 17, 5, 40, 2, 9, 60][:len(regions) - 1] + [30]
    d_maps = [torch.from_numpy(m).to(rh.device) for m in maps]
    rgb = torch.from_numpy(img).to(rh.device)
    small = enc.slic(img, rgb, d_maps, regions, n_seg)
    for r, n, s in zip(regions, n_seg, small):
        y0, x0, y1, x1 = r.bbox
        ref, _ = enhanced_slic_with_texture(img[y0:y1, x0:x1], maps[r.map][y0:y1, x0:x1] == r.label, n_segments=n)
        yi, xi = enc._nearest_tables(s.shape[0], y1 - y0), enc._nearest_tables(s.shape[1], x1 - x0)
        assert np.array_equal(s[yi][:, xi], ref), (r.bbox, n)


def test_vanishing_mask_raises_like_enhanced_slic():
    """a region whose mask is lost by the nearest-neighbour downscale: both paths raise ValueError (kmeans2 on no coordinates)"""
    from roibasedimagecompression_amd.api.slic import enhanced_slic_with_texture
    from roibasedimagecompression_amd.image import ImageEncoder, Region
    enc = ImageEncoder()
    rh = enc.rh
    img = np.ascontiguousarray(np.tile(_png("kodak_2"), (2, 2, 1))[:1000, :1000])
    lab = np.zeros((1000, 1000), np.int32)
    y = np.arange(999)
    lab[y, y + 1] = 1                                                        # scale 0.5 samples odd rows and odd columns only
    with pytest.raises(ValueError):
        enhanced_slic_with_texture(img, lab == 1, n_segments=5)
    d_maps = [torch.from_numpy(lab).to(rh.device), torch.zeros_like(torch.from_numpy(lab)).to(rh.device)]
    with pytest.raises(ValueError):
        enc.slic(img, torch.from_numpy(img).to(rh.device), d_maps, [Region(0, 0, 1, (0, 0, 1000, 1000), 999)], [5])


def test_layers_equal_subregion_quantization_with_dropped_segments():
    """synthetic regions and SLIC maps through ImageEncoder.layers and through subregion_quantization (segmenter hook): segments that
    fill their box are dropped, regions of the two maps overlap, and one call ends up with no segment at all"""
    from roibasedimagecompression_amd.api import subregions as sub
    from roibasedimagecompression_amd.frame import FrameEncoder
    from roibasedimagecompression_amd.image import ImageEncoder, Region
    enc = ImageEncoder()
    rh = enc.rh
    img = _png("kodak_4")[:200, :240].copy()
    H, W = img.shape[:2]
    maps = [np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)]
    maps[0][10:40, 10:60] = 1                      # ROI region 1: a full box
    maps[0][100:150, 30:90] = 2                    # ROI region 2 (handed to the non-ROI call), overlapping non-ROI region 1
    maps[1][80:190, 20:200] = 1
    maps[1][100:150, 30:90] = 1
    maps[1][5:60, 150:230] = 2
    regions = [Region(0, 0, 1, (10, 10, 40, 60), 1500), Region(1, 1, 1, (80, 20, 190, 200), int((maps[1] == 1).sum())),
               Region(1, 1, 2, (5, 150, 60, 230), 55 * 80), Region(1, 0, 2, (100, 30, 150, 90), 3000)]
    rng = np.random.default_rng(5)
    segs = [np.ones((30, 50), np.int32),                                          # fills its box: dropped, the ROI call is empty
            rng.integers(1, 4, size=(110, 180)).astype(np.int32),
            np.ones((55, 80), np.int32),                                          # fills its box: dropped
            np.where(np.arange(60) < 30, 1, 2)[None, :].repeat(50, 0).astype(np.int32)]   # two halves: kept, in a second layer
    d_maps = [torch.from_numpy(m).to(rh.device) for m in maps]
    classes, place, stats = enc.layers(d_maps, regions, segs, (20, 10))
    assert stats[0]["segments"] == 0 and stats[0]["segments_dropped"] == 1 and stats[1]["segments_dropped"] == 1
    ref, seen, orig = [], [], FrameEncoder.prepare

    def prepare(self, rgb, cls):
        seen.extend((c.labels.cpu().numpy(), c.seg_region.copy(), c.region_bbox.copy(), c.quality) for c in cls)
        return orig(self, rgb, cls)
    FrameEncoder.prepare = prepare
    try:
        for call, q in ((0, 20), (1, 10)):
            idx = [i for i, r in enumerate(regions) if r.call == call]
            dicts = [{"bbox": regions[i].bbox, "bbox_mask": (maps[regions[i].map] == regions[i].label)[regions[i].bbox[0]:regions[i].bbox[2],
                                                                                                        regions[i].bbox[1]:regions[i].bbox[3]]}
                     for i in idx]
            it = iter([segs[i] for i in idx])
            sub.subregion_quantization(img, dicts, quality=q, segmenter=lambda crop, mask: next(it))
            ref.append(dict(sub.last_stats))
    finally:
        FrameEncoder.prepare = orig
    for call in (0, 1):
        assert stats[call]["segments"] == ref[call]["segments"] and stats[call]["segments_dropped"] == ref[call]["segments_dropped"]
        assert stats[call]["layers"] == ref[call]["layers"]
    assert stats[1]["layers"] == 2
    assert len(classes) == len(seen)
    for (call, spec), (labels, seg_region, bbox, quality) in zip(classes, seen):
        assert np.array_equal(spec.labels.cpu().numpy(), labels)
        assert np.array_equal(spec.seg_region, seg_region) and np.array_equal(spec.region_bbox, bbox) and spec.quality == quality
