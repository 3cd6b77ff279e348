"""Host-side helpers of ImageEncoder (roibasedimagecompression_amd/image.py); no GPU needed.

The layer placement is checked against subregion_quantization's own rule, restated with full-frame numpy masks: a region goes to the
first layer whose painted pixels miss its mask, and its kept segments are numbered per layer."""
import numpy as np
import torch

from roibasedimagecompression_amd.image import Region, _block_tables, _pack_bits, overlap_candidates, place_layers


def test_block_tables():
    item, first = _block_tables([1, 256, 257, 0, 600])
    assert first.tolist() == [0, 1, 2, 4, 4]
    assert item.tolist() == [0, 1, 2, 2, 4, 4, 4]


def test_pack_bits_matches_numpy():
    rng = np.random.default_rng(1)
    for n in (1, 7, 8, 9, 1000):
        m = (rng.random(n) < 0.4).astype(np.uint8)
        got = _pack_bits(torch.from_numpy(m)).numpy()
        assert np.array_equal(got, np.packbits(m, bitorder="little"))
        assert np.array_equal(np.unpackbits(got, bitorder="little")[:n], m)


def _scene(rng, H=64, W=80):
    """an ROI label map and a non-ROI label map that overlap in places, their region list as extract_regions orders it (small ROI
    regions last in the non-ROI call), and a random SLIC label map per region box"""
    maps = [np.zeros((H, W), np.int32), np.zeros((H, W), np.int32)]
    for m, n in ((0, 4), (1, 3)):
        for k in range(1, n + 1):
            y0, x0 = rng.integers(0, H - 10), rng.integers(0, W - 10)
            h, w = rng.integers(2, 30), rng.integers(2, 30)
            maps[m][y0:y0 + h, x0:x0 + w][rng.random((min(h, H - y0), min(w, W - x0))) < 0.8] = k
    regs = []
    for m in (0, 1):
        for k in range(1, int(maps[m].max()) + 1):
            ys, xs = np.nonzero(maps[m] == k)
            if len(ys):
                regs.append(Region(m, m, k, (int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1), len(ys)))
    roi = [r for r in regs if r.map == 0]
    small = roi[-2:]                                           # two ROI regions handed to the non-ROI call
    for r in small:
        r.call = 1
    regions = roi[:-2] + [r for r in regs if r.map == 1] + small
    segs = [rng.integers(0, 4, size=r.hw).astype(np.int32) for r in regions]
    return maps, regions, segs


def _mask(maps, r):
    y0, x0, y1, x1 = r.bbox
    return maps[r.map][y0:y1, x0:x1] == r.label


def test_layer_placement_matches_subregion_quantization():
    for seed in range(20):
        rng = np.random.default_rng(seed)
        maps, regions, segs = _scene(rng)
        H, W = maps[0].shape
        # kept ids: present in the mask and not filling the box (find_contours' drop rule)
        kept = []
        for r, s in zip(regions, segs):
            m = _mask(maps, r)
            h, w = r.hw
            kept.append([int(v) for v in np.unique(s[m]) if v and not (h >= 2 and w >= 2 and ((s == v) & m).all())])
        # reference: subregion_quantization's loop per call
        ref = []
        for call in (0, 1):
            layers = []
            for i, r in enumerate(regions):
                if r.call != call:
                    continue
                y0, x0, y1, x1 = r.bbox
                m = _mask(maps, r)
                layer = next((l for l in layers if not l["labels"][y0:y1, x0:x1][m].any()), None)
                if layer is None:
                    layer = {"labels": np.zeros((H, W), np.int32), "n": 0}
                    layers.append(layer)
                view = layer["labels"][y0:y1, x0:x1]
                for v in kept[i]:
                    layer["n"] += 1
                    view[(segs[i] == v) & m] = layer["n"]
            ref += [l["labels"] for l in layers if l["n"]]
        # ImageEncoder's placement from the pairwise overlap flags
        painted = []
        for r, s, k in zip(regions, segs, kept):
            full = np.zeros((H, W), bool)
            y0, x0, y1, x1 = r.bbox
            full[y0:y1, x0:x1] = _mask(maps, r) & np.isin(s, k)
            painted.append(full)
        hit = {}
        for i, j in overlap_candidates(regions, [bool(k) for k in kept]):
            y0, x0, y1, x1 = regions[i].bbox
            m = np.zeros((H, W), bool)
            m[y0:y1, x0:x1] = _mask(maps, regions[i])
            hit[(i, j)] = bool((m & painted[j]).any())
        for i in range(len(regions)):                            # pairs left out can never meet
            for j in range(i):
                if (i, j) not in hit and regions[i].call == regions[j].call:
                    y0, x0, y1, x1 = regions[i].bbox
                    assert not (painted[j][y0:y1, x0:x1] & _mask(maps, regions[i])).any()
        layers, place = place_layers(regions, kept, hit)
        got = []
        for call, l in layers:
            lab = np.zeros((H, W), np.int32)
            for n, (i, v) in enumerate(l["segments"], 1):
                y0, x0, y1, x1 = regions[i].bbox
                lab[y0:y1, x0:x1][(segs[i] == v) & _mask(maps, regions[i])] = n
            got.append(lab)
        assert len(got) == len(ref), seed
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), seed
