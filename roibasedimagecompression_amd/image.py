"""Image -> .rhccq in one device-resident flow: ImageEncoder.encode computes what flow.script_flow computes (encoder/compression/
test.py:77-151: get_regions, extract_regions, subregion_quantization per class, region_quantization per class, quantize_image),
bit for bit, without the host round trips of the reference-shaped functions.

  regions      the resident get_regions chain stops at the device masks; both are labelled on the device (Rhccq.ccl) and only the
               stats tables come back.  A region is (call, label map, label, bbox): no RegionDict, no bbox_mask.
  split score  every region's masked statistics in ONE launch (rhccq_split_stats_regions, the tiles rhccq_split_stats uses on the
               crop), one read-back; scores_from_stats / normalize_result on the host as before.
  SLIC         the resizes on the device (the gauss1d / zoom kernels of api/slic.py); the <= 500 x 500 images and masks come back in
               one copy, the Lab image, its sigma-1 Gaussian and the centroid seeding stay the host code of slic_masked; the 2 x 10 sweeps
               of all regions run with no read-back (rhccq_slic_sweeps_regions); the labels come back in one copy for the
               connectivity pass (host) and go up again in one copy.
  layers       the upscale is never materialised: per-(region, SLIC id) in-mask counts (drop test included), the overlap test that
               places a region in its layer, and the painting of the int32 layers are three launches (csrc/image_flow.hip).
  levels       FrameEncoder.prepare / level1 over all layers, level 2 per call (FrameEncoder.level2_jobs groups), level 3, remap.
The ROI and SLIC stages are the same parity-unpinned restatements script_flow runs."""
import ctypes as C
import math
import os
import time

import numpy as np
import torch

from .api import roi_chain
from .api.roi import min_region_size
from .api.slic import _antialias_sigma_radius, _gaussian_weights, _mask_centroids, _mirror_index, _rgb2lab, _zoom_coordinates
from .api.split_score import normalize_result, scores_from_stats
from .frame import ClassSpec, FrameEncoder
from . import ops
from .ops import RhccqError, default_context, psnr_from_sse
from .palette import cluster_palettes

__all__ = ["ImageEncoder", "Region"]

_SLIC_SWEEPS = 10          # slic_masked's max_num_iter
_COMPACTNESS = 10.0        # enhanced_slic_with_texture's compactness


class Region:
    """One region of extract_regions: call 0 = ROI / 1 = non-ROI list, map 0 = ROI / 1 = non-ROI label map, its label there and
    its bbox (minr, minc, maxr, maxc)"""
    __slots__ = ("call", "map", "label", "bbox", "area")

    def __init__(self, call, map_, label, bbox, area):
        self.call, self.map, self.label, self.bbox, self.area = call, map_, label, bbox, area

    @property
    def hw(self):
        return self.bbox[2] - self.bbox[0], self.bbox[3] - self.bbox[1]


def _block_tables(sizes, per_block=256):
    """consecutive workgroups over items of `sizes` units: (block_item, block_first) int32"""
    nb = (np.asarray(sizes, np.int64) + per_block - 1) // per_block
    first = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int32)
    return np.repeat(np.arange(len(nb), dtype=np.int32), nb), first


def overlap_candidates(regions, painted):
    """pairs (i, j), j < i, of regions of one call, of different label maps, with intersecting boxes and region j painting some
    pixel (painted[j]): the only pairs whose pixels can meet (regions of one map are disjoint).  In extract_regions' lists these are
    the small ROI regions at the end of the non-ROI list against the non-ROI regions before them."""
    if not regions:
        return []
    call = np.array([r.call for r in regions])
    map_ = np.array([r.map for r in regions])
    bb = np.array([r.bbox for r in regions], np.int64).reshape(-1, 4)
    painted = np.asarray(painted, bool)
    pairs = []
    for i in np.nonzero(map_ != call)[0]:                  # a region listed in the other map's call
        j = np.arange(i)
        ok = (call[j] == call[i]) & (map_[j] != map_[i]) & painted[j]
        ok &= (np.maximum(bb[j, 0], bb[i, 0]) < np.minimum(bb[j, 2], bb[i, 2])) & (np.maximum(bb[j, 1], bb[i, 1]) < np.minimum(bb[j, 3], bb[i, 3]))
        pairs += [(int(i), int(q)) for q in j[ok]]
    return pairs


def place_layers(regions, kept, hit):
    """subregion_quantization's layer placement: per call, in list order, a region goes to the first layer none of whose painted
    pixels lie in its mask (hit[(i, j)]: region i's mask meets region j's painted pixels), else to a new layer; layers that end
    up with no segment are dropped.  kept[i]: region i's kept SLIC ids, ascending.
    -> ([(call, {"members", "bboxes", "seg_region", "segments": [(region, id)] in id order})], per region (layer, local index) or
    (-1, -1))"""
    out, place = [], [(-1, -1)] * len(regions)
    for call in (0, 1):
        layers = []
        for i, r in enumerate(regions):
            if r.call != call:
                continue
            layer = next((l for l in layers if not any(hit.get((i, j), False) for j in l["members"])), None)
            if layer is None:
                layer = {"members": [], "bboxes": [], "seg_region": [], "segments": []}
                layers.append(layer)
            local = len(layer["members"])
            layer["members"].append(i)
            layer["bboxes"].append(r.bbox)
            for s in kept[i]:
                layer["segments"].append((i, s))
                layer["seg_region"].append(local)
        for l in layers:
            if l["segments"]:
                for local, i in enumerate(l["members"]):
                    place[i] = (len(out), local)
                out.append((call, l))
    return out, place


def _pack_bits(mask_u8):
    """device uint8 0 / 1 [n] -> uint8[ceil(n / 8)], bit i % 8 of byte i / 8 (np.unpackbits(bitorder="little") order)"""
    n = mask_u8.numel()
    padded = torch.zeros(((n + 7) // 8) * 8, dtype=torch.int32, device=mask_u8.device)
    padded[:n] = mask_u8
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=mask_u8.device)
    return (padded.view(-1, 8) * weights).sum(dim=1).to(torch.uint8)


class ImageEncoder:
    def __init__(self, rh=None):
        self.rh = rh or default_context()
        self.region_map = None         # device uint8[H,W] 0 / 1 region map of the last regions() call

    # ---- stage 1 ---------------------------------------------------------------------------------------------------------------
    def regions(self, image, roi_mask=None):
        """get_regions + extract_regions on the device -> (regions [Region] in the order of the ROI list then the non-ROI list,
        label maps (ROI, non-ROI) device int32[H,W], uploaded RGB, stats).  roi_mask: a caller's bool / uint8 [H,W] mask (numpy or
        device tensor) instead of the detector.  The 0 / 1 device region map of the call stays in self.region_map."""
        rh = self.rh
        if roi_mask is None:
            unified, region_map, _, _, roi_mask, non_mask, rgb = roi_chain.get_regions_resident(image, rh)
            source = {}
        else:
            unified, region_map, _, _, roi_mask, non_mask, rgb = roi_chain.regions_from_mask_resident(image, roi_mask, rh)
            source = {"roi_source": "caller"}
        self.region_map = region_map
        frac = rh.to_host(torch.stack([region_map.sum(dtype=torch.int64), (unified != 0).sum(dtype=torch.int64)]))
        n1, lab1, st1 = rh.ccl(roi_mask, 8)
        n0, lab0, st0 = rh.ccl(non_mask, 8)
        mn = min_region_size(image)

        def listed(call, map_, n, st):
            out = []
            for lab in range(1, n + 1):
                x, y, w, h, area = (int(v) for v in st[lab])
                out.append(Region(call, map_, lab, (y, x, y + h, x + w), area))
            return out
        roi, non = listed(0, 0, n1, st1), listed(1, 1, n0, st0)
        small = [r for r in roi if r.area < mn]                    # roi.py:76-84: small ROI regions go to the end of the non-ROI list
        for r in small:
            r.call = 1
        non += small
        roi = [r for r in roi if r.area >= mn]
        hw = image.shape[0] * image.shape[1]
        stats = {"region_map_roi_fraction": float(frac[0]) / hw, "edge_fraction": float(frac[1]) / hw,
                 "roi_regions": len(roi), "nonroi_regions": len(non), **source}
        return roi + non, (lab1, lab0), rgb, stats

    # ---- stage 2 ---------------------------------------------------------------------------------------------------------------
    def split_stats(self, rgb, maps, regions):
        """Rhccq.split_stats of every region's crop and mask in one launch and one read-back -> [(sums, lbp_hist, gray_hist)]"""
        rh = self.rh
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        if not regions:
            return []
        table = np.array([[r.bbox[0], r.bbox[1], r.hw[0], r.hw[1], r.map, r.label] for r in regions], np.int32)
        nb = np.array([rh.lib.rhccq_split_stats_blocks(int(h), int(w)) for h, w in table[:, 2:4]], np.int64)
        first = np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.int32)
        item = np.repeat(np.arange(len(nb), dtype=np.int32), nb)
        part = rh.empty((int(nb.sum()), 12), torch.float64)
        hist = rh.empty((len(regions), 42), torch.int32)
        d_t, d_i, d_f = rh.dev(table), rh.dev(item), rh.dev(first)
        rh._check(rh.lib.rhccq_split_stats_regions(rh.ctx, rh._p(rgb), H, W, rh._p(maps[0]), rh._p(maps[1]), rh._p(d_t), len(regions), rh._p(d_i),
                                                   rh._p(d_f), int(nb.sum()), rh._p(part), rh._p(hist)), "split_stats_regions")
        part_h, hist_h = rh.to_host(part, hist)
        hist_h = hist_h.astype(np.int64)
        return [(part_h[first[k]:first[k] + nb[k]].sum(axis=0), hist_h[k, :10], hist_h[k, 10:]) for k in range(len(regions))]

    def split_segments(self, rgb, maps, regions):
        """_reference_segmenter's segment count of every region"""
        overall = np.zeros(len(regions))
        scored = [i for i, r in enumerate(regions) if r.area >= 100]   # split_score.py:25-27
        for i, (sums, lbp, gray) in zip(scored, self.split_stats(rgb, maps, [regions[i] for i in scored])):
            if sums[0] >= 100:
                overall[i] = scores_from_stats(sums, lbp, gray)[0]
        out = []
        for i, r in enumerate(regions):
            size = r.hw[0] * r.hw[1] * 3
            window = math.ceil(math.ceil(math.log(size, 10)) * math.log(size))
            optimal = math.ceil(normalize_result(overall[i], window))
            out.append(optimal if optimal > 0 else 1)
        return out

    # ---- stage 3 ---------------------------------------------------------------------------------------------------------------
    def _resize_linear(self, crop_u8, lo, hi, oh, ow):
        """api/slic.py _resize(order 1, anti_aliasing) of a device uint8[h,w,3] crop, device float64 out"""
        rh = self.rh
        H, W = int(crop_u8.shape[0]), int(crop_u8.shape[1])
        work = crop_u8.to(torch.float64)
        keep = []
        for axis, (n_in, n_out) in enumerate(((H, oh), (W, ow))):
            sigma, radius = _antialias_sigma_radius(n_in, n_out)
            if sigma <= 1e-15:
                continue
            outer, length, inner = (1, H, W * 3) if axis == 0 else (H, W, 3)
            nxt = torch.empty_like(work)
            d_w = rh.dev(_gaussian_weights(sigma, radius))
            rh._check(rh.lib.rhccq_gauss1d_f64(rh.ctx, rh._p(work), outer, length, inner, rh._p(d_w), radius, rh._p(nxt)), "gauss1d_f64")
            keep += [work, d_w]
            work = nxt
        cy, cx = _zoom_coordinates(H, oh), _zoom_coordinates(W, ow)
        y0, x0 = np.floor(cy).astype(np.int64), np.floor(cx).astype(np.int64)
        ty, tx = cy - np.floor(cy), cx - np.floor(cx)
        yi = np.stack([_mirror_index(y0, H), _mirror_index(y0 + 1, H)]).astype(np.int32)
        xi = np.stack([_mirror_index(x0, W), _mirror_index(x0 + 1, W)]).astype(np.int32)
        wy, wx = np.stack([1 - ty, ty]), np.stack([1 - tx, tx])
        out = rh.empty((oh, ow, 3), torch.float64)
        d_yi, d_wy, d_xi, d_wx = rh.dev(yi), rh.dev(wy), rh.dev(xi), rh.dev(wx)
        rh._check(rh.lib.rhccq_zoom_linear_f64(rh.ctx, rh._p(work), H, W, 3, rh._p(d_yi), rh._p(d_wy), rh._p(d_xi), rh._p(d_wx), oh, ow,
                                               float(lo), float(hi), rh._p(out)), "zoom_linear_f64")
        keep += [work, d_yi, d_wy, d_xi, d_wx]
        return out, keep

    @staticmethod
    def _nearest_tables(n_in, n_out):
        return _mirror_index(np.floor(_zoom_coordinates(n_in, n_out) + 0.5).astype(np.int64), n_in).astype(np.int32)

    def _resize_mask(self, mask_u8, oh, ow):
        rh = self.rh
        H, W = int(mask_u8.shape[0]), int(mask_u8.shape[1])
        d_yi, d_xi = rh.dev(self._nearest_tables(H, oh)), rh.dev(self._nearest_tables(W, ow))
        out = rh.empty((oh, ow), torch.uint8)
        rh._check(rh.lib.rhccq_zoom_nearest(rh.ctx, rh._p(mask_u8), 1, H, W, 1, rh._p(d_yi), rh._p(d_xi), oh, ow, rh._p(out)), "zoom_nearest")
        return out, [mask_u8, d_yi, d_xi]

    def slic(self, image, rgb, maps, regions, n_segments):
        """enhanced_slic_with_texture of every region -> per region (small connected labels int32[nh,nw] host, (nh, nw))"""
        from scipy import ndimage as ndi
        rh = self.rh
        smalls, masks, sizes, keep = [], [], [], []
        for r, n in zip(regions, n_segments):
            minr, minc, maxr, maxc = r.bbox
            h, w = r.hw
            scale = round(500 / max(h, w, 3), 1)
            if scale > 1:
                scale = 1
            nh, nw = int(h * scale), int(w * scale)
            crop = image[minr:maxr, minc:maxc]
            lin, k = self._resize_linear(rgb[minr:maxr, minc:maxc].contiguous(), crop.min(), crop.max(), nh, nw)
            keep += k
            smalls.append(lin.to(torch.uint8).reshape(-1, 3))
            m, k = self._resize_mask((maps[r.map][minr:maxr, minc:maxc] == r.label).to(torch.uint8).contiguous(), nh, nw)
            keep += k
            masks.append(m.reshape(-1))
            sizes.append((nh, nw, math.ceil(n * scale * scale)))
        if not regions:
            return []
        # one read-back: the small masks as bits and the colours of their in-mask pixels only (what slic_masked reads: it zeroes the rest)
        mask_cat = torch.cat(masks)
        bits, colours = rh.to_host(_pack_bits(mask_cat), torch.cat(smalls)[mask_cat.bool()])
        del keep
        mask_flat = np.unpackbits(bits, bitorder="little")[:len(mask_cat)].astype(bool)
        img_flat = np.zeros((len(mask_flat), 3), np.uint8)
        img_flat[mask_flat] = colours
        # host: what slic_masked computes on the small image before its sweeps
        o, prep = 0, []
        for nh, nw, n_seg in sizes:
            prep.append((img_flat[o:o + nh * nw].reshape(nh, nw, 3), mask_flat[o:o + nh * nw].reshape(nh, nw)))
            o += nh * nw
        px_off, seg_off, tab, steps, imgs, segs = 0, 0, [], [], [], []
        for (masked, mask), (nh, nw, n_seg) in zip(prep, sizes):
            lab = _rgb2lab(masked)
            centroids, st = _mask_centroids(mask, n_seg)
            lab = ndi.gaussian_filter(lab[None], [1.0, 1.0, 1.0, 0], mode="reflect")[0]
            K = len(centroids)
            segs.append(np.concatenate([centroids, np.zeros((K, 3))], axis=-1))
            steps.append(float(max(st)))
            imgs.append(np.ascontiguousarray(lab * (1.0 / _COMPACTNESS)).reshape(-1, 3))
            tab.append((px_off, nh, nw, K, seg_off))
            px_off += (nh * nw + 255) // 256 * 256
            seg_off += K
        img_all = np.zeros((px_off, 3))
        mask_all = np.zeros(px_off, np.uint8)
        for (o, nh, nw, K, so), im, (_, mask) in zip(tab, imgs, prep):
            img_all[o:o + nh * nw] = im
            mask_all[o:o + nh * nw] = mask.reshape(-1)
        tab = np.array(tab, np.int32)
        item, first = _block_tables(tab[:, 1].astype(np.int64) * tab[:, 2])
        seg_region = np.repeat(np.arange(len(tab), dtype=np.int32), tab[:, 3])
        wb = int(rh.lib.rhccq_slic_regions_work_bytes(len(tab), _SLIC_SWEEPS))
        d = [rh.dev(a) for a in (img_all, mask_all, np.concatenate(segs), tab, np.array(steps), item, first, seg_region)]
        work = rh.empty((wb,), torch.uint8)
        labels = rh.zeros((px_off,), torch.int32)
        rh._check(rh.lib.rhccq_slic_sweeps_regions(rh.ctx, rh._p(d[0]), rh._p(d[1]), rh._p(d[2]), rh._p(d[3]), rh._p(d[4]), len(tab),
                                                   int(tab[:, 3].max()), rh._p(d[5]), rh._p(d[6]), len(item), rh._p(d[7]), len(seg_region),
                                                   _SLIC_SWEEPS, rh._p(work), wb, rh._p(labels)), "slic_sweeps_regions")
        # the labels of the in-mask pixels only (every other one is 0), in the narrowest type that holds K
        narrow = torch.uint8 if int(tab[:, 3].max()) < 256 else torch.int16
        lab_all = np.zeros(px_off, np.int32)
        lab_all[mask_all != 0] = rh.to_host(labels[d[1].bool()].to(narrow))
        out = []
        for (o, nh, nw, K, so), (_, mask) in zip(tab, prep):
            lab = np.ascontiguousarray(lab_all[o:o + nh * nw].reshape(nh, nw))
            seg_size = mask.sum() / K
            conn = np.empty((nh, nw), np.int32)
            rc = rh._raw.rhccq_slic_connectivity_host(C.c_void_p(lab.ctypes.data), int(nh), int(nw), int(0.5 * seg_size), int(3 * seg_size),
                                                      C.c_void_p(conn.ctypes.data))
            if rc:
                raise ValueError("slic connectivity: bad arguments")
            out.append(conn)
        return out

    # ---- stage 4 ---------------------------------------------------------------------------------------------------------------
    def layers(self, maps, regions, small_labels, qualities):
        """subregion_quantization's label layers of both calls -> ([(call, ClassSpec)], per region (class index or -1, local index),
        per call {segments, segments_dropped, layers})"""
        rh = self.rh
        H, W = int(maps[0].shape[0]), int(maps[0].shape[1])
        R = len(regions)
        if R == 0:
            return [], [], [{"segments": 0, "segments_dropped": 0, "layers": 0} for _ in range(2)]
        nsid = np.array([int(s.max(initial=0)) + 1 for s in small_labels], np.int64)
        sid_off = np.concatenate([[0], np.cumsum(nsid)[:-1]]).astype(np.int64)
        sm_off = np.concatenate([[0], np.cumsum([s.size for s in small_labels])[:-1]]).astype(np.int64)
        yx, yx_off = [], 0
        tab = np.zeros((R, 11), np.int32)
        for i, (r, s) in enumerate(zip(regions, small_labels)):
            h, w = r.hw
            yx += [self._nearest_tables(s.shape[0], h), self._nearest_tables(s.shape[1], w)]
            tab[i] = (r.bbox[0], r.bbox[1], h, w, r.map, r.label, sm_off[i], s.shape[1], yx_off, sid_off[i], -1)
            yx_off += h + w
        area = tab[:, 2].astype(np.int64) * tab[:, 3]
        item, first = _block_tables(area)
        d_small = rh.dev(np.concatenate([s.reshape(-1) for s in small_labels]).astype(np.int32))
        d_yx, d_item, d_first = rh.dev(np.concatenate(yx)), rh.dev(item), rh.dev(first)
        d_tab = rh.dev(tab)
        n_sid = int(nsid.sum())
        counts = rh.empty((n_sid,), torch.int32)
        rh._check(rh.lib.rhccq_image_seg_counts(rh.ctx, rh._p(maps[0]), rh._p(maps[1]), H, W, rh._p(d_tab), rh._p(d_small), rh._p(d_yx), rh._p(d_item),
                                                rh._p(d_first), len(item), rh._p(counts), n_sid), "image_seg_counts")
        cnt = rh.to_host(counts)
        # the kept segments of every region in subregion_quantization's order (ascending ids, find_contours' drop rule)
        keep = np.zeros(n_sid, np.int32)
        kept = []
        stats = [{"segments": 0, "segments_dropped": 0, "layers": 0} for _ in range(2)]
        for i, r in enumerate(regions):
            h, w = r.hw
            c = cnt[sid_off[i]:sid_off[i] + nsid[i]]
            ids = [s for s in range(1, int(nsid[i])) if c[s] > 0]
            drop = [s for s in ids if h >= 2 and w >= 2 and c[s] == h * w]
            stats[r.call]["segments_dropped"] += len(drop)
            ks = [s for s in ids if s not in drop]
            stats[r.call]["segments"] += len(ks)
            keep[sid_off[i] + np.array(ks, np.int64)] = 1
            kept.append(ks)
        # overlaps: only regions of different label maps can share pixels (the small ROI regions at the end of the non-ROI list)
        pairs = overlap_candidates(regions, [bool(k) for k in kept])
        hit = {}
        if pairs:
            pr = np.array(pairs, np.int32)
            ia = np.maximum(tab[pr[:, 0], 0], tab[pr[:, 1], 0]), np.minimum(tab[pr[:, 0], 0] + tab[pr[:, 0], 2], tab[pr[:, 1], 0] + tab[pr[:, 1], 2])
            ib = np.maximum(tab[pr[:, 0], 1], tab[pr[:, 1], 1]), np.minimum(tab[pr[:, 0], 1] + tab[pr[:, 0], 3], tab[pr[:, 1], 1] + tab[pr[:, 1], 3])
            p_item, p_first = _block_tables((ia[1] - ia[0]).astype(np.int64) * (ib[1] - ib[0]))
            d_hit = rh.empty((len(pairs),), torch.int32)
            d_keep, d_pr, d_pi, d_pf = rh.dev(keep), rh.dev(pr), rh.dev(p_item), rh.dev(p_first)
            rh._check(rh.lib.rhccq_image_overlap(rh.ctx, rh._p(maps[0]), rh._p(maps[1]), H, W, rh._p(d_tab), rh._p(d_small), rh._p(d_yx), rh._p(d_keep),
                                                 rh._p(d_pr), len(pairs), rh._p(d_pi), rh._p(d_pf), len(p_item), rh._p(d_hit)), "image_overlap")
            hit = {p: bool(v) for p, v in zip(pairs, rh.to_host(d_hit))}
        ids = np.zeros(n_sid, np.int32)
        layers, place = place_layers(regions, kept, hit)
        specs = []
        for call, l in layers:
            stats[call]["layers"] += 1
            for n, (i, s) in enumerate(l["segments"], 1):      # ids per layer: regions in list order, SLIC ids ascending
                ids[sid_off[i] + s] = n
            for i in l["members"]:
                tab[i, 10] = len(specs)
            specs.append((call, l))
        d_layers = rh.zeros((max(len(specs), 1), H, W), torch.int32)
        if specs:
            d_tab2, d_ids = rh.dev(tab), rh.dev(ids)
            rh._check(rh.lib.rhccq_image_paint(rh.ctx, rh._p(maps[0]), rh._p(maps[1]), H, W, rh._p(d_tab2), rh._p(d_small), rh._p(d_yx), rh._p(d_ids),
                                               rh._p(d_item), rh._p(d_first), len(item), rh._p(d_layers)), "image_paint")
        classes = [(call, ClassSpec(d_layers[k], l["seg_region"], l["bboxes"], qualities[call])) for k, (call, l) in enumerate(specs)]
        return classes, place, stats

    # ---- report ----------------------------------------------------------------------------------------------------------------
    def quality(self, rgb, res, region_map, names=("nonroi", "roi")):
        """per-class quality of a result against the uploaded image: the error sums straight from palette[indices] (the decoded
        picture is never written for them), a device-side decode for the SSIM windows; only the len(names) x 6 sums and the SSIM
        partials come back.  A result smaller than the image (top_left / shape) is compared on its own rectangle."""
        from .api.comparison import region_metrics_from_sums
        rh = self.rh
        (top, left), (h, w) = res["top_left"], res["shape"]
        if (top, left, h, w) != (0, 0, int(rgb.shape[0]), int(rgb.shape[1])):
            rgb = rgb[top:top + h, left:left + w].contiguous()
            region_map = region_map[top:top + h, left:left + w].contiguous()
        pal = rh.dev(np.asarray(res["palette"], np.uint8).reshape(-1, 3))
        idx = res["indices"].reshape(-1)
        sums = rh.class_error_sums_indexed(rgb, idx, pal, region_map, len(names))
        recon = rh.decode(idx, pal).reshape(h, w, 3)
        return region_metrics_from_sums(sums, rh.class_ssim7(rgb, recon, region_map, len(names)), names)

    # ---- the whole flow --------------------------------------------------------------------------------------------------------
    def encode(self, image, roi_quality=20, nonroi_quality=10, out_path=None, exact=False, roi_mask=None, report=False, max_colours=None,
               target_bytes=None, target_psnr=None, run_slack=None, run_penalty=None, dither=None, pattern=None, pattern_size=4, png_path=None, gif_path=None):
        """image: uint8[H,W,3] (numpy or device tensor) -> the FrameEncoder result dict (palette, indices device tensor,
        indices_dtype, shape, top_left) equal to script_flow(image, roi_quality, nonroi_quality)'s `final`, plus `classes`
        ([(call, ClassSpec)], the label layers subregion_quantization builds) and `stats`.  out_path: the file is written through
        container.write_frame(exact=exact).
        roi_mask: a caller's ROI mask (bool / uint8 [H,W], numpy or device tensor) instead of the detector: stats["roi_source"] =
        "caller".  report: stats["quality"] = PSNR / SSIM / ... of the result inside ("roi"), outside ("nonroi") the region map and
        over the picture ("all") (api.comparison.region_metrics_from_sums), computed on the device from the indices.
        max_colours = N (EXTENSION, default None = off): a finished result of more than N palette rows is reduced to N by
        Rhccq.palette_reduce (exact pairwise merging, weights = the histogram of the result's own index map), and the pixels of the
        rectangle the result covers are remapped onto the reduced palette (Rhccq.palette_remap); stats["reduce"] = {from, to, empty,
        steps}.  The file and the report are those of the reduced result.
        target_bytes = B or target_psnr = P (EXTENSION; exclusive with each other and with max_colours): the finished result's
        palette is searched for the rung that meets the target, as encode_with_palette(window, palette, target_...=) searches it,
        over the rectangle the result covers, with the region map as the mask of a {"roi", "nonroi"} PSNR target and refine = 0.
        This differs from max_colours: the weights of the merge chain come from the nearest-row assignment of the pixels, not from
        the result's own index map, because the error bound needs the moments of that assignment; the result's indices become the
        nearest rows of the rung (also at the top rung, where nothing merges).  stats["target"] and stats["reduce"] as
        encode_with_palette fills them.  The palette may have at most ops.palette_reduce_max_rows() rows (RhccqError).
        run_slack = s or {"roi": a, "nonroi": b} (EXTENSION, default None = off; 0 is a value): the finished result's index map (after
        max_colours, if given) is rewritten by the run-carrying rule over its own palette and the rectangle it covers
        (Rhccq.palette_runs: a pixel keeps its left neighbour's index while that costs at most the slack more squared error than its
        nearest row), the dict's entries applying inside and outside the region map; stats["runs"] as encode_with_palette fills it.
        With a target every probe and the result run with the slack, as in encode_with_palette.
        run_penalty = p or {"roi": a, "nonroi": b} (EXTENSION, default None = off; 0 is a value; exclusive with run_slack and with
        target_psnr): the same place and the same rules, with the exact row segmentation (Rhccq.palette_segment) instead of the
        greedy rule; stats["runs"] as encode_with_palette fills it.
        dither = s or {"roi": a, "nonroi": b} (EXTENSION, default None = off; 0 is a value; exclusive with run_slack, run_penalty and
        target_psnr): the same place and the same rules, with error diffusion (Rhccq.palette_dither) over the result's own palette;
        stats["dither"] as encode_with_palette fills it, and no stats["runs"].
        pattern = s or {"roi": a, "nonroi": b}, pattern_size = 2, 4 or 8 (EXTENSION, default None = off; 0 is a value; exclusive with
        run_slack, run_penalty, dither and target_psnr): the same place and the same rules, with the position-only pattern dither
        (Rhccq.palette_pattern) over the result's own palette; stats["pattern"] as encode_with_palette fills it, and no stats["runs"].
        png_path (EXTENSION, default None = off): as encode_with_palette takes it, for the rectangle the result covers.
        gif_path (EXTENSION, default None = off): as encode_with_palette takes it (ValueError above 256 rows: max_colours or a target bring
        a result below)."""
        rh = self.rh
        png_path = self._png_arg("ImageEncoder.encode", png_path)
        gif_path = self._png_arg("ImageEncoder.encode", gif_path, "gif_path")
        searching = target_bytes is not None or target_psnr is not None
        if searching and max_colours is not None:
            raise ValueError("ImageEncoder.encode: target_bytes / target_psnr and max_colours are exclusive")
        runs = self._runs_args("ImageEncoder.encode", run_slack, run_penalty, True, target_psnr, dither=dither, pattern=pattern,
                               pattern_size=pattern_size)
        cons = self._target_args("ImageEncoder.encode", target_bytes, target_psnr, True) if searching else None
        image, png_in = self._png_in(image)
        if torch.is_tensor(image):
            image = image.cpu().numpy()                          # (the ROI chain's edge search reads a host image)
        image = np.ascontiguousarray(image, dtype=np.uint8)
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("ImageEncoder.encode: a uint8 H x W x 3 image is expected")
        H, W = image.shape[:2]
        t, t0 = {}, time.perf_counter()

        def lap(name):
            nonlocal t0
            now = time.perf_counter()
            t[name] = now - t0
            t0 = now
        regions, maps, rgb, stats = self.regions(image, roi_mask)
        region_map = self.region_map
        lap("regions")
        n_seg = self.split_segments(rgb, maps, regions)
        lap("split_score")
        small = self.slic(image, rgb, maps, regions, n_seg)
        lap("slic")
        classes, place, seg_stats = self.layers(maps, regions, small, (roi_quality, nonroi_quality))
        lap("layers")
        stats.update(roi_segments=seg_stats[0]["segments"], nonroi_segments=seg_stats[1]["segments"],
                     segments_dropped=seg_stats[0]["segments_dropped"] + seg_stats[1]["segments_dropped"],
                     roi_layers=seg_stats[0]["layers"], nonroi_layers=seg_stats[1]["layers"])
        if not classes:
            raise IndexError("no segments in either class")       # quantize_image([]): merged[0] of an empty list
        enc = FrameEncoder(rh)
        S = enc.prepare(rgb, [c for _, c in classes])
        per_class = enc.level1(S)
        lap("level1")
        groups = [(q, [place[i] for i, r in enumerate(regions) if r.call == call and place[i][0] >= 0])
                  for call, q in ((0, roi_quality), (1, nonroi_quality))]
        lvl2, q2s, jobs2 = enc.level2_jobs(S, per_class, groups)
        comps3 = enc.level2_finish(lvl2, cluster_palettes(rh, jobs2))
        m3c, q3, job3 = enc.level3_job(S, comps3, q2s)
        (res3,) = cluster_palettes(rh, [job3])
        res = enc.finish(S, comps3, m3c, q3, res3)
        torch.cuda.current_stream(rh.device).synchronize()
        lap("levels23")
        if max_colours is not None and len(res["palette"]) > int(max_colours):
            stats["reduce"] = self._reduce_result(rgb, res, int(max_colours))
            lap("reduce")
        data = None
        if searching:
            stats["reduce"], stats["target"], data, row = self._target_result(rgb, res, region_map, target_bytes, cons, exact, runs)
            if row is not None:
                stats[self._runs_key(runs)] = row
            lap("target")
        elif runs is not None:
            stats[self._runs_key(runs)] = self._runs_result(rgb, res, region_map, runs)
            lap(self._runs_key(runs))
        if out_path:
            from . import container
            if data is not None:                                                  # the probe's bytes are the file
                with open(out_path, "wb") as f:
                    f.write(data)
            else:
                container.write_frame(res, out_path, rh, exact=exact)
            lap("container")
        if png_path:
            stats["png"] = self._png_write(res, png_path, exact)
            lap("png")
        if gif_path:
            stats["gif"] = self._gif_write(res, gif_path)
            lap("gif")
        if report:
            stats["quality"] = self.quality(rgb, res, region_map)
            lap("report")
        stats["seconds"] = {k: round(v, 4) for k, v in t.items()}
        if png_in is not None:
            stats["png_in"] = png_in
        res["classes"] = classes
        res["stats"] = stats
        return res

    # ---- a PNG file as the image (EXTENSION: csrc/png_read.hip) -----------------------------------------------------------------
    def _png_in(self, image):
        """image as encode, encode_with_palette and quantize take it -> (the image, stats["png_in"] or None): a file name is read on the
        device (container.read_png); the file's alpha, if any, is ignored and reported"""
        if not isinstance(image, (str, os.PathLike)):
            return image, None
        from . import container
        fr = container.read_png(os.fspath(image), self.rh)
        info = fr["info"]
        return fr["image"], {"shape": list(fr["shape"]), "colour_type": info["colour_type"], "depth": info["depth"], "alpha_ignored": fr["alpha"] is not None,
                             "chunks": info["chunks"], "idat_chunks": info["idat_chunks"]}

    # ---- the result as a PNG file (EXTENSION: csrc/png_write.hip) ---------------------------------------------------------------
    @staticmethod
    def _png_arg(fn, png_path, what="png_path"):
        """png_path (or gif_path) as given -> a file name or None"""
        if png_path is None:
            return None
        if not isinstance(png_path, (str, os.PathLike)):
            raise TypeError(f"{fn}: {what} must be a file name, got {type(png_path).__name__}")
        if not os.fspath(png_path):
            raise ValueError(f"{fn}: {what} must not be empty")
        return os.fspath(png_path)

    def _png_write(self, res, png_path, exact):
        from . import container
        data, row = container.png_file(res, self.rh, exact=exact)
        with open(png_path, "wb") as f:
            f.write(data)
        return row

    # ---- results as a GIF file (EXTENSION: csrc/gif_write.hip) ------------------------------------------------------------------
    def _gif_write(self, results, gif_path, delay=4, loop=0, delta=False):
        """container.gif_file written to gif_path -> its row for stats["gif"]"""
        from . import container
        data, row = container.gif_file(results, self.rh, delay=delay, loop=loop, delta=delta)
        with open(gif_path, "wb") as f:
            f.write(data)
        return row

    # ---- a given palette (EXTENSION, no reference counterpart) ------------------------------------------------------------------
    def _reduce(self, pal, counts, colours):
        """Rhccq.palette_reduce and its stats row -> (palette device uint8[k_out, 3], {from, to, empty, steps})"""
        if colours < 1:
            raise ValueError("ImageEncoder: the number of colours to reduce to must be >= 1")
        K = int(pal.shape[0])
        new_pal, _, _, merges = self.rh.palette_reduce(pal, counts, min(colours, K))
        k, steps = int(new_pal.shape[0]), int(merges.shape[0])
        return new_pal.contiguous(), {"from": K, "to": k, "empty": K - k - steps, "steps": steps}

    def _reduce_result(self, rgb, res, colours):
        """encode's max_colours: the finished result in place -> its stats row"""
        from .container import index_histogram
        rh = self.rh
        (top, left), (h, w) = res["top_left"], res["shape"]
        pal = rh.dev(np.asarray(res["palette"], np.uint8).reshape(-1, 3))
        new_pal, row = self._reduce(pal, index_histogram(res["indices"], int(pal.shape[0]), rh), colours)
        window = rgb if (top, left, h, w) == (0, 0, int(rgb.shape[0]), int(rgb.shape[1])) else rgb[top:top + h, left:left + w].contiguous()
        idx, _ = rh.palette_remap(window, new_pal)
        res.update(palette=rh.to_host(new_pal), indices=idx.reshape(res["indices"].shape),                 # (the layout the result had)
                   indices_dtype="uint8" if idx.dtype == torch.uint8 else "uint16")
        return row

    def _window(self, rgb, res, region_map):
        """the pixels and the region map of the rectangle a finished result covers -> (window, class map uint8)"""
        (top, left), (h, w) = res["top_left"], res["shape"]
        whole = (top, left, h, w) == (0, 0, int(rgb.shape[0]), int(rgb.shape[1]))
        window = rgb if whole else rgb[top:top + h, left:left + w].contiguous()
        cls = (region_map if whole else region_map[top:top + h, left:left + w]).contiguous()
        if cls.dtype == torch.bool:
            cls = cls.view(torch.uint8)
        return window, cls

    def _target_result(self, rgb, res, region_map, target_bytes, cons, exact, runs=None):
        """encode's target_bytes / target_psnr: the finished result in place -> (stats["reduce"], stats["target"], the file's bytes or None,
        stats["runs"] or None)"""
        rh = self.rh
        pal = rh.dev(np.asarray(res["palette"], np.uint8).reshape(-1, 3))
        window, cls = self._window(rgb, res, region_map)
        new_pal, idx, _, _, _, runs_row, row, target, data = self._search(window, pal, cls, 1, 0, None, target_bytes, cons, exact, runs)
        res.update(palette=rh.to_host(new_pal), indices=idx.reshape(res["indices"].shape),                 # (the layout the result had)
                   indices_dtype="uint8" if idx.dtype == torch.uint8 else "uint16")
        return row, target, data, runs_row

    def _runs_result(self, rgb, res, region_map, runs):
        """encode's run_slack / run_penalty / dither / pattern without a target: the finished result's index map in place -> its stats row"""
        rh = self.rh
        pal = rh.dev(np.asarray(res["palette"], np.uint8).reshape(-1, 3))
        window, cls = self._window(rgb, res, region_map)
        idx, sums, status = self._runs_call(window, pal, cls, runs)
        res.update(indices=idx.reshape(res["indices"].shape), indices_dtype="uint8" if idx.dtype == torch.uint8 else "uint16")
        return self._runs_row(runs, self._runs_host(sums, status)[0], True)

    # ---- the run-carrying remap (EXTENSION, no reference counterpart) ------------------------------------------------------------------
    @staticmethod
    def _run_arg(fn, name, key, most, value, masked):
        """the keyword `name` (run_slack, run_penalty, dither, pattern) checked -> None (off), or {key: as given, "nonroi": v, "roi": v}, each v in 0..most"""
        if value is None:
            return None
        if isinstance(value, dict):
            if sorted(value) != ["nonroi", "roi"]:
                raise ValueError(f'{fn}: {name} is a number or a dict over "roi" and "nonroi"')
            if not masked:
                raise ValueError(f"{fn}: a roi / nonroi {name} needs roi_mask")
            given = {k: int(v) for k, v in value.items()}
            out = {key: given, "nonroi": given["nonroi"], "roi": given["roi"]}
        else:
            out = {key: int(value), "nonroi": int(value), "roi": int(value)}
        if not (0 <= out["nonroi"] <= most and 0 <= out["roi"] <= most):
            raise ValueError(f"{fn}: a {name} must be 0..{most}")
        return out

    @staticmethod
    def _runs_args(fn, run_slack, run_penalty, masked, target_psnr=None, *, dither=None, pattern=None, pattern_size=4):
        """run_slack, run_penalty, dither and pattern checked together -> None (all off) or the dict of the one given (it has "slack",
        "penalty", "dither" or "pattern"; the last also "size")"""
        if pattern is not None:
            if run_slack is not None or run_penalty is not None:
                raise ValueError(f"{fn}: pattern is exclusive with run_slack and run_penalty")
            if dither is not None:
                raise ValueError(f"{fn}: pattern and dither are exclusive")
            if target_psnr is not None:
                # as for dither: the ladder's bound is that of the nearest-row map
                raise ValueError(f"{fn}: pattern cannot be combined with target_psnr")
            if isinstance(pattern_size, bool) or pattern_size not in ops.PATTERN_SIZES:
                raise ValueError(f"{fn}: pattern_size must be 2, 4 or 8")
            out = ImageEncoder._run_arg(fn, "pattern", "pattern", ops.PATTERN_MAX, pattern, masked)
            out["size"] = int(pattern_size)
            return out
        if dither is not None:
            if run_slack is not None or run_penalty is not None:
                raise ValueError(f"{fn}: dither is exclusive with run_slack and run_penalty")
            if target_psnr is not None:
                # the ladder's bound is that of the nearest-row map; a dithered pixel may be any distance from its nearest row
                raise ValueError(f"{fn}: dither cannot be combined with target_psnr")
            return ImageEncoder._run_arg(fn, "dither", "dither", ops.DITHER_MAX, dither, masked)
        if run_slack is not None and run_penalty is not None:
            raise ValueError(f"{fn}: run_slack and run_penalty are exclusive")
        if run_penalty is not None and target_psnr is not None:
            # the only bound the segmentation gives a pixel is its two boundaries' penalties: too loose to choose a rung by
            raise ValueError(f"{fn}: run_penalty cannot be combined with target_psnr")
        if run_penalty is not None:
            return ImageEncoder._run_arg(fn, "run_penalty", "penalty", ops.RUN_PENALTY_MAX, run_penalty, masked)
        return ImageEncoder._run_arg(fn, "run_slack", "slack", ops.RUN_SLACK_MAX, run_slack, masked)

    def _runs_call(self, rgb, pal, cls, runs):
        """the final index map by the rule `runs` names: the greedy carry (Rhccq.palette_runs), the exact row segmentation
        (Rhccq.palette_segment), error diffusion (Rhccq.palette_dither) or the pattern dither (Rhccq.palette_pattern) -> (indices, sums
        device, the status word device or None: the caller reads both back through _runs_host)"""
        table, nc = self._slack_table(runs, cls is not None), 2 if cls is not None else 0
        if "pattern" in runs:
            return self.rh.palette_pattern(rgb, pal, table, runs["size"], cls, nc) + (None,)
        if "dither" in runs:
            return self.rh.palette_dither(rgb, pal, table, cls, nc, with_status=True)
        if "penalty" in runs:
            return self.rh.palette_segment(rgb, pal, table, cls, nc) + (None,)
        return self.rh.palette_runs(rgb, pal, table, cls, nc) + (None,)

    def _runs_host(self, sums, status, *more):
        """one read-back of a _runs_call's sums, its status word (checked) and whatever else the caller wants with them"""
        if status is None:
            got = self.rh.to_host(sums, *more)
            return got if more else (got,)
        got = self.rh.to_host(sums, *more, status)
        self.rh.check_dither(got[-1])
        return got[:-1]

    @staticmethod
    def _runs_key(runs):
        """the entry of stats a rule's row goes to"""
        return "dither" if "dither" in runs else "pattern" if "pattern" in runs else "runs"

    @staticmethod
    def _unbounded(runs):
        """the rules whose pixels may be any distance from their nearest row: the ladder's curve bounds nothing for them"""
        return runs is not None and ("dither" in runs or "pattern" in runs)

    @staticmethod
    def _slack_table(runs, masked):
        """Rhccq.palette_runs' table over the region map's classes (0 = outside, 1 = inside; a map holds no other value)"""
        return [runs["nonroi"], runs["roi"], min(runs["nonroi"], runs["roi"])] if masked else [runs["nonroi"]]

    @staticmethod
    def _runs_row(runs, sums, masked):
        carried = {"all": int(sums[-1][2])}
        if masked:
            carried["roi"], carried["nonroi"] = int(sums[1][2]), int(sums[0][2])
        if "dither" in runs:
            return {"strength": runs["dither"], "moved": carried, "pixels": int(sums[-1][0])}
        if "pattern" in runs:
            return {"strength": runs["pattern"], "size": runs["size"], "moved": carried, "pixels": int(sums[-1][0])}
        if "penalty" in runs:
            breaks = {"all": int(sums[-1][3])}
            if masked:
                breaks["roi"], breaks["nonroi"] = int(sums[1][3]), int(sums[0][3])
            return {"penalty": runs["penalty"], "carried": carried, "breaks": breaks, "pixels": int(sums[-1][0])}
        return {"slack": runs["slack"], "carried": carried, "pixels": int(sums[-1][0])}

    @staticmethod
    def _remap_row(pixels, sse):
        pixels, sse = int(pixels), int(sse)
        return {"pixels": pixels, "sse": sse, "mse": sse / (3.0 * pixels) if pixels else None,
                "psnr": psnr_from_sse(sse, pixels) if pixels else None}

    def _finish_palette(self, rgb, pal, cls, roi_weight, refine, runs=None):
        """the refinement, if asked for, and the final remap (by the rule `runs` names, if any) -> (palette device, indices, sums host
        {pixels, sse} per row, history host or None, iterations, the rule's stats row or None)"""
        rh = self.rh
        hist = nit = None
        if refine:
            pal, hist, nit = rh.palette_refine(rgb, pal, cls, [1, roi_weight, 1] if cls is not None else None, max_iter=refine)
        status = None
        if runs is not None:
            idx, sums, status = self._runs_call(rgb, pal, cls, runs)
        else:
            idx, sums = rh.palette_remap(rgb, pal, cls, 2 if cls is not None else 0)
        if refine:
            sums, hist, nit = self._runs_host(sums, status, hist, nit)        # one read for all
            nit = int(nit[0])
        else:
            (sums,) = self._runs_host(sums, status)
        runs_row = None
        if runs is not None:
            runs_row = self._runs_row(runs, sums, cls is not None)
            sums = sums[:, :2]
        return pal, idx, sums, hist, nit, runs_row

    # ---- the ladder of a given palette and the targets on it (EXTENSION, no reference counterpart) -------------------------------------
    _TABLES = ("nonroi", "roi", "all")                                         # the moment tables of a masked picture, in order

    @staticmethod
    def _target_args(fn, target_bytes, target_psnr, masked):
        """the two target keywords checked -> None for a byte target, {table: dB} for a PSNR target"""
        if target_bytes is not None and target_psnr is not None:
            raise ValueError(f"{fn}: target_bytes and target_psnr are exclusive")
        if target_bytes is not None:
            if int(target_bytes) < 1:
                raise ValueError(f"{fn}: target_bytes must be >= 1")
            return None
        cons = dict(target_psnr) if isinstance(target_psnr, dict) else {"all": target_psnr}
        if not cons or any(k not in ImageEncoder._TABLES for k in cons):
            raise ValueError(f'{fn}: target_psnr is a number or a dict over "all", "roi", "nonroi"')
        if not masked and any(k != "all" for k in cons):
            raise ValueError(f'{fn}: a "roi" or "nonroi" target needs roi_mask')
        return {k: float(v) for k, v in cons.items()}

    def _ladder(self, rgb, pal, cls, roi_weight):
        rh = self.rh
        first, mom = rh.palette_moments(rgb, pal, cls, 2 if cls is not None else 0)
        N = mom[:, :, 0]
        counts = (N[-1] if cls is None or roi_weight == 1 else N[-1] + (roi_weight - 1) * N[1]).contiguous()
        _, _, _, merges = rh.palette_reduce(pal, counts, 1)
        curve = rh.palette_curve(pal, counts, merges, mom)
        live = int(merges.shape[0]) + 1
        names = ("all",) if cls is None else self._TABLES
        host, merges_host = rh.to_host(torch.cat([curve[:, :live].reshape(-1), N.sum(dim=1)]), merges)      # the one read-back of the curve and the log
        sse = {n: [int(v) for v in host[t * live:(t + 1) * live]] for t, n in enumerate(names)}
        pixels = {n: int(host[len(names) * live + t]) for t, n in enumerate(names)}
        bound = {n: [psnr_from_sse(v, pixels[n]) if pixels[n] else None for v in sse[n]] for n in names}
        return {"colours": [live - s for s in range(live)], "sse": sse, "psnr_bound": bound, "pixels": pixels, "merges": merges_host,
                "state": {"palette": pal, "counts": counts, "merges": merges, "moments": mom, "indices": first, "class_map": cls}}

    def ladder(self, image, palette, roi_mask=None, roi_weight=1):
        """the rate-distortion ladder of a palette over an image, without a single encode: image uint8[H,W,3], palette uint8[K,3]
        (or a dict with "palette"), roi_mask and roi_weight as encode_with_palette takes them -> {"colours": [k of step s: rows in
        use, ..., 1], "sse": {"all": [...]} and "psnr_bound": {"all": [...]} per step (with a mask also "roi" and "nonroi"),
        "pixels": {table: pixels}, "merges": int32[steps, 2], "state": the device tensors a search reuses}.
        One moments pass (Rhccq.palette_moments: nearest-row index map, histogram and per-row moments), the counts
        sum over classes of weight x N with weights [1, roi_weight, 1] (those colours= computes), one merge chain to a single row
        with its log (Rhccq.palette_reduce), and Rhccq.palette_curve.  sse[s] is the exact squared error of the image shown through
        the clusters after s merges; the nearest-row remap onto that rung (what colours=k encodes) can only be better, so
        psnr_bound[s] is a lower bound of colours=k's PSNR for k = colours[s], refine = 0.  The host waits for the device twice:
        Rhccq.palette_reduce reads its row count (8 bytes), and one read-back fetches the curve, the pixel counts and the log
        together.  K may be at most ops.palette_reduce_max_rows() (RhccqError)."""
        rh = self.rh
        roi_weight = int(roi_weight)
        if not 1 <= roi_weight <= 255 or (roi_weight != 1 and roi_mask is None):
            raise ValueError("ImageEncoder.ladder: roi_weight (1..255) other than 1 needs roi_mask")
        if isinstance(palette, dict):
            palette = palette["palette"]
        pal = palette.to(rh.device) if torch.is_tensor(palette) else rh.dev(np.asarray(palette))
        if pal.dtype != torch.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
            raise ValueError("ImageEncoder.ladder: a uint8 K x 3 palette, K >= 1, is expected")
        rgb = image.to(rh.device).contiguous() if torch.is_tensor(image) else rh.dev(np.asarray(image))
        if rgb.dtype != torch.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("ImageEncoder.ladder: a uint8 H x W x 3 image is expected")
        cls = None
        if roi_mask is not None:
            from .api.roi import region_map_from_mask
            cls = region_map_from_mask(rgb, roi_mask, rh)
        return self._ladder(rgb, pal.contiguous(), cls, roi_weight)

    def _search(self, rgb, pal, cls, roi_weight, refine, colours, target_bytes, cons, exact, runs=None):
        """the target search of encode_with_palette on the ladder of `pal` -> (palette device, indices, sums host, history, iterations,
        stats["runs"] or None, stats["reduce"], stats["target"], the file's bytes or None)"""
        from . import container
        rh = self.rh
        if colours is not None and int(colours) < 1:
            raise ValueError("ImageEncoder: the number of colours to reduce to must be >= 1")
        L = self._ladder(rgb, pal, cls, roi_weight)
        st = L["state"]
        K, live = int(pal.shape[0]), len(L["colours"])
        k0 = min(int(colours) if colours is not None else K, live)
        names = ("all",) if cls is None else self._TABLES
        table_row = {"all": -1, "nonroi": 0, "roi": 1}

        def rung(k):
            return rh.palette_rung(pal, st["counts"], st["merges"], k)[0].contiguous()

        # with a run slack a pixel may lose at most its slack against the nearest row: the curve's sum plus slack x pixels per table
        # bounds the run-carrying result's squared error (exact integers).  With a run penalty a pixel may lose the penalties of its two
        # boundaries, its own and its right neighbour's (of either class): own + largest per pixel (a byte target records this bound)
        extra = None
        if runs is not None and not self._unbounded(runs):
            px = L["pixels"]
            per = {n: runs[n] + (max(runs["nonroi"], runs["roi"]) if "penalty" in runs else 0) for n in ("nonroi", "roi")}
            extra = {"all": per["nonroi"] * px["all"]} if cls is None else {"nonroi": per["nonroi"] * px["nonroi"], "roi": per["roi"] * px["roi"]}
            if cls is not None:
                extra["all"] = extra["nonroi"] + extra["roi"]

        def bound(k):
            if self._unbounded(runs):                                                # the curve bounds the nearest-row map only
                return {n: None for n in names}
            if extra is None:
                return {n: L["psnr_bound"][n][live - k] for n in names}
            return {n: (psnr_from_sse(L["sse"][n][live - k] + extra[n], L["pixels"][n]) if L["pixels"][n] else None) for n in names}

        def misses(figures):
            """the constraints a {table: PSNR or None} misses"""
            return {n for n, want in cons.items() if figures[n] is not None and not figures[n] >= want}

        def achieved(sums):
            return {n: (psnr_from_sse(int(sums[table_row[n]][1]), int(sums[table_row[n]][0])) if int(sums[table_row[n]][0]) else None) for n in names}

        if target_bytes is None:
            k = next((k for k in range(1, k0 + 1) if not misses(bound(k))), k0)
            out = self._finish_palette(rgb, rung(k), cls, roi_weight, refine, runs)
            dropped = False
            if refine:
                lost = misses(achieved(out[2]))
                if lost:
                    plain = self._finish_palette(rgb, rung(k), cls, roi_weight, 0, runs)
                    if lost - misses(achieved(plain[2])):                        # the unrefined rung meets one of them
                        out, dropped = plain, True
            target = {"kind": "psnr", "target": dict(cons), "met": not misses(achieved(out[2])), "colours": k, "probes": [], "bound_psnr": bound(k),
                      "refine_dropped": dropped}
            data = None
        else:
            B, probes, fits, first = int(target_bytes), [], None, None

            def probe(k):
                nonlocal fits, first
                out = self._finish_palette(rgb, rung(k), cls, roi_weight, refine, runs)
                res = {"palette": rh.to_host(out[0]), "indices": out[1], "shape": (int(rgb.shape[0]), int(rgb.shape[1]))}
                data = container.frame_bytes(res, rh, exact=exact)
                probes.append((k, len(data)))
                if len(data) <= B:
                    fits = (k, out, data)                                      # the best feasible probe: kept, not recomputed
                elif k == 1:
                    first = (k, out, data)
                return len(data) <= B
            if not probe(k0):
                lo, hi = 0, k0
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    if probe(mid):
                        lo = mid
                    else:
                        hi = mid
            k, out, data = fits if fits is not None else first                   # (nothing fits: rung 1 was the last probe)
            target = {"kind": "bytes", "target": B, "met": fits is not None, "colours": k, "probes": probes, "bound_psnr": bound(k), "refine_dropped": False}
        row = {"from": K, "to": k, "empty": K - live, "steps": live - k}
        return out + (row, target, data)

    def encode_with_palette(self, image, palette, out_path=None, exact=False, roi_mask=None, report=False, refine=0, roi_weight=1, colours=None,
                            target_bytes=None, target_psnr=None, run_slack=None, run_penalty=None, dither=None, pattern=None, pattern_size=4,
                            png_path=None, gif_path=None):
        """image: uint8[H,W,3] (numpy or device tensor); palette: uint8[K,3] (numpy or device tensor) or a dict with "palette" (an
        earlier result, container.read_frame's) -> the FrameEncoder result dict (palette, indices device tensor [H,W], indices_dtype,
        shape, top_left = (0, 0)) whose every index is the nearest palette row (Rhccq.palette_remap: exact integers, ties to the
        lowest row), plus `stats`.  One pass over the pixels: no region, SLIC or clustering stage runs.
        stats["remap"]["all"] = {pixels, sse, mse, psnr} of the result against the image (the kernel's by-product); with roi_mask
        (as encode takes it) also "roi" and "nonroi", inside and outside the mask.  report: stats["quality"] as encode fills it
        (regions() for the region map, then quality()).  out_path: container.write_frame(exact=exact).
        refine = N > 0: the palette is first refined with up to N exact Lloyd iterations over the image (Rhccq.palette_refine: rows
        move to the mean of their pixels, K stays), then the remap runs onto the refined palette, which is the result's "palette".
        With roi_mask a pixel inside the mask weighs roi_weight (1..255) and one outside 1 in the refinement; without a mask
        roi_weight must be 1.  stats["refine"] = {iterations, converged, sse: [...], changed: [...]} (the weighted sums of the
        iterations that ran); stats["remap"] stays the unweighted figures of the final remap.  Rows that receive no pixel never
        move, so a palette far from the image collapses onto a few rows: refinement follows drift, it does not replace encode.
        colours = N (default None = off): the palette is first reduced to at most N rows for this image: a remap onto the given
        palette, the rows' counts (torch.bincount; with roi_mask a pixel inside the mask counts roi_weight, as it weighs in the
        refinement, and roi_weight needs no refine then), Rhccq.palette_reduce (exact pairwise merging; rows no pixel uses are dropped),
        then the refinement, if asked for, of the reduced palette, and the final remap.  stats["reduce"] = {from: K, to: rows kept,
        empty: rows dropped unused, steps: merges}.  K may be at most ops.palette_reduce_max_rows() (RhccqError).
        target_bytes = B or target_psnr = P (exclusive; default None = off): the number of colours is searched on the palette's
        ladder (ladder(): one moments pass, one merge chain, the exact error bound of every rung) instead of given.  The rungs are
        1..k0, k0 = min(colours or K, rows in use); rung k is the palette colours=k uses, and the result is what colours=k, refine=R
        gives (stats["reduce"] and stats["remap"] as colours=k fills them).  stats["target"] = {kind: "bytes" / "psnr", target, met,
        colours: k, probes: [(k, bytes), ...] in the order they ran ([] for a PSNR target), bound_psnr: {table: the bound of rung k},
        refine_dropped}.
        target_psnr: a number for the whole picture, or a dict over "all", "roi", "nonroi" (the last two need roi_mask).  k is the
        smallest rung whose bound (ops.psnr_from_sse of the curve's sum, float64) is >= every constraint; a table without pixels
        meets any; no rung meets them: k = k0.  No probe runs.  Without refine the achieved figures cannot fall below the bound;
        with refine a class can lose to another, and when the final remap's own sums miss a constraint that the unrefined rung
        meets, the unrefined result is returned and refine_dropped is set.  met: the result's own sums meet every constraint.
        target_bytes: probe(k) = rung k, the refinement if asked for, the remap, the container built in memory
        (container.frame_bytes(exact=exact)).  k0 is probed first and is the result when it fits; otherwise a bisection over
        lo = 0 (virtual), hi = k0 with mid = (lo + hi) // 2 keeps lo at the last rung that fitted, and rung lo is the result (lo == 0:
        rung 1 with met False).  File size need not fall monotonically with k: the search returns a rung it verified, not provably
        the largest one that fits.  With out_path the probe's bytes are the file, so its length is the recorded size.
        run_slack = s or {"roi": a, "nonroi": b} (the dict needs roi_mask; default None = off, and 0 is a value: at an exact tie the
        left neighbour's row wins): the final remap, whatever came before it (refine, colours, a target's rungs and probes), is
        the run-carrying one (Rhccq.palette_runs): along every image row a pixel keeps its left neighbour's index while that costs
        at most the slack (0..195075, a squared distance) more squared error than its nearest row.  The index map gets repetitive,
        which the container's zlib stage rewards; the file format does not change.  stats["remap"] stays the figures of the index
        map returned; stats["runs"] = {slack: as given, carried: {all: pixels whose index is not the nearest row[, roi, nonroi]},
        pixels}.  A PSNR target keeps its guarantee: a rung's bound is formed from the curve's sum plus slack x pixels per table
        (exact integers, a valid bound of the run-carrying result's squared error), so rungs come out larger than without a slack,
        and bound_psnr records the adjusted bound.  A byte target probes every rung with the given slack; slack and colours are not
        searched jointly.
        run_penalty = p or {"roi": a, "nonroi": b} (the dict needs roi_mask; default None = off, and 0 is a value; exclusive with
        run_slack: both given raise ValueError): the final remap, in the same place as run_slack's (behind refine, colours and in
        every probe of target_bytes), is the exact row segmentation (Rhccq.palette_segment): per image row the index map that
        minimises the squared error plus the penalty (0..16777215) of every pixel whose index differs from its left neighbour's,
        the pixel's own class deciding its penalty.  The greedy slack approximates this; at equal value the exact map has fewer
        bytes and no more error.  A pixel is at most the penalties of its two boundaries worse than its
        nearest row.  stats["remap"] stays the figures of the index map returned; stats["runs"] = {penalty: as given, carried: {all:
        pixels whose index is not the nearest row[, roi, nonroi]}, breaks: {all: pixels whose index differs from their left
        neighbour's[, roi, nonroi]}, pixels}.  With target_psnr it raises ValueError: two penalties a pixel is the only valid bound
        and too loose to choose a rung by.  A byte target's bound_psnr adds (own + largest penalty) x pixels per table.  The palette
        may have at most ops.palette_segment_max_rows() rows (RhccqError).
        dither = s or {"roi": a, "nonroi": b} (the dict needs roi_mask; default None = off, and 0 is a value: the nearest-row map;
        exclusive with run_slack and run_penalty: ValueError): the final remap, in the same place as theirs (behind refine, colours
        and in every probe of target_bytes), is Floyd-Steinberg error diffusion in exact integers (Rhccq.palette_dither; raster
        order, no serpentine, RGB): a pixel aims at its colour plus s / 256 of the error its left and upper neighbours left behind
        (weights 7, 1, 5, 3 over 16) and takes the nearest row of that; 256 is the classic rule.  It keeps the local mean colour at
        a fixed K, where the nearest-row map bands a gradient; it costs PSNR and index-map bytes.  The
        strength is the receiving pixel's: with {"roi": 0, "nonroi": s} the pixels inside the mask keep their nearest row.
        stats["remap"] stays the figures of the index map returned; stats["dither"] = {strength: as given, moved: {all: pixels whose
        index is not the nearest row[, roi, nonroi]}, pixels}; there is no stats["runs"].  With target_psnr it raises ValueError:
        the ladder's bound is that of the nearest-row map.  A byte target probes every rung with the dither on, and its bound_psnr is
        {table: None}.  The palette may have at most ops.palette_dither_max_rows() rows (RhccqError).
        pattern = s or {"roi": a, "nonroi": b} with pattern_size = n in ops.PATTERN_SIZES (the dict needs roi_mask; default None = off,
        and 0 is a value: the nearest-row map; exclusive with run_slack and run_penalty, and with dither: ValueError): the final remap,
        in the same place as theirs, is pattern dithering in exact integers (Rhccq.palette_pattern): a pixel builds n x n candidate
        rows whose mean approaches it (each candidate the nearest row of the pixel plus s / 256 of the error the earlier ones left),
        orders them by luma, and the Bayer threshold of (y mod n, x mod n) picks one.  The index depends on the pixel and its position
        only, so the same pixel gets the same index in every frame, tile and batch slot, and small noise moves few indices where
        error diffusion moves them everywhere; it is one launch of independent pixels.  On smooth content the periodic pattern reaches
        error diffusion's block means at a fraction of its bytes; on natural content with a rich palette it comes close to its block
        means but does not beat its bytes or PSNR.  stats["remap"] stays the figures of the index map returned;
        stats["pattern"] = {strength: as given, size: n, moved: {all: pixels whose index is not the nearest row[, roi, nonroi]},
        pixels}; there is no stats["runs"].  With target_psnr it raises ValueError, for dither's reason.  A byte target probes every
        rung with the pattern on, and its bound_psnr is {table: None}.  The palette may have at most ops.palette_pattern_max_rows()
        rows (RhccqError).
        png_path (default None = off; independent of out_path): the index map returned, after every rule above, is also written as
        a PNG file built on the device (container.write_png: a palette PNG up to 256 rows, truecolour with adaptive row filters above;
        exact= is shared with out_path and sends IDAT through the level-9 encoder).  stats["png"] = {bytes, colour_type, depth,
        filter_rows}.  A target_bytes counts the .rhccq file's bytes, not the PNG's.
        gif_path (default None = off; independent of out_path and png_path): the index map returned is also written as a one-frame GIF89a
        file built on the device (container.write_gif: one global colour table, segmented LZW, include/rhccq.h).  stats["gif"] = {bytes,
        frames: 1, table: "global", colours, delta: False, stream_bytes}.  A result of more than 256 rows raises ValueError."""
        rh = self.rh
        png_path = self._png_arg("ImageEncoder.encode_with_palette", png_path)
        gif_path = self._png_arg("ImageEncoder.encode_with_palette", gif_path, "gif_path")
        refine, roi_weight = int(refine), int(roi_weight)
        searching = target_bytes is not None or target_psnr is not None
        if refine < 0 or refine > 64:
            raise ValueError("ImageEncoder.encode_with_palette: refine must be 0..64")
        if not 1 <= roi_weight <= 255 or (roi_weight != 1 and (roi_mask is None or not (refine or colours is not None or searching))):
            raise ValueError("ImageEncoder.encode_with_palette: roi_weight (1..255) other than 1 needs roi_mask and refine > 0, colours or a target")
        cons = self._target_args("ImageEncoder.encode_with_palette", target_bytes, target_psnr, roi_mask is not None) if searching else None
        runs = self._runs_args("ImageEncoder.encode_with_palette", run_slack, run_penalty, roi_mask is not None, target_psnr, dither=dither,
                               pattern=pattern, pattern_size=pattern_size)
        if isinstance(palette, dict):
            palette = palette["palette"]
        pal = palette.to(rh.device) if torch.is_tensor(palette) else rh.dev(np.asarray(palette))
        if pal.dtype != torch.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < 1:
            raise ValueError("ImageEncoder.encode_with_palette: a uint8 K x 3 palette, K >= 1, is expected")
        pal = pal.contiguous()
        image, png_in = self._png_in(image)
        rgb = image.to(rh.device).contiguous() if torch.is_tensor(image) else rh.dev(np.asarray(image))
        if rgb.dtype != torch.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("ImageEncoder.encode_with_palette: a uint8 H x W x 3 image is expected")
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        t, t0 = {}, time.perf_counter()

        def lap(name):
            nonlocal t0
            now = time.perf_counter()
            t[name] = now - t0
            t0 = now
        cls = None
        if roi_mask is not None:
            from .api.roi import region_map_from_mask
            cls = region_map_from_mask(rgb, roi_mask, rh)                     # 0 / 1: quality()'s rows
            lap("mask")
        reduce_row = target = data = None
        if searching:
            pal, idx, sums, hist, nit, runs_row, reduce_row, target, data = self._search(rgb, pal, cls, roi_weight, refine, colours, target_bytes, cons,
                                                                                         exact, runs)
            refined = hist is not None
            lap("target")
        else:
            if colours is not None:
                from .container import index_histogram
                first, _ = rh.palette_remap(rgb, pal)
                weights = None if cls is None or roi_weight == 1 else 1 + (roi_weight - 1) * (cls == 1).to(torch.int64)
                pal, reduce_row = self._reduce(pal, index_histogram(first, int(pal.shape[0]), rh, weights), int(colours))
                lap("reduce")
            pal, idx, sums, hist, nit, runs_row = self._finish_palette(rgb, pal, cls, roi_weight, refine, runs)
            refined = bool(refine)
            lap("remap")
        remap = {"all": self._remap_row(*sums[-1])}
        if cls is not None:
            remap["nonroi"], remap["roi"] = self._remap_row(*sums[0]), self._remap_row(*sums[1])
        res = {"palette": rh.to_host(pal), "indices": idx, "indices_dtype": "uint8" if idx.dtype == torch.uint8 else "uint16",
               "shape": (H, W), "top_left": (0, 0)}
        stats = {"remap": remap}
        if reduce_row is not None:
            stats["reduce"] = reduce_row
        if target is not None:
            stats["target"] = target
        if runs_row is not None:
            stats[self._runs_key(runs)] = runs_row
        if refined:
            stats["refine"] = {"iterations": nit, "converged": nit == 0 or int(hist[nit - 1, 1]) == 0,
                               "sse": [int(v) for v in hist[:nit, 0]], "changed": [int(v) for v in hist[:nit, 1]]}
        if out_path:
            from . import container
            if data is not None:                                                  # the probe's bytes are the file
                with open(out_path, "wb") as f:
                    f.write(data)
            else:
                container.write_frame(res, out_path, rh, exact=exact)
            lap("container")
        if png_path:
            stats["png"] = self._png_write(res, png_path, exact)
            lap("png")
        if gif_path:
            stats["gif"] = self._gif_write(res, gif_path)
            lap("gif")
        if report:
            host = image.cpu().numpy() if torch.is_tensor(image) else np.ascontiguousarray(image, dtype=np.uint8)
            _, _, rgb_r, rstats = self.regions(host, roi_mask)
            stats.update(rstats)
            stats["quality"] = self.quality(rgb_r, res, self.region_map)
            lap("report")
        stats["seconds"] = {k: round(v, 4) for k, v in t.items()}
        if png_in is not None:
            stats["png_in"] = png_in
        res["stats"] = stats
        return res

    def _frame_tensor(self, fn, image):
        rh = self.rh
        rgb = image.to(rh.device).contiguous() if torch.is_tensor(image) else rh.dev(np.asarray(image))
        if rgb.dtype != torch.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"ImageEncoder.{fn}: a uint8 H x W x 3 image is expected")
        return rgb

    def _cells(self, fn, rgb, roi_mask, roi_weight, into=None):
        """the frame's histogram table (Rhccq.palette_cells); with a mask a pixel inside it weighs roi_weight and one outside 1"""
        rh = self.rh
        if roi_mask is None:
            return rh.palette_cells(rgb, into=into)
        from .api.roi import region_map_from_mask
        return rh.palette_cells(rgb, region_map_from_mask(rgb, roi_mask, rh), 2, [1, roi_weight, 1], into=into)

    def quantize(self, image, colours=256, out_path=None, exact=False, roi_mask=None, report=False, refine=0, roi_weight=1, target_bytes=None,
                 target_psnr=None, run_slack=None, run_penalty=None, dither=None, pattern=None, pattern_size=4, png_path=None, gif_path=None):
        """image: uint8[H,W,3] (numpy or device tensor) or the name of a PNG file (read on the device by container.read_png; its alpha is
        ignored and stats["png_in"] says what the file was), colours = N -> the result dict of encode_with_palette for a palette of at most N
        rows made from the image itself: one pass over the pixels into a 32 x 32 x 32 colour histogram (Rhccq.palette_cells), greedy
        variance-minimising box splitting over it in exact integers (Rhccq.palette_build: the box whose best cut removes the most
        squared error is split until N boxes exist; a row is the mean of its box's pixels), then exactly what
        encode_with_palette(image, that palette, ...) does: out_path, exact, roi_mask, report, refine, target_bytes, target_psnr,
        run_slack, run_penalty, dither, pattern and pattern_size keep their meaning and validation.  No region, SLIC or clustering stage runs, and no palette is
        needed to start from.  With roi_mask a pixel inside the mask weighs roi_weight (1..255) in the histogram, so roi_weight other
        than 1 needs only the mask here (and weighs in the refinement too when refine > 0).  N may be at most
        ops.palette_build_max_rows() (RhccqError).  Colours that share a cell of the histogram (equal in their upper five bits per
        channel) are never separated, so fewer than N rows come back when fewer cells are occupied, and two boxes may round to the
        same row.  stats["build"] = {asked: N, rows: rows built, cells: occupied cells, steps: splits}; everything else as
        encode_with_palette fills it.  png_path, gif_path: as encode_with_palette takes them (gif_path raises ValueError when
        colours is above 256, before anything runs)."""
        rh = self.rh
        png_path = self._png_arg("ImageEncoder.quantize", png_path)
        gif_path = self._png_arg("ImageEncoder.quantize", gif_path, "gif_path")
        if gif_path and int(colours) > 256:
            raise ValueError("ImageEncoder.quantize: gif_path needs colours <= 256 (a GIF colour table has at most 256 rows)")
        colours, refine, roi_weight = int(colours), int(refine), int(roi_weight)
        searching = target_bytes is not None or target_psnr is not None
        if colours < 1:
            raise ValueError("ImageEncoder.quantize: colours >= 1 is required")
        if refine < 0 or refine > 64:
            raise ValueError("ImageEncoder.quantize: refine must be 0..64")
        if not 1 <= roi_weight <= 255 or (roi_weight != 1 and roi_mask is None):
            raise ValueError("ImageEncoder.quantize: roi_weight (1..255) other than 1 needs roi_mask")
        if searching:
            self._target_args("ImageEncoder.quantize", target_bytes, target_psnr, roi_mask is not None)
        self._runs_args("ImageEncoder.quantize", run_slack, run_penalty, roi_mask is not None, target_psnr, dither=dither, pattern=pattern,
                        pattern_size=pattern_size)
        image, png_in = self._png_in(image)
        rgb = self._frame_tensor("quantize", image)
        t0 = time.perf_counter()
        cells = self._cells("quantize", rgb, roi_mask, roi_weight)
        pal, _, splits, _ = rh.palette_build(cells, colours)
        build = {"asked": colours, "rows": int(pal.shape[0]), "cells": int((cells[0] != 0).sum()), "steps": int(splits.shape[0])}
        seconds = time.perf_counter() - t0
        res = self.encode_with_palette(rgb, pal, out_path=out_path, exact=exact, roi_mask=roi_mask, report=report, refine=refine,
                                       roi_weight=roi_weight if (refine or searching) else 1, target_bytes=target_bytes, target_psnr=target_psnr,
                                       run_slack=run_slack, run_penalty=run_penalty, dither=dither, pattern=pattern, pattern_size=pattern_size,
                                       png_path=png_path, gif_path=gif_path)
        res["stats"]["build"] = build
        res["stats"]["seconds"] = dict({"build": round(seconds, 4)}, **res["stats"]["seconds"])
        if png_in is not None:
            res["stats"]["png_in"] = png_in
        return res

    # images of one slice of quantize_batch: a slice holds 1 MiB of histogram and 1.1 MiB of summed-volume table per image beside its
    # pixels and indices (128 images: 275 MiB), and 128 chains are half the card's CUs, so two slices' chains already fill it
    QUANTIZE_BATCH_SLICE = 128

    def quantize_batch(self, images, colours=256, refine=0, roi_masks=None, roi_weight=1, out_paths=None, exact=False, pattern=None, pattern_size=4,
                       gif_path=None, delay=4):
        """images: a list of uint8[H,W,3] images of any sizes (numpy or device tensors), or one uint8[B,H,W,3] array or device tensor
        (a contiguous device tensor is used in place, nothing is concatenated) -> a list with one result dict per image: what
        quantize(image, colours, refine=refine, roi_mask=mask, roi_weight=...) returns for that image alone, bit for bit (palette
        trimmed to its rows, indices [H,W], stats["build"], stats["remap"], stats["refine"]); only stats["seconds"] differs
        ({"batch": the whole call}).  roi_masks: one mask (or None) per image; a pixel inside its mask weighs roi_weight (1..255),
        which other than 1 needs at least one mask; an image without a mask is quantised as with roi_weight = 1.
        The images are laid back to back and every stage runs once for all of them (Rhccq.palette_cells_batch, palette_build_batch:
        one split chain per image side by side, palette_refine_batch, palette_remap_batch); the rows each image got stay on the
        device between the stages, and the host reads everything it needs (rows, sums, histories, iterations, occupied cells, the
        palettes) ONCE, after the whole batch is queued.  The index width is chosen by `colours` (uint8 up to 256, else 16 bits);
        an image that ends with 256 rows or fewer is narrowed to uint8 afterwards, as quantize returns it.  More than
        QUANTIZE_BATCH_SLICE (128) images are queued in slices of that many, which bounds the workspace; the one read stays one.
        out_paths: one file name (or None) per image, written afterwards with container.write_frame(exact=exact), one by one.
        pattern = s or {"roi": a, "nonroi": b} with pattern_size (default None = off): as quantize takes them; the last stage is then
        Rhccq.palette_pattern_batch instead of the remap, every image's result still what quantize(..., pattern=, pattern_size=) gives
        for it alone, stats["pattern"] included.  A pixel's index depends on the pixel and its position only, which is what lets a
        batch take this rule and not dither.  The dict needs a mask for every image.
        target_bytes, target_psnr, run_slack, run_penalty, dither and report are not parameters: each needs a host decision per image
        (dither: a status word and a workspace per image); quantize has them.  Validation and error types follow quantize; an image whose table is empty (no pixels) raises
        RhccqError after the read, as quantize does for it.
        gif_path (default None = off), delay (centiseconds, one number or one an image): the results are also written as ONE GIF89a
        file on the device (container.write_gif), every image a frame with its own palette in a local colour table, no delta; the
        images must then be of one size and colours at most 256 (ValueError).  stats["gif"] (the same row in every result) =
        {bytes, frames, table: "local" ("global" when all palettes came out equal), colours, delta: False, stream_bytes}."""
        rh = self.rh
        fn = "ImageEncoder.quantize_batch"
        colours, refine, roi_weight = int(colours), int(refine), int(roi_weight)
        gif_path = self._png_arg(fn, gif_path, "gif_path")
        if gif_path and colours > 256:
            raise ValueError(f"{fn}: gif_path needs colours <= 256 (a GIF colour table has at most 256 rows)")
        if colours < 1:
            raise ValueError(f"{fn}: colours >= 1 is required")
        if refine < 0 or refine > 64:
            raise ValueError(f"{fn}: refine must be 0..64")
        stacked = None
        if (torch.is_tensor(images) or isinstance(images, np.ndarray)) and images.ndim == 4:
            stacked = images.to(rh.device).contiguous() if torch.is_tensor(images) else rh.dev(images)
            if stacked.dtype != torch.uint8 or stacked.shape[3] != 3:
                raise ValueError(f"{fn}: a uint8 B x H x W x 3 tensor is expected")
            frames = list(stacked)                                               # views
        else:
            frames = [self._frame_tensor("quantize_batch", im) for im in images]
        B = len(frames)
        masks = [None] * B if roi_masks is None else list(roi_masks)
        paths = [None] * B if out_paths is None else list(out_paths)
        if B < 1 or len(masks) != B or len(paths) != B:
            raise ValueError(f"{fn}: at least one image, and one mask and one path (or None) per image, are expected")
        if gif_path and any(f.shape[:2] != frames[0].shape[:2] for f in frames):
            raise ValueError(f"{fn}: gif_path needs images of one size")
        masked = any(m is not None for m in masks)
        if not 1 <= roi_weight <= 255 or (roi_weight != 1 and not masked):
            raise ValueError(f"{fn}: roi_weight (1..255) other than 1 needs roi_masks")
        runs = self._runs_args(fn, None, None, all(m is not None for m in masks), pattern=pattern, pattern_size=pattern_size)
        if colours > ops.palette_build_max_rows():
            raise RhccqError(f"{fn}: {colours} colours, the device form returns at most {ops.palette_build_max_rows()} (palette_build_max_rows())")
        t0 = time.perf_counter()
        nc, weights = (2, [1, roi_weight, 1]) if masked else (0, None)
        queued = []
        for s0 in range(0, B, self.QUANTIZE_BATCH_SLICE):
            part = frames[s0:s0 + self.QUANTIZE_BATCH_SLICE]
            off = np.concatenate([[0], np.cumsum([int(f.shape[0]) * int(f.shape[1]) for f in part])]).astype(np.int64)
            if stacked is not None:
                rgb = stacked[s0:s0 + len(part)].reshape(-1, 3)
            else:
                rgb = part[0].reshape(-1, 3) if len(part) == 1 else torch.cat([f.reshape(-1, 3) for f in part])
            cls = None
            if masked:
                # an image without a mask takes the class outside both (2): weight 1 everywhere, and no row of the class sums
                from .api.roi import region_map_from_mask
                maps = [torch.full((int(off[i + 1] - off[i]),), 2, dtype=torch.uint8, device=rh.device) if m is None
                        else region_map_from_mask(f, m, rh).reshape(-1) for i, (f, m) in enumerate(zip(part, masks[s0:s0 + len(part)]))]
                cls = maps[0] if len(maps) == 1 else torch.cat(maps)
            off_dev = rh.dev(off)
            cells = rh.palette_cells_batch(rgb, off, cls, nc, weights, px_off_dev=off_dev)
            occupied = (cells[:, 0] != 0).sum(dim=(1, 2, 3))
            pal, _, _, _, k = rh.palette_build_batch(cells, colours)
            hist = nit = None
            if refine:
                pal, hist, nit = rh.palette_refine_batch(rgb, off, pal, k, cls, weights, max_iter=refine, px_off_dev=off_dev)
            if runs is not None:
                idx, sums = rh.palette_pattern_batch(rgb, off, [int(f.shape[1]) for f in part], pal, k, self._slack_table(runs, masked), runs["size"], cls,
                                                     nc, px_off_dev=off_dev)
            else:
                idx, sums = rh.palette_remap_batch(rgb, off, pal, k, cls, nc, px_off_dev=off_dev)
            queued.append((off, idx, [k, occupied, sums, pal] + ([hist, nit] if refine else [])))
        host = rh.to_host(*[t for _, _, ts in queued for t in ts])                 # the one read
        out, at = [], 0
        for s, (off, idx, ts) in enumerate(queued):
            k, occupied, sums, pal = host[at:at + 4]
            hist, nit = host[at + 4:at + 6] if refine else (None, None)
            at += len(ts)
            for b in range(len(off) - 1):
                i = s * self.QUANTIZE_BATCH_SLICE + b
                rows = int(k[b])
                if rows < 0:                                                     # the errors only the table shows come back through k
                    raise RhccqError(f"{fn}: image {i}: palette_build failed ({rows}): "
                                     + ("the table is empty" if rows == -1 else "the table's N adds up to more than 2^32 - 1"))
                H, W = int(frames[i].shape[0]), int(frames[i].shape[1])
                ind = idx[int(off[b]):int(off[b + 1])].reshape(H, W)
                if ind.dtype != torch.uint8 and rows <= 256:
                    ind = ind.to(torch.uint8)
                remap = {"all": self._remap_row(*sums[b][-1][:2])}
                if masks[i] is not None:
                    remap["nonroi"], remap["roi"] = self._remap_row(*sums[b][0][:2]), self._remap_row(*sums[b][1][:2])
                stats = {"remap": remap}
                if runs is not None:
                    stats["pattern"] = self._runs_row(runs, sums[b], masks[i] is not None)
                if refine:
                    n = int(nit[b])
                    stats["refine"] = {"iterations": n, "converged": n == 0 or int(hist[b][n - 1, 1]) == 0,
                                       "sse": [int(v) for v in hist[b][:n, 0]], "changed": [int(v) for v in hist[b][:n, 1]]}
                stats["build"] = {"asked": colours, "rows": rows, "cells": int(occupied[b]), "steps": rows - 1}
                out.append({"palette": np.ascontiguousarray(pal[b][:rows]), "indices": ind, "indices_dtype": "uint8" if ind.dtype == torch.uint8 else "uint16",
                            "shape": (H, W), "top_left": (0, 0), "stats": stats})
        if any(p for p in paths):
            from . import container
            for res, p in zip(out, paths):
                if p:
                    container.write_frame(res, p, rh, exact=exact)
        if gif_path:
            row = self._gif_write(out, gif_path, delay=delay)
            for res in out:
                res["stats"]["gif"] = row
        seconds = {"batch": round(time.perf_counter() - t0, 4)}
        for res in out:
            res["stats"]["seconds"] = dict(seconds)
        return out

    def shared_palette(self, images, colours, roi_masks=None, roi_weight=1):
        """images: uint8[H,W,3] each (any sizes), colours = N -> one palette (device uint8[k, 3], k <= N) for all of them: the images'
        histogram tables are summed into one (Rhccq.palette_cells(into=)) and the split chain runs once (Rhccq.palette_build), so the
        result is the palette quantize would build for the pictures laid side by side.  roi_masks: one mask (or None) per image;
        a pixel inside its mask weighs roi_weight (1..255).  The weights of all images together may add up to at most 2^32 - 1."""
        colours, roi_weight = int(colours), int(roi_weight)
        images = list(images)
        masks = [None] * len(images) if roi_masks is None else list(roi_masks)
        if not images or len(masks) != len(images):
            raise ValueError("ImageEncoder.shared_palette: at least one image, and one mask (or None) per image, are expected")
        if colours < 1:
            raise ValueError("ImageEncoder.shared_palette: colours >= 1 is required")
        if not 1 <= roi_weight <= 255 or (roi_weight != 1 and all(m is None for m in masks)):
            raise ValueError("ImageEncoder.shared_palette: roi_weight (1..255) other than 1 needs roi_masks")
        cells = None
        for image, mask in zip(images, masks):
            cells = self._cells("shared_palette", self._frame_tensor("shared_palette", image), mask, roi_weight, into=cells)
        return self.rh.palette_build(cells, colours)[0]

    def animate(self, images, colours=256, gif_path=None, delay=None, loop=None, delta=True, refine=0, roi_masks=None, roi_weight=1, pattern=None,
                pattern_size=4):
        """images: a list of uint8[H,W,3] frames of ONE size (numpy or device tensors), or one uint8[B,H,W,3] array or device tensor ->
        {"palette": uint8[k, 3], "indices": device uint8[B, H, W], "indices_dtype": "uint8", "shape": (H, W), "stats"}: an animated GIF89a built on the device from end to end.  One shared_palette over all frames (at most `colours` rows,
        1..256; with delta at most 255, because the transparent index is one more table entry: stats["gif"]["colours"] says what was
        built), refine = N > 0 Lloyd iterations of that ONE palette over the pixels of all frames (Rhccq.palette_refine), every frame
        onto the palette in one batch launch (Rhccq.palette_remap_batch, or palette_pattern_batch with pattern = s or {"roi": a,
        "nonroi": b} and pattern_size, as quantize_batch takes them), then the file (Rhccq.gif_encode: one global colour table, delay
        in centiseconds -- one number or one a frame --, loop = the repeat count, 0 for ever).  delta=True writes a pixel that keeps its
        index from the frame in front as transparent; a frame's index map is what encode_with_palette(frame, palette[, pattern=]) gives
        for it alone, so with pattern a pixel that does not change keeps its index and costs nothing.  roi_masks: one mask (or None) a
        frame; a pixel inside weighs roi_weight (1..255) in the shared histogram and the refinement.  gif_path: where the file is written
        (None: it is built, stats["gif"] says what it is, and it is dropped).  stats = {"build": {asked, rows}, "remap": [a row a frame], "pattern": [a row a frame] with pattern, "refine" with refine,
        "gif": container.gif_file's row, "seconds"}.
        dither, run_slack, run_penalty and the targets are not parameters: error diffusion is not frame-stable (a changed pixel moves
        the indices of everything to its right and below, so delta would find nothing), and the run rules and targets decide per
        image on the host.
        images may also be an animated GIF itself: a file name ending in .gif, or bytes that start with "GIF8".  It is read on the device
        (container.read_gif: the composed frames, an uncovered pixel as colour 0), and delay and loop default to the file's own (loop 0
        where the file has no loop count); otherwise they default to 4 and 0."""
        rh = self.rh
        fn = "ImageEncoder.animate"
        colours, refine, roi_weight = int(colours), int(refine), int(roi_weight)
        gif_path = self._png_arg(fn, gif_path, "gif_path")
        if not 1 <= colours <= 256:
            raise ValueError(f"{fn}: colours must be 1..256 (a GIF colour table has at most 256 rows)")
        if refine < 0 or refine > 64:
            raise ValueError(f"{fn}: refine must be 0..64")
        if (isinstance(images, str) and images.lower().endswith(".gif")) or (isinstance(images, (bytes, bytearray, memoryview)) and bytes(images[:4]) == b"GIF8"):
            from . import container
            src = container.read_gif(images, rh)
            images = src["images"]
            delay = src["delays"] if delay is None else delay
            loop = (src["loop"] or 0) if loop is None else loop
        delay, loop = 4 if delay is None else delay, 0 if loop is None else loop
        stacked = None
        if (torch.is_tensor(images) or isinstance(images, np.ndarray)) and images.ndim == 4:
            stacked = images.to(rh.device).contiguous() if torch.is_tensor(images) else rh.dev(images)
            if stacked.dtype != torch.uint8 or stacked.shape[3] != 3:
                raise ValueError(f"{fn}: a uint8 B x H x W x 3 tensor is expected")
            frames = list(stacked)                                               # views
        else:
            frames = [self._frame_tensor("animate", im) for im in images]
        B = len(frames)
        masks = [None] * B if roi_masks is None else list(roi_masks)
        if B < 1 or len(masks) != B:
            raise ValueError(f"{fn}: at least one frame, and one mask (or None) per frame, are expected")
        if any(f.shape[:2] != frames[0].shape[:2] for f in frames):
            raise ValueError(f"{fn}: every frame must have the same shape")
        H, W = int(frames[0].shape[0]), int(frames[0].shape[1])
        if H > 65535 or W > 65535:
            raise ValueError(f"{fn}: a GIF frame is at most 65535 x 65535")
        masked = any(m is not None for m in masks)
        if not 1 <= roi_weight <= 255 or (roi_weight != 1 and not masked):
            raise ValueError(f"{fn}: roi_weight (1..255) other than 1 needs roi_masks")
        runs = self._runs_args(fn, None, None, all(m is not None for m in masks), pattern=pattern, pattern_size=pattern_size)
        t0 = time.perf_counter()
        asked = min(colours, 255) if delta else colours
        pal = self.shared_palette(frames, asked, masks if masked else None, roi_weight)
        rgb = stacked.reshape(-1, 3) if stacked is not None else frames[0].reshape(-1, 3) if B == 1 else torch.cat([f.reshape(-1, 3) for f in frames])
        off = (np.arange(B + 1) * (H * W)).astype(np.int64)
        nc, weights, cls = 0, None, None
        if masked:
            from .api.roi import region_map_from_mask
            nc, weights = 2, [1, roi_weight, 1]
            maps = [torch.full((H * W,), 2, dtype=torch.uint8, device=rh.device) if m is None else region_map_from_mask(f, m, rh).reshape(-1)
                    for f, m in zip(frames, masks)]
            cls = maps[0] if B == 1 else torch.cat(maps)
        hist = nit = None
        if refine:
            pal, hist, nit = rh.palette_refine(rgb, pal, cls, weights, max_iter=refine)
        K = int(pal.shape[0])
        pals = pal.unsqueeze(0).expand(B, K, 3).contiguous()
        k = torch.full((B,), K, dtype=torch.int32, device=rh.device)
        off_dev = rh.dev(off)
        if runs is not None:
            idx, sums = rh.palette_pattern_batch(rgb, off, [W] * B, pals, k, self._slack_table(runs, masked), runs["size"], cls, nc, px_off_dev=off_dev)
        else:
            idx, sums = rh.palette_remap_batch(rgb, off, pals, k, cls, nc, px_off_dev=off_dev)
        out, length, lens = rh.gif_encode_async(idx, B, H, W, pal, None, delay, loop, bool(delta))
        host = rh.to_host(*([sums, pal, length, lens] + ([hist, nit] if refine else [])))
        sums, pal_host, size, lens = host[0], host[1], int(host[2][0]), host[3]
        stats = {"build": {"asked": asked, "rows": K}, "remap": []}
        for b in range(B):
            row = {"all": self._remap_row(*sums[b][-1][:2])}
            if masks[b] is not None:
                row["nonroi"], row["roi"] = self._remap_row(*sums[b][0][:2]), self._remap_row(*sums[b][1][:2])
            stats["remap"].append(row)
        if runs is not None:
            stats["pattern"] = [self._runs_row(runs, sums[b], masks[b] is not None) for b in range(B)]
        if refine:
            n = int(host[5][0])
            stats["refine"] = {"iterations": n, "converged": n == 0 or int(host[4][n - 1, 1]) == 0, "sse": [int(v) for v in host[4][:n, 0]],
                               "changed": [int(v) for v in host[4][:n, 1]]}
        stats["gif"] = {"bytes": size, "frames": B, "table": "global", "colours": K, "delta": bool(delta), "stream_bytes": [int(v) for v in lens]}
        if gif_path:
            with open(gif_path, "wb") as f:
                f.write(rh.to_host(out[:size]).tobytes())
        stats["seconds"] = {"animate": round(time.perf_counter() - t0, 4)}
        return {"palette": np.ascontiguousarray(pal_host), "indices": idx.reshape(B, H, W), "indices_dtype": "uint8", "shape": (H, W),
                "stats": stats}

    def encode_sequence(self, images, roi_quality, nonroi_quality, max_drop_db, out_paths=None, exact=False, refine=0, roi_weight=1, max_colours=None,
                        target_bytes=None, target_psnr=None, run_slack=None, run_penalty=None, key_colours=None, pattern=None, pattern_size=4):
        """generator over `images` (uint8[H,W,3] each): frame 0 is a key frame, a plain encode(image, roi_quality, nonroi_quality);
        every later frame is remapped onto the current key frame's palette (encode_with_palette; the palette stays on the device)
        and kept as that iff its PSNR is at least the key frame's PSNR - max_drop_db, otherwise it is encoded in full and becomes
        the key.  Both PSNRs are ops.psnr_from_sse over the same pixels: the key frame's sum comes from
        Rhccq.class_error_sums_indexed over the rectangle its result covers (top_left / shape), the remap's from the kernel's
        sums, over the whole picture when the key covers it and else over that rectangle (the remap then runs with the rectangle
        as its roi_mask, and its stats["remap"] has the "roi" / "nonroi" rows too).  A frame of another size than its key's is
        compared over the whole picture.  Every result has stats["key_frame"] (bool), stats["key_index"] (the frame whose
        palette it uses) and stats["psnr"]; a remap also stats["key_psnr"].  out_paths: one file per frame (entries may be None).
        refine = N > 0: a frame whose plain remap falls below the bound is next tried as encode_with_palette(image, current palette,
        refine=N) (with the key's rectangle as roi_mask and roi_weight inside it when the key covers a rectangle) and kept iff that
        reaches the bound: stats["key_frame"] = False, stats["refined"] = True, key_index and key_psnr stay the key frame's, and the
        refined palette is the one later frames are remapped onto.  Otherwise the frame is encoded in full as before.  Every
        result that is not a key frame has stats["refined"] (bool; always False with refine = 0).
        max_colours: passed to the key frames' encode (default None = off).  target_bytes / target_psnr: passed to the key
        frames' encode too (exclusive with each other and with max_colours; see encode for how the search differs from max_colours).
        run_slack: one number (default None = off), passed to the key frames' encode and to every remap (plain and refined), whose
        PSNRs the key-frame rule then compares; a roi / nonroi dict raises ValueError, because a remapped frame has no region map.
        run_penalty: one number (default None = off), by the same rules (exclusive with run_slack and with target_psnr).
        key_colours = N (default None = off: key frames are encoded in full, as above): a key frame is made by
        quantize(image, colours=N) instead of encode, in about the time of a few remaps; roi_quality and nonroi_quality are not used
        then, max_colours is exclusive with it (ValueError), and target_bytes, target_psnr, run_slack and run_penalty go to quantize.
        pattern: one number (default None = off) with pattern_size, by run_slack's rules (exclusive with it, with run_penalty and with
        target_psnr): key frames and remapped or refined frames alike end in the pattern dither (Rhccq.palette_pattern), whose index for
        a pixel depends on the pixel and its position only, so what does not change between frames keeps its index.  The PSNR the
        key-frame rule compares is that of the dithered map, the map that is returned."""
        rh = self.rh
        refine, roi_weight = int(refine), int(roi_weight)
        if key_colours is not None:
            key_colours = int(key_colours)
            if max_colours is not None:
                raise ValueError("ImageEncoder.encode_sequence: key_colours and max_colours are exclusive")
            if key_colours < 1:
                raise ValueError("ImageEncoder.encode_sequence: key_colours >= 1 is required")
        if target_bytes is not None or target_psnr is not None:
            if max_colours is not None:
                raise ValueError("ImageEncoder.encode_sequence: target_bytes / target_psnr and max_colours are exclusive")
            self._target_args("ImageEncoder.encode_sequence", target_bytes, target_psnr, True)
        if isinstance(run_slack, dict) or isinstance(run_penalty, dict):
            raise ValueError("ImageEncoder.encode_sequence: run_slack / run_penalty is one number (a remapped frame has no region map)")
        if isinstance(pattern, dict):
            raise ValueError("ImageEncoder.encode_sequence: pattern is one number (a remapped frame has no region map)")
        self._runs_args("ImageEncoder.encode_sequence", run_slack, run_penalty, False, target_psnr, pattern=pattern, pattern_size=pattern_size)
        if refine < 0 or refine > 64:
            raise ValueError("ImageEncoder.encode_sequence: refine must be 0..64")
        if not 1 <= roi_weight <= 255 or (roi_weight != 1 and not refine):
            raise ValueError("ImageEncoder.encode_sequence: roi_weight must be 1..255, and 1 without refine")
        key_pal = key_psnr = key_window = key_frame_shape = None
        key_index = -1
        for n, image in enumerate(images):
            path = out_paths[n] if out_paths is not None else None
            if key_pal is not None:
                window = key_window if tuple(image.shape[:2]) == key_frame_shape else None
                res = self.encode_with_palette(image, key_pal, roi_mask=window, run_slack=run_slack, run_penalty=run_penalty, pattern=pattern,
                                               pattern_size=pattern_size)
                row = res["stats"]["remap"]["all" if window is None else "roi"]
                kept = row["psnr"] is not None and row["psnr"] >= key_psnr - max_drop_db
                refined = False
                if not kept and refine:
                    res = self.encode_with_palette(image, key_pal, roi_mask=window, refine=refine, roi_weight=roi_weight if window is not None else 1,
                                                   run_slack=run_slack, run_penalty=run_penalty, pattern=pattern, pattern_size=pattern_size)
                    row = res["stats"]["remap"]["all" if window is None else "roi"]
                    kept = refined = row["psnr"] is not None and row["psnr"] >= key_psnr - max_drop_db
                if kept:
                    if path:
                        from . import container
                        container.write_frame(res, path, rh, exact=exact)
                    res["stats"].update(key_frame=False, key_index=key_index, psnr=row["psnr"], key_psnr=key_psnr)
                    res["stats"]["refined"] = refined
                    if refined:
                        key_pal = rh.dev(np.asarray(res["palette"], np.uint8).reshape(-1, 3))
                    yield res
                    continue
            if key_colours is not None:
                res = self.quantize(image, colours=key_colours, out_path=path, exact=exact, target_bytes=target_bytes, target_psnr=target_psnr,
                                    run_slack=run_slack, run_penalty=run_penalty, pattern=pattern, pattern_size=pattern_size)
            else:
                res = self.encode(image, roi_quality, nonroi_quality, out_path=path, exact=exact, max_colours=max_colours, target_bytes=target_bytes,
                                  target_psnr=target_psnr, run_slack=run_slack, run_penalty=run_penalty, pattern=pattern, pattern_size=pattern_size)
            (top, left), (h, w) = res["top_left"], res["shape"]
            rgb = image.to(rh.device) if torch.is_tensor(image) else rh.dev(np.ascontiguousarray(image, dtype=np.uint8))
            key_frame_shape = (int(rgb.shape[0]), int(rgb.shape[1]))
            key_window = None
            if (int(top), int(left), int(h), int(w)) != (0, 0) + key_frame_shape:
                key_window = torch.zeros(key_frame_shape, dtype=torch.uint8, device=rh.device)
                key_window[top:top + h, left:left + w] = 1
            rgb = rgb[top:top + h, left:left + w].contiguous()
            every = torch.zeros((h, w), dtype=torch.uint8, device=rh.device)      # one class: the whole rectangle
            key_pal = rh.dev(np.asarray(res["palette"], np.uint8).reshape(-1, 3))
            row = rh.class_error_sums_indexed(rgb, res["indices"].reshape(-1), key_pal, every, 1)[0]
            key_index = n
            key_psnr = psnr_from_sse(int(row[0]) + int(row[1]) + int(row[2]), int(row[5]))
            res["stats"].update(key_frame=True, key_index=n, psnr=key_psnr)
            yield res
