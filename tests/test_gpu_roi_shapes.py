"""Every step of the ROI stage (csrc/edges.hip, morph.hip, ccl.hip through ops.Rhccq, api/edges.py, api/roi_chain.py, api/roi.py and
the mirrored encoder/ROI) on tile-edge and degenerate shapes: device == oracle, exactly, dtype included.  GPU only.

The shapes, contents and the oracle side of every step come from tests/test_roi_shapes_cpu.py (which pins the oracle itself to scipy
/ literal definitions on the same shapes): frames narrower than one 64 x 16 tile, of exactly one tile, one pixel over, strips, and
frames smaller than the structuring element or window (the halo tiles are (16 + 2r) x (64 + 2r), BORDER_REFLECT_101 reflects several
times).  Contents: random masks, discs, all set / unset, single pixels, and pixels / lines on either side of every tile seam.

Not vacuous: for every shape of 64 pixels or more each step of MUST_VARY / MUST_VARY_CHAIN must give an oracle output with more than
one distinct value for at least one content (asserted from the oracle's outputs here and, without a GPU, in test_roi_shapes_cpu.py).
The chain entry points (get_edge_map, find_best_edges_by_quality, get_regions) saturate on small frames (ROI = everything), which is
why every step is compared on its own; they are compared all the same, and where the oracle raises (no threshold pair yields an edge)
the device must raise the same exception type."""
import numpy as np
import pytest

from test_roi_shapes_cpu import (ELEMENTS, MUST_VARY, MUST_VARY_CHAIN, SHAPE_IDS, SHAPES, _u8, chain_contents, image_contents, mask_contents,
                                 oracle_chain_steps, oracle_mask_steps, varies)

pytestmark = pytest.mark.gpu
shapes = pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), what


class Varied:
    """which steps gave a non-constant ORACLE output on at least one content of this shape"""

    def __init__(self):
        self.seen = set()

    def note(self, step, want):
        if varies(want):
            self.seen.add(step)

    def check(self, shape, must):
        if shape[0] * shape[1] >= 64:
            missing = [s for s in must if s not in self.seen]
            assert not missing, (shape, missing)


def _ctx():
    import torch
    from roibasedimagecompression_amd.ops import default_context
    rh = default_context()
    return rh, (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rh.device))


def device_mask_steps(rh):
    from encoder.ROI.edges import compute_local_density
    s = {}
    for name, hw in ELEMENTS:
        s[f"dilate_{name}"] = lambda t, m, hw=hw: rh.morph(t, hw).cpu().numpy()
        s[f"erode_{name}"] = lambda t, m, hw=hw: rh.morph(t, hw, erode=True).cpu().numpy()
        s[f"close_{name}"] = lambda t, m, hw=hw: rh.morph_close(t, hw).cpu().numpy()
    s["dilate_rect18"] = lambda t, m: rh.morph_rect(t, 18).cpu().numpy()                   # even: the spans form
    s["erode_rect18"] = lambda t, m: rh.morph_rect(t, 18, erode=True).cpu().numpy()
    s["close_rect18"] = lambda t, m: rh.morph_close_rect(t, 18).cpu().numpy()
    s["chamfer"] = lambda t, m: rh.dist_chamfer(t).cpu().numpy()
    for k in (3, 15, 25, 31):
        s[f"box_count_{k}"] = lambda t, m, k=k: rh.box_count(t, k).cpu().numpy().view(np.uint16)
    for k in (3, 7, 11, 13, 15, 25):
        s[f"density_{k}"] = lambda t, m, k=k: compute_local_density(m, k)
    return s


@shapes
def test_mask_primitives_on_shape(shape):
    """dilate / erode / close (rectangles 3, 15, 31, the ellipses 5 and 11, an element with empty rows, the even 18 x 18 through the
    spans form), the chamfer distance, box counts 3 / 15 / 25 / 31 and the local density 3 / 7 / 11 (direct) / 13 / 15 / 25 (DFT) on
    every content; masks come back 0 / 255 uint8, distances int32, counts uint16, densities float32"""
    rh, up = _ctx()
    ora, dev = oracle_mask_steps(), device_mask_steps(rh)
    seen = Varied()
    for cname, m in mask_contents(*shape):
        t = up(m)
        for step, f in ora.items():
            want = f(m)
            seen.note(step, want)
            got = dev[step](t, m)
            if want.dtype == bool:
                want = _u8(want)                                              # the device's planes are 0 / 255
            elif step == "chamfer":
                assert got.dtype == np.int32
                got = got.astype(np.int64)
            elif step.startswith("box_count"):
                got = got.astype(np.int64)
            same(got, want, (cname, step))
    seen.check(shape, MUST_VARY)


@shapes
def test_local_density_planes_on_shape(shape):
    """compute_local_density and the sequential float32 box filter on 0 / 255, 0 / 1 and mixed 0 / 1 / 255 planes"""
    from oracle import rhccq_oracle as O
    from encoder.ROI.edges import compute_local_density
    rh, up = _ctx()
    for cname, m in chain_contents(*shape):
        mixed = m.copy()
        mixed[::3, ::2] = np.where(mixed[::3, ::2] != 0, 1, 0)
        for pname, plane in (("0/255", m), ("0/1", (m != 0).astype(np.uint8)), ("mixed", mixed)):
            for k in (3, 7, 11, 13, 15, 25):
                want = O.local_density(plane, k)
                same(compute_local_density(plane, k), want, (cname, pname, k))
                if k <= 11:
                    same(rh.box_filter_seq(up(plane), k, bool(plane.max() > 1)).cpu().numpy(), want, (cname, pname, k, "seq"))
            if len(np.unique(plane)) == 3:
                same(rh.box_sum(up(plane), 15).cpu().numpy().astype(np.int64), _window_sums(plane, 15), (cname, "box_sum"))


def _window_sums(plane, k):
    pad = np.pad(plane.astype(np.int64), k // 2, mode="reflect")
    h, w = plane.shape
    return sum(pad[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k))


@shapes
def test_connected_components_and_label_sums_on_shape(shape):
    """ccl for both connectivities and numberings with cap = 1 (any mask of two components takes the capacity retry), ccl_select, and
    label_sum of a uint16 and an int32 plane"""
    from oracle import rhccq_oracle as O
    rh, up = _ctx()
    retried = False
    for cname, m in mask_contents(*shape):
        t = up(m)
        for connectivity in (4, 8):
            for numbering in ("opencv", "raster"):
                n, lab, stats = rh.ccl(t, connectivity, cap=1, numbering=numbering)
                num, want, wstats = O.cv_connected_components_with_stats(m, connectivity, numbering)
                retried |= n > 1
                assert n + 1 == num, (cname, connectivity, numbering)
                same(lab.cpu().numpy(), want, (cname, connectivity, numbering))
                same(stats[1:], wstats[1:], (cname, connectivity, numbering))
                if (m == 0).any():
                    same(stats[0], wstats[0], (cname, connectivity, numbering))
            keep = np.zeros(n + 1, np.uint8)
            keep[1::2] = 255
            same(rh.ccl_select(lab, keep).cpu().numpy(), keep[want], (cname, connectivity, "select"))
            labels = lab.cpu().numpy()
            for k in (3, 15):
                sums = rh.label_sum(lab, n, rh.box_count(t, k))
                same(sums, np.bincount(labels.ravel(), weights=O.box_counts(m, k).ravel(), minlength=n + 1).astype(np.uint64), (cname, "label_sum", k))
            dist = O.cv_dist_chamfer3(m)
            same(rh.label_sum(lab, n, rh.dist_chamfer(t)),
                 np.bincount(labels.ravel(), weights=dist.ravel(), minlength=n + 1).astype(np.uint64), (cname, "label_sum dist"))   # (< 2^53: exact)
    if shape[0] * shape[1] >= 64:
        assert retried, "no content of this shape had two components: the capacity retry never ran"


PAIRS = [(10, 30), (10, 10), (200, 255), (37, 90), (36, 90), (37, 37), (0, 0), (0, 600), (120, 121), (64, 200), (65, 66), (10, 255)]


def oracle_scores(gray, nm, pairs):
    """the inputs of the oracle's edge_quality, recomputed from cv_canny: (edge components, edge pixels, sum and sum of squares of gray)"""
    from scipy import ndimage
    from oracle import rhccq_oracle as O
    out = []
    for lo, hi in pairs:
        e = O.cv_canny(gray, lo, hi, nm) > 0
        v = gray[e].astype(np.int64)
        out.append((int(ndimage.label(e, structure=np.ones((3, 3)))[1]), int(e.sum()), int(v.sum()), int((v * v).sum())))
    return out


@shapes
def test_edge_front_end_on_shape(shape):
    """EdgeAnalysis on a photo, a poster and a noise frame: gray and its histogram, the non-maximum suppression for gray and colour
    input, Canny for five threshold pairs, the thresholds of every method, and the score tuples nested == scratch == the oracle's"""
    from oracle import rhccq_oracle as O
    from encoder.ROI import edges as E
    from roibasedimagecompression_amd.api.edges import EdgeAnalysis
    rh, up = _ctx()
    seen = Varied()
    for cname, img in image_contents(*shape):
        a = EdgeAnalysis(img, rh)
        gray = O.cv_rgb2gray(img)
        seen.note("gray", gray)
        same(a.gray.cpu().numpy(), gray, (cname, "gray"))
        assert np.array_equal(a.hist, np.bincount(gray.ravel(), minlength=256)), cname
        for colour, src in ((False, gray), (True, img)):
            nm = O.cv_canny_nms(src)
            seen.note(f"nm{colour}", nm)
            same(a.nm(colour).cpu().numpy().view(np.uint16), nm, (cname, "nm", colour))
            for lo, hi in ((10, 40), (50, 150), (120.7, 60.2), (0, 0), (300, 400)):
                want = O.cv_canny(src, lo, hi, nm)
                seen.note(f"canny{colour}", want)
                same(a.canny(lo, hi, colour).cpu().numpy(), want, (cname, "canny", colour, lo, hi))
        for method in ("otsu", "percentile", "gradient", "hybrid", "other"):
            for sens in (0.5, 0.7, 1.0, 1.3, 1.5):
                assert a.thresholds(method, sens) == O.adaptive_canny_thresholds(gray, method, sens), (cname, method, sens)
        want = oracle_scores(gray, O.cv_canny_nms(gray), PAIRS)
        nested = a.rh.canny_scores(a.nm(False), a.gray, PAIRS, nested=True)
        scratch = a.rh.canny_scores(a.nm(False), a.gray, PAIRS, nested=False)
        assert nested == scratch == want, (cname, nested, scratch, want)
        same(E.get_edge_map_fast(img), O.get_edge_map_fast(img), (cname, "get_edge_map_fast"))
    seen.check(shape, ["gray", "nmFalse", "nmTrue", "cannyFalse", "cannyTrue"])


def device_chain_steps():
    from encoder.ROI.thin_regions2 import remove_thin_structures_optimized as thin_rm, identify_thin_regions_ultrafast as thin
    from encoder.ROI.small_regions import remove_small_regions, connect_by_closing_fast
    from encoder.ROI.small_gaps import bridge_small_gaps_fast
    from encoder.ROI.roi import (remove_small_noise_regions as noise, detect_meaningful_borders, protect_border_regions, fill_closed_regions,
                                 remove_small_components_density_aware_fast as aware)
    from encoder.ROI.edges import compute_local_density
    from oracle import rhccq_oracle as O
    s = {"thin": thin, "thin_3_0.6": lambda m: thin(m, 3, 0.6)}
    for thr in (0.10, 0.25):
        s[f"remove_thin_{thr}"] = lambda m, thr=thr: thin_rm(m, thr, 0.3, 25, 25)
    for win in (11, 5, 25):
        s[f"remove_thin_win{win}"] = lambda m, win=win: thin_rm(m, 0.3, 0.3, win)
        s[f"noise_30_win{win}"] = lambda m, win=win: noise(m, 30, 0.3, win)
    s["remove_thin_conn4"] = lambda m: thin_rm(m, 0.3, connectivity=4)
    for ms, thr in ((75, 0.2), (12, 0.4)):
        s[f"noise_{ms}"] = lambda m, ms=ms, thr=thr: noise(m, min_size=ms, density_threshold=thr)
    for win in (15, 7):
        s[f"density_aware_{win}"] = lambda m, win=win: aware(m, 40, density_map=compute_local_density(m, win), density_threshold=0.3, window_size=win)
    for dist in (5, 2):
        s[f"closing_{dist}"] = lambda m, dist=dist: connect_by_closing_fast(m, dist, 25)
    for gap, win in ((100, 15), (25, 15), (3, 5)):
        s[f"bridge_{gap}"] = lambda m, gap=gap, win=win: bridge_small_gaps_fast(m, gap, 0.2, win, 25)
    for sens in (0.5, 0.7, 1.2):
        s[f"borders_{sens}"] = lambda m, sens=sens: detect_meaningful_borders(m, sens)
    for k in (15, 18, 6):
        s[f"protect_{k}"] = lambda m, k=k: protect_border_regions(m, O.detect_meaningful_borders(m, 0.5), k)
    for conn in (4, 8):
        s[f"fill_{conn}"] = lambda m, conn=conn: fill_closed_regions(m, 10, 10000, conn)
    s["fill_01"] = lambda m: fill_closed_regions((m > 0).astype(np.uint8), 2, 50)
    s["small_5"] = lambda m: remove_small_regions(m, 5, True, 30)
    return s


@shapes
def test_cleanup_functions_on_shape(shape):
    """every clean-up function of test_gpu_roi.py's two clean-up tests with the same argument sets, the unification (both outputs), gap
    bridging on a 0 / 1 / 255 plane and process_and_unify_borders"""
    from oracle import rhccq_oracle as O
    from encoder.ROI.roi import directional_region_unification, process_and_unify_borders
    from encoder.ROI.small_gaps import bridge_small_gaps_fast
    ora, dev = oracle_chain_steps(), device_chain_steps()
    assert set(ora) == set(dev)
    seen = Varied()
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    for cname, m in chain_contents(*shape):
        for step, f in ora.items():
            want = f(m)
            seen.note(step, want)
            same(dev[step](m), want, (cname, step))
        got, want = directional_region_unification(m), O.directional_region_unification(m)
        same(got[0], want[0], (cname, "unify"))
        same(got[1], want[1], (cname, "unify map"))
        mixed = m.copy()
        mixed[::3, ::2] = np.where(mixed[::3, ::2] != 0, 1, 0)
        for win in (11, 25):
            same(bridge_small_gaps_fast(mixed, 6, 0.2, 15, win), O.bridge_small_gaps(mixed, 6, 0.2, 15, win), (cname, "bridge mixed", win))
        dens = O.local_density(m, 3)
        got = process_and_unify_borders(m, dens, img, density_threshold=0.2)
        want = O.process_and_unify_borders(m, dens, img, density_threshold=0.2)
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, (cname, "process_and_unify_borders", i))
    seen.check(shape, MUST_VARY_CHAIN)


def test_unification_varies_on_enough_shapes():
    """directional_region_unification saturates on most small frames: it must vary on at least 5 shapes of the list (oracle side; the
    comparison itself is in test_cleanup_functions_on_shape)"""
    from test_roi_shapes_cpu import unification_varied_shapes
    assert len(unification_varied_shapes()) >= 5


@shapes
def test_extract_roi_nonroi_on_shape(shape):
    from oracle import rhccq_oracle as O
    from encoder.ROI.roi import extract_roi_nonroi
    rng = np.random.default_rng(shape[0] * 1000 + shape[1] + 1)
    img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    seen = Varied()
    for cname, m in chain_contents(*shape):
        region_map = (m != 0).astype(np.uint8)
        for bs in (0, 1, 3, 5):
            got, want = extract_roi_nonroi(img, region_map, bs), O.extract_roi_nonroi(img, region_map, bs)
            assert len(got) == len(want) == 4
            seen.note(f"buffer_{bs}", want[2])
            for i, (g, w) in enumerate(zip(got, want)):
                same(g, w, (cname, bs, i))
    seen.check(shape, ["buffer_1", "buffer_3"])


def _outcome(f, *args):
    try:
        return None, f(*args)
    except Exception as e:                                                        # compared by type below, never swallowed
        return type(e), None


@shapes
def test_chain_entry_points_on_shape(shape):
    """get_edge_map, find_best_edges_by_quality, get_regions: where the oracle raises (UnboundLocalError when no threshold pair yields
    an edge: 1 x 1, flat frames) the device raises the same type; where it returns, equal outputs"""
    from oracle import rhccq_oracle as O
    from encoder.ROI import edges as E
    from encoder.ROI.roi import get_regions
    contents = image_contents(*shape) + [("flat", np.full(shape + (3,), 77, np.uint8))]
    for cname, img in contents:
        for name, dev, ora in (("get_edge_map", E.get_edge_map, O.get_edge_map), ("find_best_edges_by_quality", E.find_best_edges_by_quality,
                                                                                   O.find_best_edges_by_quality), ("get_regions", get_regions, O.get_regions)):
            werr, want = _outcome(ora, img)
            gerr, got = _outcome(dev, img)
            assert gerr is werr, (cname, name, gerr, werr)
            if werr is not None:
                continue
            if name == "get_edge_map":
                same(got, want, (cname, name))
            elif name == "find_best_edges_by_quality":
                assert tuple(got[1:]) == tuple(want[1:]), (cname, name, got[1:], want[1:])
                same(got[0], want[0], (cname, name))
            else:
                assert len(got) == len(want) == 6
                for i, (g, w) in enumerate(zip(got, want)):
                    same(g, w, (cname, name, i))
    assert _outcome(O.get_edge_map, contents[-1][1])[0] is UnboundLocalError                 # the raising branch is really taken
