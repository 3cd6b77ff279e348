"""The ROI stage against the CPU oracle at 2160 x 3840: the size the benchmark quotes, where thousands of workgroups run the union-find
at once, the capacity retries of Rhccq.ccl and the CANNY_SCORES_CAP fallback fire, the fixed-size LDS tables overflow, the 16-bit
prefix counts / distances / box counts approach their ranges and the chamfer row loop runs thousands of rows deep.  GPU only.

One module-scoped fixture holds the frames (tests/test_roi_shapes_cpu.py fullsize_frames: the plain photo and a mosaic of photo and
poster tiles) and runs each oracle entry point once, on first use; the tests share its results.  The tests are dominated by the
single-threaded oracle; each docstring gives the oracle and device seconds measured on an MI355X host (the whole file: 149 s)."""
import time

import numpy as np
import pytest

from test_gpu_roi_shapes import oracle_scores, same
from test_roi_shapes_cpu import FULL_H, FULL_W, _u8, assert_both_classes, fullsize_frames, oracle_regions_from_edge_map

pytestmark = pytest.mark.gpu
FRAMES = ("photo", "mosaic")
H, W = FULL_H, FULL_W


class Clock:
    """oracle / device seconds of one test, printed (pytest -s shows them; the docstrings record a run)"""

    def __init__(self):
        self.t = {"oracle": 0.0, "device": 0.0}

    def run(self, side, f, *a, **k):
        import torch
        t0 = time.perf_counter()
        out = f(*a, **k)
        if side == "device":
            torch.cuda.synchronize()
        self.t[side] += time.perf_counter() - t0
        return out

    def report(self, name):
        print(f"\n[time] {name}: oracle {self.t['oracle']:.1f} s, device {self.t['device']:.2f} s", flush=True)


class _Full:
    def __init__(self):
        self.frames = fullsize_frames()
        self._cache = {}
        self.oracle_seconds = {}

    def get(self, key, f):
        if key not in self._cache:
            t0 = time.perf_counter()
            self._cache[key] = f()
            self.oracle_seconds[key] = time.perf_counter() - t0
            print(f"\n[time] oracle {key}: {self.oracle_seconds[key]:.1f} s", flush=True)
        return self._cache[key]

    def best(self, name):
        from oracle import rhccq_oracle as O
        return self.get(("best", name), lambda: O.find_best_edges_by_quality(self.frames[name]))

    def edge_map(self, name):
        """O.get_edge_map: the winner of find_best_edges_by_quality applied to the colour image (its two lines, the search shared)"""
        from oracle import rhccq_oracle as O
        _, lo, hi, _ = self.best(name)
        return self.get(("edge_map", name), lambda: O.cv_canny(self.frames[name], lo, hi))

    def regions(self, name):
        em = self.edge_map(name)
        return self.get(("regions", name), lambda: oracle_regions_from_edge_map(self.frames[name], em))


@pytest.fixture(scope="module")
def full():
    return _Full()


def _up(a):
    import torch
    from roibasedimagecompression_amd.ops import default_context
    return torch.from_numpy(np.ascontiguousarray(a)).to(default_context().device)


@pytest.mark.parametrize("name", FRAMES)
def test_edge_map_and_threshold_scores_fullsize(full, name):
    """get_edge_map and find_best_edges_by_quality (low, high, method, the edge image) == oracle, and the score tuples of all 20
    threshold pairs: nested == scratch == two-step == recomputed from the oracle's cv_canny.
    Measured: photo oracle 9.0 s (search 6.2, colour Canny 0.9, scores 1.9) / device 0.26 s; mosaic oracle 7.4 s / device 0.30 s."""
    from oracle import rhccq_oracle as O
    from encoder.ROI import edges as E
    from roibasedimagecompression_amd.api.edges import EdgeAnalysis
    img, c = full.frames[name], Clock()
    want = full.best(name)
    got = c.run("device", E.find_best_edges_by_quality, img)
    assert tuple(got[1:]) == tuple(want[1:]), (got[1:], want[1:])
    same(got[0], want[0], "best edges")
    same(c.run("device", E.get_edge_map, img), full.edge_map(name), "get_edge_map")
    gray = O.cv_rgb2gray(img)
    pairs = sorted({O.adaptive_canny_thresholds(gray, m, s) for m in ("otsu", "percentile", "gradient", "hybrid") for s in (0.5, 0.7, 1.0, 1.3, 1.5)})
    ref = c.run("oracle", oracle_scores, gray, O.cv_canny_nms(gray), pairs)
    a = EdgeAnalysis(img)
    assert [a.thresholds(m, s) for m in ("otsu", "hybrid") for s in (0.5, 1.5)] == [O.adaptive_canny_thresholds(gray, m, s) for m in ("otsu", "hybrid") for s in (0.5, 1.5)]
    nested = c.run("device", a.rh.canny_scores, a.nm(False), a.gray, pairs, nested=True)
    scratch = c.run("device", a.rh.canny_scores, a.nm(False), a.gray, pairs, nested=False)
    two_step = c.run("device", lambda: [a.rh.canny_components(a.nm(False), lo, hi, a.gray)[2] for lo, hi in pairs])
    assert nested == scratch == two_step == ref, (nested, scratch, two_step, ref)
    assert max(r[0] for r in ref) > 1000                                   # thousands of components: the union-find has real work
    c.report(f"edge map and scores, {name}")


@pytest.mark.parametrize("name", FRAMES)
def test_get_regions_fullsize(full, name):
    """get_regions == oracle on all six outputs, each set on 5 % .. 95 % of the frame (asserted from the oracle's), then
    extract_regions' areas and bounding boxes against the oracle's component statistics and its minimum-size rule.
    Measured: photo oracle 15.3 s / device 0.17 s; mosaic oracle 14.6 s / device 0.03 s (the edge map comes from the fixture)."""
    from oracle import rhccq_oracle as O
    from encoder.ROI.roi import get_regions, extract_regions
    img, c = full.frames[name], Clock()
    want = full.regions(name)
    assert_both_classes(name, want)
    got = c.run("device", get_regions, img)
    assert len(got) == len(want) == 6
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, (name, i))
    roi, non = c.run("device", extract_regions, img, got[4], got[5])

    def boxes(mask):
        num, _, stats = O.cv_connected_components_with_stats(np.asarray(mask).astype(np.uint8), 8)
        return [((int(y), int(x), int(y + h), int(x + w)), int(area)) for x, y, w, h, area in stats[1:]]
    wroi, wnon = c.run("oracle", boxes, want[4]), c.run("oracle", boxes, want[5])
    mn = O.roi_min_region_size(img)
    wnon = wnon + [r for r in wroi if r[1] < mn]
    wroi = [r for r in wroi if r[1] >= mn]
    assert [(tuple(r["bbox"]), r["area"]) for r in roi] == wroi and [(tuple(r["bbox"]), r["area"]) for r in non] == wnon
    assert len(wroi) >= 1 and len(wnon) >= 1
    c.report(f"get_regions, {name}")


def test_capacity_paths_fullsize():
    """A 4K noise frame whose Canny map has more than 1 << 16 components (count taken from the oracle): both retries of Rhccq.ccl fire
    through the API (cap 1 << 16 in evaluate_edge_quality, 1 << 14 in the clean-up chain's components) and the labelling, the
    statistics, the quality score and two clean-up steps equal the oracle's.  The fused scoring's fallback: 4K does not reach
    CANNY_SCORES_CAP = 1 << 20 components at a cost the oracle can score, so the cap is lowered to 1000 on this test's own Rhccq
    instance; the device's returned component counts (all above the cap) show the two-step path was taken.
    Measured: oracle 3.1 s, device 0.09 s."""
    from scipy import ndimage
    from oracle import rhccq_oracle as O
    from encoder.ROI import edges as E
    from encoder.ROI.roi import fill_closed_regions
    from encoder.ROI.small_regions import remove_small_regions
    from roibasedimagecompression_amd.ops import Rhccq
    c = Clock()
    rng = np.random.default_rng(4)
    gray = rng.integers(0, 256, (H, W), dtype=np.uint8)
    nm = O.cv_canny_nms(gray)
    edges = c.run("oracle", O.cv_canny, gray, 300, 500, nm)
    n_ref = int(ndimage.label(edges > 0, structure=np.ones((3, 3)))[1])
    assert n_ref > 1 << 16, n_ref
    rh = Rhccq(0)
    for cap in (1 << 14, 1 << 16):
        n, lab, stats = c.run("device", rh.ccl, _up(edges), 8, cap=cap)
        assert n == n_ref > cap                                               # the first call overflowed `cap`: the retry ran
        if cap == 1 << 14:
            num, wlab, wstats = c.run("oracle", O.cv_connected_components_with_stats, edges, 8)
            same(lab.cpu().numpy(), wlab, "labels")
            same(stats, wstats, "stats")
    s_dev, s_ref = c.run("device", E.evaluate_edge_quality, edges, gray), c.run("oracle", O.edge_quality, edges, gray)
    assert abs(s_dev - s_ref) <= 1e-9 * abs(s_ref), (s_dev, s_ref)
    same(c.run("device", remove_small_regions, edges, 5, True, 30), c.run("oracle", O.remove_small_regions, edges, 5), "remove_small_regions")
    same(c.run("device", fill_closed_regions, edges, 10, 10000, 4), c.run("oracle", O.fill_closed_regions, edges, 10, 10000, 4), "fill_closed_regions")
    pairs = [(300, 500), (300, 700), (400, 600)]
    ref = c.run("oracle", oracle_scores, gray, nm, pairs)
    assert min(r[0] for r in ref) > 1000
    rh.CANNY_SCORES_CAP = 1000                                                 # this instance only
    g, n16 = _up(gray), _up(nm.view(np.int16))
    low = c.run("device", rh.canny_scores, n16, g, pairs, nested=False)
    assert low == ref == c.run("device", rh.canny_scores, n16, g, pairs, nested=True), (low, ref)
    # the per-labelling component counts the fused call returns (column 4) exceed the lowered cap: canny_scores took the fallback
    for lo, _ in pairs:
        assert rh.canny_label(n16, lo, g)[0] > rh.CANNY_SCORES_CAP
    c.report("capacity paths")


ELEMENTS = (("rect15", [7] * 15), ("rect31", [15] * 31), ("ell11", [0, 3, 4, 5, 5, 5, 5, 5, 4, 3, 0]))


@pytest.mark.parametrize("which", ["edge_map", "roi_mask"])
def test_primitives_fullsize(full, which):
    """On the oracle's 4K edge map and on its ROI mask (photo frame): dilate / erode / close with [7] * 15, [15] * 31 and the 11-ellipse,
    the chamfer distance, box counts 3 and 31, label_sum, local density 7 and 15, gap bridging, borders, fill, thin regions.
    Measured: edge map oracle 18.5 s / device 0.14 s; ROI mask oracle 27.9 s / device 0.11 s."""
    from oracle import rhccq_oracle as O
    from encoder.ROI.edges import compute_local_density
    from encoder.ROI.roi import detect_meaningful_borders, fill_closed_regions
    from encoder.ROI.small_gaps import bridge_small_gaps_fast
    from encoder.ROI.thin_regions2 import identify_thin_regions_ultrafast
    from roibasedimagecompression_amd.ops import default_context
    rh, c = default_context(), Clock()
    m = full.edge_map("photo") if which == "edge_map" else _u8(full.regions("photo")[4])
    assert 0.02 < (m != 0).mean() < 0.98
    t = _up(m)
    assert O.cv_ellipse_half_widths(11) == ELEMENTS[2][1]
    for ename, hw in ELEMENTS:
        same(c.run("device", lambda: rh.morph(t, hw).cpu().numpy()), _u8(c.run("oracle", O.cv_dilate, m, hw)), (ename, "dilate"))
        same(c.run("device", lambda: rh.morph(t, hw, erode=True).cpu().numpy()), _u8(c.run("oracle", O.cv_erode, m, hw)), (ename, "erode"))
        same(c.run("device", lambda: rh.morph_close(t, hw).cpu().numpy()), _u8(c.run("oracle", O.cv_close, m, hw)), (ename, "close"))
    dist = c.run("oracle", O.cv_dist_chamfer3, m)
    d_dev = c.run("device", rh.dist_chamfer, t)
    same(d_dev.cpu().numpy().astype(np.int64), dist, "chamfer")
    n, lab, stats = c.run("device", rh.ccl, t, 8, cap=1 << 14)
    labels = lab.cpu().numpy()
    same(c.run("device", rh.label_sum, lab, n, d_dev), np.bincount(labels.ravel(), weights=dist.ravel(), minlength=n + 1).astype(np.uint64), "label_sum dist")
    for k in (3, 31):
        cnt = c.run("oracle", O.box_counts, m, k)
        c_dev = c.run("device", rh.box_count, t, k)
        same(c_dev.cpu().numpy().view(np.uint16).astype(np.int64), cnt, ("box_count", k))
        same(c.run("device", rh.label_sum, lab, n, c_dev), np.bincount(labels.ravel(), weights=cnt.ravel(), minlength=n + 1).astype(np.uint64), ("label_sum", k))
    for k in (7, 15):
        same(c.run("device", compute_local_density, m, k), c.run("oracle", O.local_density, m, k), ("density", k))
    same(c.run("device", bridge_small_gaps_fast, m, 25, 0.2, 15, 25), c.run("oracle", O.bridge_small_gaps, m, 25, 0.2, 15, 25), "bridge")
    same(c.run("device", detect_meaningful_borders, m, 0.7), c.run("oracle", O.detect_meaningful_borders, m, 0.7), "borders")
    same(c.run("device", fill_closed_regions, m, 10, 10000, 4), c.run("oracle", O.fill_closed_regions, m, 10, 10000, 4), "fill")
    same(c.run("device", identify_thin_regions_ultrafast, m), c.run("oracle", O.identify_thin_regions, m), "thin")
    c.report(f"primitives, {which}")


def test_adversarial_masks_fullsize():
    """The long loops and the 16-bit ranges: all set but one corner pixel (the chamfer loop walks every row; against the closed form
    a * (max - min) + b * min of (y, x) as well as the oracle), all set (OpenCV's DIST_MAX everywhere; prefix counts and box counts at
    their maxima) and a single set column at x = 3839.
    Measured: oracle 31.8 s, device 0.08 s."""
    from oracle import rhccq_oracle as O
    from roibasedimagecompression_amd.ops import default_context
    rh, c = default_context(), Clock()
    corner = np.full((H, W), 255, np.uint8)
    corner[0, 0] = 0
    yy, xx = np.mgrid[0:H, 0:W]
    closed_form = 62587 * np.abs(yy - xx).astype(np.int64) + 89738 * np.minimum(yy, xx).astype(np.int64)
    assert closed_form.max() < (2 ** 31 - 1) >> 2
    got = c.run("device", lambda: rh.dist_chamfer(_up(corner)).cpu().numpy())
    assert got.dtype == np.int32
    same(got.astype(np.int64), closed_form, "corner chamfer, closed form")
    same(got.astype(np.int64), c.run("oracle", O.cv_dist_chamfer3, corner), "corner chamfer, oracle")
    full_set = np.full((H, W), 255, np.uint8)
    assert (c.run("device", lambda: rh.dist_chamfer(_up(full_set)).cpu().numpy()) == (2 ** 31 - 1) >> 2).all()
    column = np.zeros((H, W), np.uint8)
    column[:, W - 1] = 255
    for mname, m in (("corner", corner), ("all set", full_set), ("column", column)):
        t = _up(m)
        for k in (3, 31):
            same(c.run("device", lambda: rh.box_count(t, k).cpu().numpy().view(np.uint16).astype(np.int64)), c.run("oracle", O.box_counts, m, k), (mname, "box", k))
        for hw in ([15] * 31, [1] * 3):
            same(c.run("device", lambda: rh.morph(t, hw).cpu().numpy()), _u8(c.run("oracle", O.cv_dilate, m, hw)), (mname, "dilate", len(hw)))
            same(c.run("device", lambda: rh.morph(t, hw, erode=True).cpu().numpy()), _u8(c.run("oracle", O.cv_erode, m, hw)), (mname, "erode", len(hw)))
    same(c.run("device", lambda: rh.dist_chamfer(_up(column)).cpu().numpy().astype(np.int64)), c.run("oracle", O.cv_dist_chamfer3, column), "column chamfer")
    c.report("adversarial masks")


def test_quality_metrics_and_split_score_fullsize():
    """calculate_quality_metrics and calculate_adaptive_quality_metrics on a 4K pair with the tolerances of tests/test_gpu_api.py
    (float32 statistics 2e-6 relative, psnr 1e-12, ssim 1e-9 absolute; integers identical): the 64-bit sums had not run past 233 x 40.
    calculate_split_score on the 4K frame with mask=None and with a ragged mask, 1e-9 as test_split_score_vs_oracle.
    Measured: oracle 10.7 s, device 0.35 s.
    Found by this test: the device path took mean / std of the error distribution with numpy's float32 sums over the SORTED multiset of
    25 million values, std 1.9861755 against the oracle's 1.9861636 (exact 1.9861647), 6e-6 relative; api/comparison.py now derives
    both from the exact 256-row table in float64."""
    from decoder.uncompression.comparison import calculate_adaptive_quality_metrics, calculate_quality_metrics
    from encoder.subregions.split_score import calculate_split_score
    from oracle import rhccq_oracle as O
    from roibasedimagecompression_amd import synth
    c = Clock()
    rng = np.random.default_rng(11)
    a = synth.photo(H, W, 5)
    b = np.clip(a.astype(np.int32) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    b[10:20, 5:30] = b[12, 7]
    for _ in range(600):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        b[y, x] = 255 - b[y, x]
    got, want = c.run("device", calculate_quality_metrics, a, b), c.run("oracle", O.quality_metrics, a, b)
    assert set(got) == set(want)
    for k in want:
        assert type(got[k]) is type(want[k]) or k == "ssim", (k, type(got[k]), type(want[k]))
        tol = {"psnr": 1e-12, "ssim": 0.0}.get(k, 2e-6)
        assert abs(float(got[k]) - float(want[k])) <= tol * abs(float(want[k])) + (1e-9 if k == "ssim" else 0.0), (k, got[k], want[k])

    def check(got, want, path=""):
        assert set(got) == set(want), (path, set(got) ^ set(want))
        for k, w in want.items():
            g = got[k]
            if isinstance(w, dict):
                check(g, w, path + k + ".")
            elif isinstance(w, list):
                assert len(g) == len(w) and np.allclose(g, w, rtol=2e-6, atol=1e-9), path + k
                if k == "bins":
                    assert list(g) == list(w)
            elif isinstance(w, str) or isinstance(w, (int, np.integer)) and not isinstance(w, bool):
                assert g == w, (path + k, g, w)
            else:
                assert abs(float(g) - float(w)) <= 2e-6 * abs(float(w)) + 1e-9 or (np.isinf(g) and np.isinf(w)), (path + k, g, w)
    check(c.run("device", calculate_adaptive_quality_metrics, a, b), c.run("oracle", O.adaptive_quality_metrics, a, b))
    m = np.zeros((H, W), bool)
    m[H // 8:H - H // 6, W // 7:W - W // 5] = True
    m &= rng.random((H, W)) > 0.1
    # the raw statistics behind the scores too (the colour score of this photo is clipped to 1.0, which hides its seven sums): what
    # calculate_split_score's own launch returned, by the rule of tests/test_gpu_subregion_shapes.py
    from roibasedimagecompression_amd.ops import default_context
    from test_gpu_subregion_shapes import check_stats
    rh, raw = default_context(), []
    launch = rh.split_stats
    rh.split_stats = lambda *args: raw.append(launch(*args)) or raw[-1]
    try:
        for mask in (None, m):
            got, want = c.run("device", calculate_split_score, a, mask), c.run("oracle", O.split_score, a, mask)
            assert np.allclose(got, want, rtol=0, atol=1e-9), (got, want)
            assert len(raw) == 1
            ratio = check_stats(raw.pop(), c.run("oracle", O.split_stats, a, mask), "4K raw statistics")
            print(f"4K split_stats, mask {'given' if mask is not None else 'None'}: largest error / bound = {ratio:.3g}")
    finally:
        del rh.split_stats
    c.report("metrics and split score")
