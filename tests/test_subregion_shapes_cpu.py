"""The shapes and contents on which tests/test_gpu_subregion_shapes.py compares the sub-region stage (split statistics -> scores,
masked SLIC) with the oracle, the reference side of every comparison, and CPU checks of the oracle itself on them.  The oracle
restates scikit-image (PARITY UNPINNED: absent from the build container), so where scipy or a literal per-pixel loop holds an
independent definition the restatement is pinned to it here, on the same tile-edge and degenerate shapes:

  sk_sobel              scipy.ndimage.convolve with skimage's [1,2,1]/4 x [1,0,-1] kernels, mode="reflect": 1e-14 on the gray plane
                        ([0, 1]) and 1e-14 x 128 on the Lab planes (|L|, |a|, |b| <= 128: the same bound relative to the scale)
  sk_lbp_uniform_8_1    a per-pixel loop over the 8 points (offsets rounded to 5 decimals, bilinear, zero outside), exact
  slic_sweeps           a per-pixel loop over the centroids in ascending order for one sweep, exact
  split_stats           api.split_score.scores_from_stats of its sums == split_score, 1e-9

It also asserts, from the oracle alone, that the comparisons are not vacuous: the LBP and gray histograms spread over several bins,
some content of every >= 100-pixel shape has an UNCLIPPED colour score inside (0, 1), the flat-patch LBP code is 9 for some gray
levels and 8 for others, and the assignment cases hold unassigned masked pixels, exact ties and more than one label."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import rhccq_oracle as O  # noqa: E402

# ---- split statistics: tile 32 x 8 with a 1-pixel halo (csrc/split_score.hip kSsTW, kSsTH) ---------------------------------------
HEIGHTS = (1, 2, 7, 8, 9, 15, 16, 17)
WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65)
SPLIT_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 65), (17, 1), (17, 65),                                  # corners
                (7, 31), (8, 32), (9, 33), (15, 63), (16, 64), (7, 33), (9, 31), (15, 65), (17, 63),       # one under / exact / one over
                (8, 31), (8, 33), (7, 32), (9, 32), (16, 63), (16, 65), (15, 64), (17, 64),
                (1, 31), (1, 32), (1, 33), (1, 63), (1, 64), (7, 1), (8, 1), (9, 2), (15, 2), (16, 1), (2, 31), (2, 33), (2, 64), (2, 65)]
SCORE_SHAPES = [(8, 32), (9, 33), (17, 65), (2, 64), (1, 128), (128, 1)]                                    # >= 100 pixels
ALL_SPLIT_SHAPES = SPLIT_SHAPES + [s for s in SCORE_SHAPES if s not in SPLIT_SHAPES]
assert len(set(SPLIT_SHAPES)) == len(SPLIT_SHAPES) >= 30
assert {h for h, w in SPLIT_SHAPES} >= set(HEIGHTS) and {w for h, w in SPLIT_SHAPES} >= set(WIDTHS)
SEAM_COLS, SEAM_ROWS = ((31, 63), (32, 64)), ((7, 15), (8, 16))             # (left / upper side of each seam, right / lower side)

# ---- SLIC: workgroup 256 pixels, update chunk 64 x 8 = 512 pixels, 4 centroids per workgroup (csrc/slic.hip) ---------------------
SLIC_SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (257, 1), (16, 16), (2, 128), (23, 11), (3, 171), (1, 511), (16, 32), (19, 27), (32, 33)]
SLIC_K = (1, 2, 3, 4, 5, 255, 256, 257)
K_LDS_MAX = 1097                                                            # 56 bytes per centroid, 60 KB
assert K_LDS_MAX * 56 <= 60 * 1024 < (K_LDS_MAX + 1) * 56

RESIZE_SHAPES = [((5, 2000), (1, 500)), ((2000, 5), (500, 1)), ((3, 1200), (1, 480)), ((2, 900), (1, 540)), ((1, 700), (1, 490)),
                 ((700, 1), (490, 1)), ((4, 1000), (2, 500)), ((1, 1), (1, 1))]
SLIC_REGIONS = [(1, 1, 1), (1, 40, 3), (40, 1, 3), (2, 2, 1), (3, 171, 4), (16, 16, 5), (23, 11, 2), (1, 257, 7), (5, 2000, 6), (9, 33, 300),
                (30, 30, 900)]
SLIC_RAISING = (1, 600, 3)                                                  # the downscale to 0 rows


def ids(shapes):
    return [f"{h}x{w}" for h, w in shapes]


def _seed(h, w, salt=0):
    return 100003 * h + 17 * w + salt


# ---- contents ---------------------------------------------------------------------------------------------------------------------
def split_images(h, w):
    """photo / poster / noise as test_roi_shapes_cpu.image_contents, two low-contrast photos (their colour scores stay below the clip;
    the 2 x 64 photo is two unlike rows and needs the lower one), a photo with near-black pixels (mask=None drops them) and bright one-pixel lines on either side of every tile seam"""
    from roibasedimagecompression_amd import synth
    rng = np.random.default_rng(_seed(h, w, 7))
    photo = synth.photo(h, w, _seed(h, w, 1), sigma=3.0)
    dark = photo.copy()
    dark[rng.random((h, w)) < 0.3] = (2, 1, 3)                                  # gray 0.0055: below the 0.01 of mask=None
    out = [("photo", photo), ("poster", synth.poster(h, w, _seed(h, w, 2))), ("noise", rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
           ("low", (photo // 8 + 100).astype(np.uint8)), ("lower", (photo // 16 + 100).astype(np.uint8)), ("dark", dark)]
    for side in (0, 1):
        img = (photo // 4 + 20).astype(np.uint8)
        for x in SEAM_COLS[side]:
            if x < w:
                img[:, x] = (250, 40, 10 + 100 * side)
        for y in SEAM_ROWS[side]:
            if y < h:
                img[y, :] = (30, 240, 200 - 100 * side)
        out.append((f"seam{side}", img))
    return out


def split_masks(h, w):
    """all set, ragged random masks of density 0.9 / 0.5, a disc, one-pixel lines on either side of every tile seam; None = the
    function's own gray > 0.01"""
    rng = np.random.default_rng(_seed(h, w, 3))
    yy, xx = np.mgrid[0:h, 0:w]
    out = [("none", None), ("all", np.ones((h, w), bool)), ("rand0.9", rng.random((h, w)) < 0.9), ("rand0.5", rng.random((h, w)) < 0.5),
           ("disc", ((yy - (h - 1) / 2) / (h / 2 + 0.5)) ** 2 + ((xx - (w - 1) / 2) / (w / 2 + 0.5)) ** 2 <= 1)]
    for side in (0, 1):
        lines = np.zeros((h, w), bool)
        for x in SEAM_COLS[side]:
            lines[:, x:x + 1] = True
        for y in SEAM_ROWS[side]:
            lines[y:y + 1, :] = True
        lines[h - 1 if side else 0, :] = True
        lines[:, 0 if side else w - 1] = True
        out.append((f"seam{side}", lines))
    return out


def score_mask(h, w, n):
    """a ragged mask of exactly n pixels"""
    m = np.zeros(h * w, bool)
    m[np.random.default_rng(_seed(h, w, n)).permutation(h * w)[:n]] = True
    return m.reshape(h, w)


def stats_tolerance(ref):
    """test 1's bound per sum: 1e-9 x max(count, sum of |term|)"""
    sums, _, _, abs_sums = ref
    return 1e-9 * np.maximum(sums[0], abs_sums)


def unclipped_colour_score(sums):
    n = sums[0]
    std = [np.sqrt(max(sums[2 + 2 * c] / n - (sums[1 + 2 * c] / n) ** 2, 0.0)) for c in range(3)]
    return 0.7 * (std[0] / 100 + std[1] / 128 + std[2] / 128) / 3 + 0.3 * (sums[7] / n) / 3


def outcome(f, *args, **kw):
    """("ok", value) or ("raised", exception type): where the oracle raises, the device must raise the same type"""
    try:
        return "ok", f(*args, **kw)
    except Exception as e:      # noqa: BLE001
        return "raised", type(e)


# ---- the LBP rounding probe ---------------------------------------------------------------------------------------------------------
def lbp_probe_frames():
    """80 x 80 frames of 256 flat 5 x 5 blocks: block v at gray level v; the same layout with 256 random flat colours; the mask of the
    3 x 3 block interiors (their 8 sample points lie inside the block)"""
    rng = np.random.default_rng(256)
    v = np.kron(np.arange(256).reshape(16, 16), np.ones((5, 5), int))
    gray = np.repeat(v[..., None], 3, axis=-1).astype(np.uint8)
    colour = rng.integers(0, 256, (256, 3), dtype=np.uint8)[v]
    inner = np.zeros((5, 5), bool)
    inner[1:4, 1:4] = True
    return gray, colour, np.kron(np.ones((16, 16), bool), inner).astype(bool)


def flat_level(v):
    return np.full((9, 33, 3), v, np.uint8)


@functools.lru_cache(None)
def flat_levels_with_code_9():
    return tuple(v for v in range(256) if (O.sk_lbp_uniform_8_1(O.sk_rgb2gray(flat_level(v)))[1:-1, 1:-1] == 9).any())


# ---- independent definitions --------------------------------------------------------------------------------------------------------
def literal_lbp(gray):
    """skimage.feature.local_binary_pattern(gray, 8, 1, "uniform") pixel by pixel, from its published definition: point p at offset
    (-sin, cos)(2 pi p / 8) rounded to 5 decimals, bilinear interpolation between the four surrounding pixels (floor / ceil of the
    offset, weights = the offset's fractional part) with zeros outside the image, bit = sample - centre >= 0; at most two 0 / 1
    transitions around the circle -> the number of ones, else 9"""
    H, W = gray.shape
    pts = []
    for p in range(8):
        rp, cp = float(np.round(-np.sin(2 * np.pi * p / 8), 5)), float(np.round(np.cos(2 * np.pi * p / 8), 5))
        r0, c0, r1, c1 = int(np.floor(rp)), int(np.floor(cp)), int(np.ceil(rp)), int(np.ceil(cp))
        pts.append((r0, c0, r1, c1, rp - r0, cp - c0))
    gray = gray.tolist()

    def get(y, x):
        return gray[y][x] if 0 <= y < H and 0 <= x < W else 0.0
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            bits = []
            for r0, c0, r1, c1, dr, dc in pts:
                top = (1 - dc) * get(y + r0, x + c0) + dc * get(y + r0, x + c1)
                bottom = (1 - dc) * get(y + r1, x + c0) + dc * get(y + r1, x + c1)
                bits.append(1 if ((1 - dr) * top + dr * bottom) - gray[y][x] >= 0 else 0)
            changes = sum(bits[i] != bits[(i + 1) % 8] for i in range(8))
            out[y, x] = sum(bits) if changes <= 2 else 9
    return out


def literal_assign(img, mask, seg, step, ignore_color):
    """One assignment sweep of skimage's _slic_cython, pixel by pixel: every masked pixel goes over the centroids in ascending order,
    skips those whose window [c - 2 step, c + 2 step + 1) (clipped to the image, truncated to int) does not hold it and those
    holding a NaN (they compare smaller than nothing), and takes a centroid whose distance is STRICTLY smaller than the best so far.
    -> (labels int32 [H][W], masked pixels left at 0, pixels whose two smallest distances are equal)"""
    H, W = mask.shape
    inv = 1.0 / (step * step)
    seg = [[float(v) for v in row] for row in seg]
    wins = []
    for cy, cx, *_ in seg:
        if cy != cy or cx != cx:
            wins.append(None)
            continue
        wins.append((int(max(cy - 2 * step, 0)), int(min(cy + 2 * step + 1, H)), int(max(cx - 2 * step, 0)), int(min(cx + 2 * step + 1, W))))
    labels = np.zeros((H, W), np.int32)
    unassigned = ties = 0
    pix = img.tolist()
    for y in range(H):
        for x in range(W):
            if not mask[y, x]:
                continue
            best, bd, tied = 0, float(np.finfo(np.float64).max), False
            for k, (s, win) in enumerate(zip(seg, wins)):
                if win is None or not (win[0] <= y < win[1] and win[2] <= x < win[3]):
                    continue
                dy, dx = s[0] - y, s[1] - x
                d = (dy * dy + dx * dx) * inv
                if not ignore_color:
                    dc = 0.0
                    for c in range(3):
                        e = pix[y][x][c] - s[2 + c]
                        dc = dc + e * e
                    d = d + dc
                if bd > d:                                                  # (false for a NaN distance)
                    best, bd, tied = k + 1, d, False
                elif d == bd:
                    tied = True
            labels[y, x] = best
            unassigned += best == 0
            ties += tied
    return labels, int(unassigned), int(ties)


# ---- the assignment cases -------------------------------------------------------------------------------------------------------------
def _slic_mask(kind, h, w, rng):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 0:
        return np.ones((h, w), bool)
    if kind == 3:
        return ((yy - (h - 1) / 2) / (h / 2 + 0.5)) ** 2 + ((xx - (w - 1) / 2) / (w / 2 + 0.5)) ** 2 <= 1
    return rng.random((h, w)) < (0.9 if kind == 1 else 0.5)


def _slic_image(h, w, rng):
    """a float64 image on the scale of Lab / compactness, with repeated values so that colour distances can tie"""
    return np.round(rng.normal(0, 3, (h, w, 3)) * 4) / 4


@functools.lru_cache(None)
def assign_cases():
    """[(name, img float64[H][W][3], mask bool[H][W], seg float64[K][5], step)]: every SLIC shape with K = 1..5 and one of 255 / 256 /
    257 (all three on 16 x 32), centroids at integer and fractional positions inside and up to 2 pixels beyond the image, steps that
    are natural (sqrt(HW / K)), fractional, tiny (most pixels outside every window) and huge (max(H, W)); then the chosen cases: exact
    ties, duplicated centroids, centroids outside the mask and beyond the border, a NaN row, the largest K the LDS check admits"""
    cases = []
    for si, (h, w) in enumerate(SLIC_SHAPES):
        ks = list(SLIC_K[:5]) + ([255, 256, 257] if (h, w) == (16, 32) else [SLIC_K[5 + si % 3]])
        for ki, K in enumerate(ks):
            rng = np.random.default_rng(_seed(h, w, 1000 + K))
            seg = np.concatenate([rng.uniform(-2, h + 2, (K, 1)), rng.uniform(-2, w + 2, (K, 1)), rng.normal(0, 3, (K, 3))], axis=1)
            seg[::2, :2] = np.floor(seg[::2, :2])                           # every other centroid on the pixel grid
            seg[::3, 2:] = np.round(seg[::3, 2:] * 4) / 4
            step = (max(np.sqrt(h * w / K), 1.0), 2.5, 0.3, float(max(h, w)), 1.37)[(si + ki) % 5]
            img, mask = _slic_image(h, w, rng), _slic_mask((si + ki) % 4, h, w, rng)
            mask[0, 0] = mask[h - 1, w - 1] = True
            if K == 1:
                step = float(max(h, w))                                     # what _get_mask_centroids gives for one centroid
                seg[0, :2] = ((h - 1) / 2, (w - 1) / 2)
            elif h * w > 1:                                                 # two centroids ON masked pixels, so that no map is constant
                ys, xs = np.nonzero(mask)
                for k, j in ((0, len(ys) // 3), (1, len(ys) - 1 - len(ys) // 4)):
                    seg[k] = (ys[j], xs[j], *img[ys[j], xs[j]])
            cases.append((f"{h}x{w}_K{K}_step{step:.3g}", img, mask, seg, float(step)))
    rng = np.random.default_rng(5)
    flat = np.zeros((9, 9, 3))
    full = np.ones((9, 9), bool)
    tie = np.array([[4, 2, 0, 0, 0], [4, 6, 0, 0, 0], [0, 4, 0, 0, 0], [8, 4, 0, 0, 0]], float)     # (4, 4): equal to all four, takes the first
    cases.append(("tie_9x9", flat, full, tie, 4.0))
    cases.append(("tie_colour_9x9", _slic_image(9, 9, rng), full, np.array([[4, 2, 1, -2, .5], [4, 6, 1, -2, .5]], float), 3.0))
    img = _slic_image(16, 16, rng)
    dup = np.array([[5, 5, 1, 1, 1], [5, 5, 1, 1, 1], [11.5, 9.25, 0, 0, 0], [11.5, 9.25, 0, 0, 0], [5, 5, 1, 1, 1]], float)
    cases.append(("duplicates_16x16", img, full_mask(16, 16), dup, 4.0))
    disc = _slic_mask(3, 23, 11, rng)
    corners = np.array([[0, 0, 0, 0, 0], [22, 10, 1, 0, 0], [0, 10, 0, 1, 0], [22, 0, 0, 0, 1], [11, 5, 0, 0, 0]], float)
    assert not disc[0, 0] and not disc[22, 10]
    cases.append(("outside_mask_23x11", _slic_image(23, 11, rng), disc, corners, 5.5))
    beyond = np.array([[-3, -3, 0, 0, 0], [16, 32, 0, 0, 0], [21, 2, 0, 0, 0], [-0.5, 31.5, 0, 0, 0], [15, 31, 0, 0, 0], [8, -40, 0, 0, 0],
                       [7.5, 16, 1, 1, 1]], float)
    cases.append(("beyond_border_16x32", _slic_image(16, 32, rng), _slic_mask(1, 16, 32, rng), beyond, 2.0))
    cases.append(("beyond_border_big_step_16x32", _slic_image(16, 32, rng), full_mask(16, 32), beyond, 32.0))
    cases.append(("tiny_step_19x27", _slic_image(19, 27, rng), full_mask(19, 27),
                  np.concatenate([rng.uniform(0, 19, (40, 1)), rng.uniform(0, 27, (40, 1)), rng.normal(0, 3, (40, 3))], axis=1), 0.2))
    nan = np.array([[4, 4, 0, 0, 0], [np.nan, 8, 0, 0, 0], [8, 8, 1, 1, 1], [12, 12, np.nan, 0, 0], [3, 13, 0, 0, 0], [np.nan] * 5], float)
    cases.append(("nan_rows_16x16", img, full_mask(16, 16), nan, 4.0))
    seg = np.concatenate([rng.uniform(0, 16, (K_LDS_MAX, 1)), rng.uniform(0, 32, (K_LDS_MAX, 1)), rng.normal(0, 3, (K_LDS_MAX, 3))], axis=1)
    cases.append((f"lds_limit_16x32_K{K_LDS_MAX}", _slic_image(16, 32, rng), _slic_mask(1, 16, 32, rng), seg, 1.5))
    return cases


def full_mask(h, w):
    return np.ones((h, w), bool)


@functools.lru_cache(None)
def assign_reference(i, ignore_color):
    """the literal loop on case i, computed once per session"""
    _, img, mask, seg, step = assign_cases()[i]
    return literal_assign(img, mask, seg, step, ignore_color)


# ---- the regions of the direct rhccq_slic_sweeps_regions call -----------------------------------------------------------------------
SWEEP_REGIONS = [(1, 1, 1), (7, 9, 2), (8, 8, 3), (5, 13, 2), (7, 73, 4), (16, 32, 5), (19, 27, 4), (25, 41, 9), (12, 12, 3), (16, 16, 4),
                 (23, 11, 2)]                                               # (h, w, K): 1, 63, 64, 65, 511, 512, 513, 1025 pixels, ...
SWEEP_NO_WINDOW = 8                                                         # the 12 x 12 region: no masked pixel in any window
SWEEP_ITERS = 10
assert sum(k for _, _, k in SWEEP_REGIONS) % 4 != 0                         # the update's last workgroup is partly empty


@functools.lru_cache(None)
def sweep_regions():
    """[(img float64[H][W][3], mask, seg0 float64[K][5], step)] per region: seeds and step as slic_masked takes them
    (slic_mask_centroids), a smooth image plus noise so that every centroid keeps pixels over all sweeps (a centroid that loses all its
    pixels becomes NaN, on which the oracle raises where the device goes on); region SWEEP_NO_WINDOW has its centroids moved away
    from every masked pixel"""
    out = []
    for r, (h, w, K) in enumerate(SWEEP_REGIONS):
        rng = np.random.default_rng(_seed(h, w, 50 + r))
        mask = full_mask(h, w) if r % 3 == 0 else rng.random((h, w)) < 0.85
        mask[0, 0] = True
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([yy / 7.0 + rng.normal(0, .3, (h, w)), xx / 9.0 + rng.normal(0, .3, (h, w)), rng.normal(0, .5, (h, w))], axis=-1)
        cent, steps = O.slic_mask_centroids(mask[None], K)
        seg = np.concatenate([cent[:, 1:], np.zeros((len(cent), 3))], axis=-1)
        step = float(max(steps))
        if r == SWEEP_NO_WINDOW:
            mask = np.zeros((h, w), bool)
            mask[:3, :] = True
            seg[:, 0], step = (10.0, 11.0, 11.5), 1.5                       # windows start at row 7 or later
        out.append((img, mask, seg, step))
    return out


@functools.lru_cache(None)
def sweep_reference():
    """O.slic_sweeps twice per region (colour ignored, then with colour), as slic_masked runs it -> [(labels, final segments)]"""
    out = []
    for img, mask, seg, step in sweep_regions():
        seg = seg.copy()
        O.slic_sweeps(img, mask, seg, step, SWEEP_ITERS, True)
        labels = O.slic_sweeps(img, mask, seg, step, SWEEP_ITERS, False)
        out.append((labels, seg))
    return out


# ---- whole masked SLIC at degenerate regions ----------------------------------------------------------------------------------------
def slic_region_inputs(ragged):
    """[(img uint8[h][w][3], mask bool[h][w], n_segments)] for SLIC_REGIONS; ragged: density 0.8 with the first pixel kept"""
    from roibasedimagecompression_amd import synth
    out = []
    for h, w, n in SLIC_REGIONS:
        rng = np.random.default_rng(_seed(h, w, 9))
        mask = rng.random((h, w)) < 0.8 if ragged else full_mask(h, w)
        mask[0, 0] = True
        out.append((synth.photo(h, w, _seed(h, w, 4), sigma=3.0), mask, n))
    return out


# ======================================================================================================================================
# CPU tests
# ======================================================================================================================================
@pytest.mark.parametrize("shape", ALL_SPLIT_SHAPES, ids=ids(ALL_SPLIT_SHAPES))
def test_sobel_vs_scipy_convolve(shape):
    from scipy import ndimage as ndi
    K = np.array([[1, 2, 1], [0, 0, 0], [-1, -2, -1]]) / 4.0
    for name, img in split_images(*shape):
        lab = O.sk_rgb2lab(img)
        for pname, plane, tol in [("gray", O.sk_rgb2gray(img), 1e-14)] + [("Lab"[c], lab[..., c], 128e-14) for c in range(3)]:
            h, v = ndi.convolve(plane, K, mode="reflect"), ndi.convolve(plane, K.T, mode="reflect")
            got = O.sk_sobel(plane)
            assert got.shape == plane.shape and np.abs(np.sqrt((h * h + v * v) / 2) - got).max() <= tol, (name, pname)


@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=ids(SPLIT_SHAPES))
def test_lbp_vs_literal_loop(shape):
    contents = split_images(*shape)
    for name, img in contents if shape[0] * shape[1] <= 600 else contents[:3]:
        g = O.sk_rgb2gray(img)
        assert np.array_equal(O.sk_lbp_uniform_8_1(g), literal_lbp(g)), name


def test_lbp_vs_literal_loop_on_flat_levels():
    """the flat-patch code is 8 or 9 by float rounding alone: the loop and the vectorised restatement round alike"""
    for v in range(0, 256, 5):
        g = O.sk_rgb2gray(flat_level(v)[:5, :7])
        assert np.array_equal(O.sk_lbp_uniform_8_1(g), literal_lbp(g)), v


def test_flat_patch_code_depends_on_the_level():
    nine = flat_levels_with_code_9()
    assert 0 < len(nine) < 256
    gray, colour, inner = lbp_probe_frames()
    codes = O.sk_lbp_uniform_8_1(O.sk_rgb2gray(gray))
    assert set(np.unique(codes[inner])) == {8, 9}
    blocks = codes.reshape(16, 5, 16, 5).transpose(0, 2, 1, 3).reshape(256, 5, 5)[:, 1:4, 1:4]
    assert all((b == b[0, 0]).all() for b in blocks)                          # one code per flat block
    assert tuple(int(v) for v in np.nonzero(blocks[:, 0, 0] == 9)[0]) == nine  # and the one the level gives alone
    ccodes = O.sk_lbp_uniform_8_1(O.sk_rgb2gray(colour))[inner]
    assert set(np.unique(ccodes)) == {8, 9}
    lbp = O.split_stats(gray, inner)[1]
    assert lbp[9] == 9 * len(nine) and lbp[8] == 9 * (256 - len(nine)) and lbp.sum() == 9 * 256


@pytest.mark.parametrize("shape", SCORE_SHAPES, ids=ids(SCORE_SHAPES))
def test_scores_from_oracle_stats_equal_split_score(shape):
    from roibasedimagecompression_amd.api.split_score import scores_from_stats
    unclipped = []
    for iname, img in split_images(*shape):
        for mname, m in split_masks(*shape):
            ref = O.split_stats(img, m)
            if ref[0][0] < 100:
                assert O.split_score(img, m) == (0.0, 0.0, 0.0)
                continue
            got, want = scores_from_stats(*ref[:3]), O.split_score(img, m)
            assert np.allclose(got, want, rtol=0, atol=1e-9), (iname, mname, got, want)
            unclipped.append(unclipped_colour_score(ref[0]))
    # not vacuous: some content's colour score is not clipped, so that it depends on the seven Lab / gradient sums
    assert any(0.0 < u < 1.0 for u in unclipped), unclipped
    assert len({round(u, 6) for u in unclipped if u < 1.0}) >= 2


@pytest.mark.parametrize("shape", [s for s in ALL_SPLIT_SHAPES if s[0] * s[1] >= 64], ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_histograms_spread(shape):
    spread = []
    for iname, img in split_images(*shape):
        _, lbp, gray, _ = O.split_stats(img, np.ones(shape, bool))
        spread.append(((lbp > 0).sum(), (gray > 0).sum()))
    assert any(a >= 3 and b >= 2 for a, b in spread), spread


def test_split_stats_shape_and_count():
    img = split_images(9, 33)[0][1]
    for mname, m in split_masks(9, 33):
        sums, lbp, gray, abs_sums = O.split_stats(img, m)
        n = (O.sk_rgb2gray(img) > 0.01).sum() if m is None else m.sum()
        assert sums.shape == abs_sums.shape == (12,) and sums.dtype == np.float64 and lbp.shape == (10,) and gray.shape == (32,)
        assert sums[0] == n == lbp.sum() == gray.sum() and (abs_sums >= np.abs(sums)).all()


def test_score_boundary_masks():
    """99 / 100 / 101 masked pixels, and frames whose pixels above gray 0.01 number 99 and 100"""
    for n in (99, 100, 101):
        assert score_mask(17, 65, n).sum() == n
    for n in (99, 100):
        assert (O.sk_rgb2gray(dark_frame(n)) > 0.01).sum() == n
    img = split_images(17, 65)[0][1]
    assert O.split_score(img, score_mask(17, 65, 99)) == (0.0, 0.0, 0.0) != O.split_score(img, score_mask(17, 65, 100))
    assert O.split_score(dark_frame(99)) == (0.0, 0.0, 0.0) != O.split_score(dark_frame(100))


def dark_frame(n):
    """a 16 x 33 frame of (2, 2, 2) (gray 0.0078) with n brighter pixels, some of them at (3, 3, 3) (gray 0.0118, just above 0.01)"""
    rng = np.random.default_rng(n)
    img = np.full((16 * 33, 3), 2, np.uint8)
    at = rng.permutation(16 * 33)[:n]
    img[at] = rng.integers(3, 256, (n, 3))
    img[at[:10]] = 3
    return img.reshape(16, 33, 3)


def test_slic_sweeps_vs_literal_loop():
    """one sweep of O.slic_sweeps == the per-pixel loop on every assignment case without NaN centroids (on those the oracle raises:
    int(nan)), with both values of ignore_color; and the cases hold what they are there for"""
    cases = assign_cases()
    unassigned = ties = 0
    for i, (name, img, mask, seg, step) in enumerate(cases):
        for ic in (True, False):
            want, un, ti = assign_reference(i, ic)
            unassigned += un
            ties += ti
            if np.isnan(seg).any():
                with pytest.raises(ValueError):
                    O.slic_sweeps(img, mask, seg.copy(), step, 1, ic)
            else:
                assert np.array_equal(O.slic_sweeps(img, mask, seg.copy(), step, 1, ic), want), (name, ic)
            assert (want[~mask] == 0).all()
            if len(seg) >= 2 and mask.size >= 64:
                assert len(np.unique(want[mask])) >= 2, (name, ic)
    assert unassigned > 0 and ties > 0
    by_name = {c[0]: i for i, c in enumerate(cases)}
    lab = assign_reference(by_name["tie_9x9"], True)[0]
    assert lab[4, 4] == 1 and assign_reference(by_name["tie_9x9"], True)[2] > 0
    assert assign_reference(by_name["tie_colour_9x9"], False)[2] > 0
    assert assign_reference(by_name["tiny_step_19x27"], True)[1] > 19 * 27 // 2          # most pixels outside every window
    lab = assign_reference(by_name["nan_rows_16x16"], False)[0]
    assert set(np.unique(lab)) <= {0, 1, 3, 5} and len(np.unique(lab)) >= 3              # the NaN rows take no pixel
    lab = assign_reference(by_name["duplicates_16x16"], False)[0]
    assert set(np.unique(lab)) - {0} == {1, 3}                                              # the first of equal centroids
    assert {c[1].shape[:2] for c in cases} >= set(SLIC_SHAPES) and {len(c[3]) for c in cases} >= set(SLIC_K) | {K_LDS_MAX}


def test_sweep_regions_reference():
    """the oracle runs the 2 x 10 sweeps of every region without raising, every region but the windowless one keeps all its centroids
    (no NaN) and, from 64 pixels on, two labels or more; the windowless one keeps label 0 and its seeds"""
    regions, ref = sweep_regions(), sweep_reference()
    assert {m.size for _, m, _, _ in regions} >= {1, 63, 64, 65, 511, 512, 513, 1025}
    for r, ((img, mask, seg0, step), (labels, seg)) in enumerate(zip(regions, ref)):
        if r == SWEEP_NO_WINDOW:
            assert mask.any() and (labels == 0).all() and seg.tobytes() == seg0.tobytes()
            continue
        assert not np.isnan(seg).any() and (labels[mask] > 0).all() and (labels[~mask] == 0).all()
        assert seg.tobytes() != seg0.tobytes()
        if mask.size >= 64 and len(seg) >= 2:
            assert len(np.unique(labels[mask])) >= 2, r


def test_degenerate_slic_regions_on_the_oracle():
    """O.sk_resize and O.enhanced_slic run on every thin shape; the downscale to 0 rows raises OverflowError"""
    for (h, w), out_hw in RESIZE_SHAPES:
        img = np.random.default_rng(h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert O.sk_resize(img, out_hw, 1, True).shape == out_hw + (3,)
    labelled = 0
    for ragged in (False, True):
        for img, mask, n in slic_region_inputs(ragged):
            seg = O.enhanced_slic(img, mask, n_segments=n)
            assert seg.shape == mask.shape and seg.dtype == np.int32
            labelled += int(seg.max() >= 1)             # (5 x 2000 ragged: every run of the 1 x 400 mask is under min_size -> all 0)
    assert labelled >= 2 * len(SLIC_REGIONS) - 2
    h, w, n = SLIC_RAISING
    with pytest.raises(OverflowError), np.errstate(divide="ignore"):
        O.enhanced_slic(np.zeros((h, w, 3), np.uint8), full_mask(h, w), n_segments=n)
