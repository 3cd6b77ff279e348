"""The oracle's statement of the image -> .rhccq script flow (oracle.rhccq_oracle.script_flow) and its G16 fixtures, on the CPU.

The cheap cases of tests/golden/make_golden_flow.py are re-run and must reproduce their fixtures exactly (this ties the fixtures
that tests/test_gpu_flow_oracle.py compares the device with to the oracle); the glue the oracle states between the stages (segment
count, find_contours' drop rule, the swallowed exception of an empty class) has unit tests of its own."""
import importlib.util
import math
import os

import numpy as np
import pytest

from oracle import rhccq_oracle as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen():
    spec = importlib.util.spec_from_file_location("make_golden_flow", os.path.join(G, "make_golden_flow.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MG = _gen()


def _fixture(name):
    with np.load(os.path.join(G, MG.PREFIX + name + ".npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("name", MG.CHEAP)
def test_oracle_flow_reproduces_fixture(name):
    fx = _fixture(name)
    img = MG.case_image(name, fx)
    arrays, _ = MG.fixture_arrays(name, img, tuple(int(q) for q in fx["qualities"]))
    assert sorted(arrays) == sorted(fx)
    for k in fx:
        assert arrays[k].dtype == fx[k].dtype and np.array_equal(arrays[k], fx[k]), k


@pytest.mark.parametrize("name", list(MG.CASES))
def test_fixture_normalize_margin(name):
    """every region's normalize_result is more than 1e-6 from the integer its ceil changes at: a failure here is a precision tie
    between two correct float64 statements of the split score, not a bug"""
    fx = _fixture(name)
    if "error" in fx:
        # flat: the ROI stage's unset best_low (edges.py); strip2: its one segment is dropped, quantize_image([]) -> merged[0]
        assert str(fx["error"]) == {"flat": "UnboundLocalError", "strip2": "IndexError"}[name]
        return
    for v in fx["norm"]:
        assert MG.normalize_margin(float(v)) > 1e-6, f"precision tie: normalize_result {v!r}"


def test_fixture_sizes():
    total = 0
    for name in MG.CASES:
        n = os.path.getsize(os.path.join(G, MG.PREFIX + name + ".npz"))
        assert n < 500_000, name
        total += n
    assert total < 3_000_000


# ---- the glue -------------------------------------------------------------------------------------------------------------------
def test_drop_rule_constant_mask():
    assert O.find_contours_drops(np.ones((2, 2), bool))
    assert O.find_contours_drops(np.ones((7, 5), bool))


def test_drop_rule_non_constant_mask():
    m = np.ones((4, 6), bool)
    m[3, 5] = False                                           # one level crossing is enough for a contour
    assert not O.find_contours_drops(m)
    m = np.zeros((4, 6), bool)
    m[1:3, 1:4] = True
    assert not O.find_contours_drops(m)


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1)])
def test_drop_rule_one_pixel_boxes(shape):
    """boxes thinner than 2 px take the tiny-segment branch (slic.py:168-186): kept, even when the segment fills the box"""
    assert not O.find_contours_drops(np.ones(shape, bool))


def test_kept_segments_order_and_drops():
    lab = np.array([[3, 3, 0], [5, 5, 5]], np.int32)
    kept, dropped, out = O.kept_segments(lab, np.ones((2, 3), bool))
    assert kept == [3, 5] and dropped == []
    assert np.array_equal(out, lab)
    lab = np.full((3, 4), 7, np.int32)
    mask = np.ones((3, 4), bool)
    mask[0, 0] = False
    kept, dropped, out = O.kept_segments(lab, mask)
    assert kept == [7] and dropped == [] and out[0, 0] == 0        # (0, 0) is outside the mask: 7 does not fill the box
    kept, dropped, out = O.kept_segments(np.full((3, 4), 7, np.int32), np.ones((3, 4), bool))
    assert kept == [] and dropped == [7] and not out.any()
    kept, dropped, out = O.kept_segments(np.full((1, 4), 7, np.int32), np.ones((1, 4), bool))
    assert kept == [7] and dropped == []


def test_under_100_pixels_scores_zero_and_gives_one_segment():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (12, 12, 3), dtype=np.uint8)
    mask = np.zeros((12, 12), bool)
    mask.reshape(-1)[:99] = True
    n, nr, score = O.region_segment_count(img, mask)
    assert score == 0.0 and n == 1
    window = math.ceil(math.ceil(math.log(img.size, 10)) * math.log(img.size))
    assert nr == window / (1 + math.exp(6.0))
    mask.reshape(-1)[99] = True                                # 100 pixels: scored
    assert O.region_segment_count(img, mask)[2] > 0


def test_segment_count_slope():
    """ceil(window / (1 + exp(-12 (s - 0.5)))) away from s = 0.5, where a wrong slope is visible"""
    w = 40
    for s, want, slope11 in ((0.25, 2, 3), (0.75, 39, 38)):
        assert math.ceil(O.normalize_result(s, w)) == want
        assert math.ceil(w / (1 + math.exp(-11 * (s - 0.5)))) == slope11 != want


def test_empty_class_is_swallowed_and_empty_image_raises(monkeypatch):
    """script_flow's bare except around region_quantization: a class without components is left out of level 3; with no
    component at all quantize_image's merged[0] raises IndexError"""
    img = np.zeros((8, 8, 3), np.uint8)
    img[:, :4] = (200, 10, 10)
    img[:, 4:] = (10, 10, 200)
    mask = np.ones((8, 8), bool)
    lab = np.zeros((8, 8), np.int32)
    lab[:, :4], lab[:, 4:] = 1, 2
    region = {"bbox": (0, 0, 8, 8), "bbox_mask": mask, "area": 64}
    monkeypatch.setattr(O, "get_regions", lambda image: (None, np.ones((8, 8), np.uint8), None, None, mask, ~mask))
    monkeypatch.setattr(O, "extract_regions", lambda image, a, b: ([dict(region)], []))
    monkeypatch.setattr(O, "enhanced_slic", lambda image, m, n_segments: lab)
    r = O.script_flow(img, 20, 10)
    assert r["level2"][1] is None and r["level2_error"] == [None, "IndexError"]
    assert r["regions"][0][0]["kept"] == [1, 2]
    assert tuple(r["final"]["shape"]) == (8, 8)
    pal, idx, shape = O.decode_container(O.load_container(r["file_bytes"]))
    assert np.array_equal(pal, np.asarray(r["final"]["palette"], np.uint8).reshape(-1, 3)) and shape == (8, 8)
    # every segment fills the box: dropped, both calls raise, quantize_image raises
    monkeypatch.setattr(O, "enhanced_slic", lambda image, m, n_segments: np.ones((8, 8), np.int32))
    with pytest.raises(IndexError):
        O.script_flow(img, 20, 10)
