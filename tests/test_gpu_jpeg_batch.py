"""The batch JPEG reader on the device (csrc/jpeg_batch.hip; include/rhccq.h "JPEG files read as a batch"): every file of a batch against
Pillow's decode, byte for byte, and its counters against those container.read_jpeg reports for the file alone."""
import numpy as np
import pytest

import jpeg_cases as J

pytestmark = pytest.mark.gpu

BIG, SMALL = "noise_many_subsequences", ["8x8_grey_0", "8x8_444_1", "8x8_420_0"]
COMPOSITIONS = {
    "all_128": (J.names(), 128),
    "all_default": (J.names(), None),
    "one": (["17x33_420_0"], None),
    "thrice": (["17x33_420_0"] * 3, None),
    "big_first": ([BIG] + SMALL, 128),
    "big_middle": (SMALL[:2] + [BIG] + SMALL[2:], 128),
    "big_last": (SMALL + [BIG], 128),
}
COUNTERS = ("bytes", "subsequences", "subsequence_bits", "sync_rounds", "worst_walk")


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


@pytest.fixture(scope="module")
def alone(rh):
    """(name, bits) -> read_jpeg's counters for the file alone, read once"""
    from roibasedimagecompression_amd import container
    seen = {}

    def get(name, bits):
        if (name, bits) not in seen:
            seen[name, bits] = {k: container.read_jpeg(J.case(name), rh, subsequence_bits=bits)["stats"][k] for k in COUNTERS}
        return seen[name, bits]
    return get


def _right(res, i, name):
    return res["shapes"][i] == J.reference(name).shape[:2] and np.array_equal(res["images"][i].cpu().numpy(), J.reference(name))


@pytest.mark.parametrize("comp", list(COMPOSITIONS))
def test_batch_equals_pillow_and_the_files_alone(rh, alone, comp):
    from roibasedimagecompression_amd import container
    names, bits = COMPOSITIONS[comp]
    res = container.read_jpeg_batch([J.case(n) for n in names], rh, subsequence_bits=bits)
    assert res["status"] == [(0, 0)] * len(names)
    for i, name in enumerate(names):
        assert _right(res, i, name), (i, name)
        assert res["stats"]["files"][i] == alone(name, bits), (i, name)
    if BIG in names and bits == 128:
        assert res["stats"]["files"][names.index(BIG)]["subsequences"] > 256, "several workgroups' worth: the boundary walk runs"


@pytest.mark.parametrize("bad, status", [(J.bad_scan()[0], (J.BAD_SCAN, 2)), (J.malformed()["progressive"][0], (J.UNSUPPORTED, None))])
def test_a_refused_file_in_the_middle(rh, bad, status):
    from roibasedimagecompression_amd import container
    from roibasedimagecompression_amd._lib import RhccqError
    files = [J.case("17x33_420_0"), bad, J.case("33x15_444_1")]
    res = container.read_jpeg_batch(files, rh, subsequence_bits=128, strict=False)
    assert res["status"][0] == res["status"][2] == (0, 0) and res["status"][1][0] == status[0] and status[1] in (None, res["status"][1][1])
    assert res["images"][1] is None and res["shapes"][1] is None and "batch" not in res
    assert _right(res, 0, "17x33_420_0") and _right(res, 2, "33x15_444_1")
    with pytest.raises(RhccqError, match=rf"read_jpeg_batch: file 1: RHCCQ_JPEG_\w+ \(status {status[0]}\)") as e:
        container.read_jpeg_batch(files, rh, subsequence_bits=128)
    assert e.value.index == 1 and e.value.status == status[0]


@pytest.mark.parametrize("shape, view", [("16x16", True), ("7x9", False)])
def test_equal_shapes_give_one_tensor(rh, shape, view):
    from roibasedimagecompression_amd import container
    names = [f"{shape}_{mode}" for mode in ("grey_0", "444_1", "422_0", "420_1")]
    res = container.read_jpeg_batch([J.case(n) for n in names], rh)
    want = np.stack([J.reference(n) for n in names])
    assert (3 * want.shape[1] * want.shape[2] % 16 == 0) == view
    assert tuple(res["batch"].shape) == want.shape and np.array_equal(res["batch"].cpu().numpy(), want)
    assert (res["batch"].data_ptr() == res["images"][0].data_ptr()) == view


def test_animate_reads_its_jpeg_names_together(rh, tmp_path):
    from roibasedimagecompression_amd import container
    from roibasedimagecompression_amd.image import ImageEncoder
    names = ["16x16_444_1", "16x16_420_1", "16x16_grey_0"]
    paths = [tmp_path / f"{n}.jpg" for n in names]
    for path, n in zip(paths, names):
        path.write_bytes(J.case(n))
    enc = ImageEncoder()
    a, b = enc.animate([str(paths[0]), J.reference(names[1]), paths[2]], 16), enc.animate([J.reference(n) for n in names], 16)
    assert np.array_equal(a["indices"].cpu().numpy(), b["indices"].cpu().numpy()) and np.array_equal(np.asarray(a["palette"]), np.asarray(b["palette"]))
    alone = [container.read_jpeg(str(paths[i]), rh) for i in (0, 2)]
    assert a["stats"]["jpeg_in"] == [{"shape": [16, 16], **fr["info"], **{k: fr["stats"][k] for k in ("subsequences", "sync_rounds")}} for fr in alone]
    both = container.read_images(paths[:2], rh)
    assert all(np.array_equal(fr["image"].cpu().numpy(), J.reference(n)) and fr["shape"] == (16, 16) for fr, n in zip(both, names))
