"""The optimising JPEG writer on the device (csrc/jpeg_optimize.hip; include/rhccq.h "JPEG files written with optimised Huffman tables")
against its serial host forms, the bytes Pillow saves with optimize=True, and libjpeg's table rule, over tests/jpegopt_cases.py."""
import numpy as np
import pytest
import torch

import jpegopt_cases as O
import jpegwrite_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


@pytest.mark.parametrize("name", list(O.CASES))
def test_device_equals_host_and_pillow(rh, name):
    from roibasedimagecompression_amd import container
    _, _, mode, quality, rows, _ = O.CASES[name]
    coef, counts, data = O.host(name)
    src = torch.from_numpy(O.image(name)).to(rh.device)
    got = rh.jpeg_histogram(rh.jpeg_blocks(src, mode, quality), src.shape, mode, rows)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), counts), name
    assert container.jpeg_bytes(src, rh, quality=quality, subsampling=mode, restart_rows=rows, optimize=True) == data == O.pillow(name), name


@pytest.mark.parametrize("name", list(O.COUNT_CASES))
def test_device_tables_equal_libjpegs_rule(rh, name):
    made = rh.jpeg_huffman(O.counts_of(name), (16, 16), O.COUNT_CASES[name][0]).cpu().numpy()
    O.check_tables(name, made)
    assert np.array_equal(made, O.host_tables(name)), name


@pytest.mark.parametrize("name", ["17x33_420", "noise_q100", "impulses"])
def test_optimize_off_is_the_writer(rh, name):
    from roibasedimagecompression_amd import container
    _, _, mode, quality, rows, _ = W.CASES[name]
    assert container.jpeg_bytes(W.image(name), rh, quality=quality, subsampling=mode, restart_rows=rows, optimize=False) == W.pillow(name), name


def test_resize_writes_the_optimised_file_of_what_it_returns(rh, tmp_path):
    import io
    from PIL import Image
    from roibasedimagecompression_amd.image import ImageEncoder
    path = tmp_path / "out.jpg"
    small = ImageEncoder(rh).resize(O.image("64x64_q100"), (20, 28), "triangle", jpeg_path=str(path), quality=90, subsampling="444", optimize=True)
    want = io.BytesIO()
    Image.fromarray(small.cpu().numpy()).save(want, "JPEG", quality=90, subsampling=0, optimize=True)
    assert path.read_bytes() == want.getvalue()
