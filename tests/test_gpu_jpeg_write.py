"""The JPEG writer on the device (csrc/jpeg_write.hip; include/rhccq.h "JPEG files written on the device") against its serial host form and
against the bytes Pillow saves, over the cases of tests/jpegwrite_cases.py."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpegwrite_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("name", W.names())
def test_device_equals_host_and_pillow(rh, name, resident):
    from roibasedimagecompression_amd import container
    _, _, mode, quality, rows, _ = W.CASES[name]
    img = W.image(name)
    coef, _ = W.host_encode(img, mode, quality, rows)
    src = torch.from_numpy(img).to(rh.device) if resident else img
    assert np.array_equal(rh.jpeg_blocks(src, mode, quality).cpu().numpy(), coef), name
    assert container.jpeg_bytes(src, rh, quality=quality, subsampling=mode, restart_rows=rows) == W.pillow(name), name


def test_a_result_dict_is_written_as_it_is_shown(rh):
    from roibasedimagecompression_amd import container
    rng = np.random.default_rng(5)
    pal, idx = rng.integers(0, 256, (7, 3)).astype(np.uint8), rng.integers(0, 7, (19, 23)).astype(np.uint8)
    got = container.jpeg_bytes({"palette": pal, "indices": idx.reshape(-1), "shape": (19, 23)}, rh, quality=80, subsampling="422")
    assert got == W.save(pal[idx], 80, "422", 0)


def test_the_reader_reads_the_writer(rh, tmp_path):
    from roibasedimagecompression_amd import container
    path = tmp_path / "x.jpg"
    n = container.write_jpeg(W.image("17x33_420"), str(path), rh, quality=85, restart_rows=2)
    assert n == path.stat().st_size
    assert np.array_equal(container.read_jpeg(str(path), rh)["image"].cpu().numpy(), np.asarray(Image.open(io.BytesIO(path.read_bytes())).convert("RGB")))


def test_resize_writes_the_file_of_what_it_returns(rh, tmp_path):
    from roibasedimagecompression_amd.image import ImageEncoder
    src, path = tmp_path / "in.jpg", tmp_path / "out.jpg"
    src.write_bytes(W.pillow("noise_q100"))
    small = ImageEncoder(rh).resize(str(src), (20, 28), "triangle", jpeg_path=str(path), quality=90, subsampling="444")
    assert tuple(small.shape) == (20, 28, 3) and path.read_bytes() == W.save(small.cpu().numpy(), 90, "444", 0)
