"""The resize on the device (csrc/resize.hip, Rhccq.resize, the size= / resample= keywords of ImageEncoder.animate and
container.reduce_gif) against the numpy reference of tests/resize_cases.py, byte for byte.  GPU only."""
import io

import numpy as np
import pytest

import resize_cases as RC

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


def _raw_resize(rh, a, OH, OW, filt):
    """rhccq_resize itself into a buffer pre-filled and longer than the output: unwritten and overrun bytes show"""
    import torch
    B, H, W, Cn = a.shape
    n = B * OH * OW * Cn
    src = rh.dev(np.ascontiguousarray(a))
    dst = torch.full((n + GUARD,), 0xAB, dtype=torch.uint8, device=rh.device)
    need = int(rh.lib.rhccq_resize_workspace_bytes(B, H, W, Cn, OH, OW))
    work = torch.full((need,), 0xCD, dtype=torch.uint8, device=rh.device)
    rc = rh.lib.rhccq_resize(rh.ctx, rh._p(src), B, H, W, Cn, rh._p(dst), OH, OW, RC.FILTERS.index(filt), rh._p(work), need)
    out = dst.cpu().numpy()
    return rc, out[:n].reshape(B, OH, OW, Cn), out[n:]


@pytest.mark.parametrize("filt", RC.FILTERS)
@pytest.mark.parametrize("name", list(RC.SHAPES))
def test_device_equals_reference(rh, name, filt):
    rc, out, guard = _raw_resize(rh, RC.case(name), *RC.SHAPES[name][4:6], filt)
    assert rc == 0
    assert np.array_equal(out, RC.reference(name, filt))
    assert (guard == 0xAB).all()


@pytest.mark.parametrize("filt", RC.FILTERS)
def test_batch_equals_single_calls_and_every_rank(rh, filt):
    a = RC.case("batch3")
    OH, OW = RC.SHAPES["batch3"][4:6]
    whole = rh.resize(a, (OH, OW), filt).cpu().numpy()
    assert np.array_equal(whole, RC.reference("batch3", filt))
    for b in range(a.shape[0]):
        assert np.array_equal(rh.resize(a[b], (OH, OW), filt).cpu().numpy(), whole[b])
    grey = np.ascontiguousarray(a[0, :, :, 0])
    assert np.array_equal(rh.resize(grey, (OH, OW), filt).cpu().numpy(), RC.resize_reference(grey, OH, OW, filt))
    assert tuple(rh.resize(rh.dev(a[0]), 10, filt).shape) == (6, 10, 3)               # one integer: the longest side (35 -> 10, 21 -> 6)


def test_animate_and_reduce_gif_resize(rh, tmp_path):
    """animate(size=, resample=) is animate of the frames the reference resizes; reduce_gif(size=) writes frames of the new size that
    decode under Pillow to palette[indices]"""
    from PIL import Image
    from roibasedimagecompression_amd import container
    from roibasedimagecompression_amd.image import ImageEncoder
    enc = ImageEncoder(rh)
    rng = np.random.default_rng(3)
    base = rng.integers(0, 256, (1, 12, 16, 3), dtype=np.uint8).repeat(4, axis=1).repeat(4, axis=2)
    frames = np.concatenate([np.roll(base, 3 * i, axis=2) for i in range(3)])        # 3 frames of 48 x 64
    got = enc.animate(frames, colours=16, size=(20, 27), resample="cubic", delta=False)
    want = enc.animate(RC.resize_reference(frames, 20, 27, "cubic"), colours=16, delta=False)
    assert got["shape"] == (20, 27) and got["stats"]["resize"] == {"from": (48, 64), "to": (20, 27), "filter": "cubic"}
    assert np.array_equal(got["palette"], want["palette"]) and np.array_equal(got["indices"].cpu().numpy(), want["indices"].cpu().numpy())
    src, dst = str(tmp_path / "in.gif"), str(tmp_path / "out.gif")
    enc.animate(frames, colours=32, gif_path=src, delta=False)
    res = container.reduce_gif(src, dst, 16, rh, delta=False, size=32)
    assert res["shape"] == (24, 32) and res["stats"]["resize"]["to"] == (24, 32)
    shown = container.read_gif(src, rh)["images"].cpu().numpy()
    want = enc.animate(RC.resize_reference(shown, 24, 32, "lanczos"), colours=16, delta=False)
    assert np.array_equal(res["indices"].cpu().numpy(), want["indices"].cpu().numpy())
    with Image.open(io.BytesIO(open(dst, "rb").read())) as im:
        assert im.size == (32, 24) and im.n_frames == 3
        for i in range(3):
            im.seek(i)
            assert np.array_equal(np.asarray(im.convert("RGB")), res["palette"][res["indices"][i].cpu().numpy()])
