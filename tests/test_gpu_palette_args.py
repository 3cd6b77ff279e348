"""The argument layer of the Rhccq.palette_* wrappers on the device: every wrapper that takes pixels gives the same tensors (dtype, shape,
values) whether its inputs come as numpy arrays, CPU tensors or device tensors and whether the class map is bool or uint8, at K = 3
and at K = 257 (the first K with 2-byte indices); and an empty image gives empty indices and zeroed sums.  What the values ARE is the
business of each operation's own test file.  GPU only."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W = 5, 7
OFF = [0, 2 * W, H * W]                       # the batched forms: two images, 2 and 3 image rows
WEIGHTS, TABLE = [1, 3, 1], [40, 0, 9]


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


def _batch(t, pal):
    """the two palettes of the batched forms and their rows: the second image uses one row less"""
    return t(np.stack([pal, pal])), t(np.array([len(pal), len(pal) - 1], np.int32))


def _flat(t, a):
    return None if a is None else t(a.reshape((-1,) + a.shape[2:]))


# name -> call(rh, t, rgb, pal, cls, nc, off): t puts a numpy array into the form under test; cls is None with nc = 0
WRAPPERS = {
    "remap": lambda rh, t, rgb, pal, cls, nc, off: rh.palette_remap(t(rgb), t(pal), cls, nc),
    "runs": lambda rh, t, rgb, pal, cls, nc, off: rh.palette_runs(t(rgb), t(pal), TABLE if nc else 40, cls, nc),
    "segment": lambda rh, t, rgb, pal, cls, nc, off: rh.palette_segment(t(rgb), t(pal), TABLE if nc else 40, cls, nc),
    "refine": lambda rh, t, rgb, pal, cls, nc, off: rh.palette_refine(t(rgb), t(pal), cls, WEIGHTS if nc else None, max_iter=2),
    "moments": lambda rh, t, rgb, pal, cls, nc, off: rh.palette_moments(t(rgb), t(pal), cls, nc),
    "cells": lambda rh, t, rgb, pal, cls, nc, off: (rh.palette_cells(t(rgb), cls, nc, WEIGHTS if nc else None),),
    "cells_batch": lambda rh, t, rgb, pal, cls, nc, off: (rh.palette_cells_batch(_flat(t, rgb), off, cls, nc, WEIGHTS if nc else None),),
    "remap_batch": lambda rh, t, rgb, pal, cls, nc, off: rh.palette_remap_batch(_flat(t, rgb), off, *_batch(t, pal), cls, nc),
    "refine_batch": lambda rh, t, rgb, pal, cls, nc, off: rh.palette_refine_batch(_flat(t, rgb), off, *_batch(t, pal), cls, WEIGHTS if nc else None, 2),
}


def _forms(rh):
    return {"numpy": lambda a: a, "cpu tensor": lambda a: torch.from_numpy(a.copy()), "device tensor": lambda a: rh.dev(a)}


def _same(got, want):
    return len(got) == len(want) and all((g is None and w is None) or (g.dtype == w.dtype and g.shape == w.shape and g.is_cuda and torch.equal(g, w))
                                         for g, w in zip(got, want))


def _inputs(K, h=H):
    rng = np.random.default_rng(K)
    rgb, pal = rng.integers(0, 256, (h, W, 3), dtype=np.uint8), rng.integers(0, 256, (K, 3), dtype=np.uint8)
    return rgb, pal, rng.integers(0, 2, (h, W)).astype(bool)


@pytest.mark.parametrize("K", [3, 257])
@pytest.mark.parametrize("name", list(WRAPPERS))
def test_every_input_form_gives_the_same_tensors(rh, name, K):
    rgb, pal, m = _inputs(K)
    call = WRAPPERS[name]
    plain = call(rh, lambda a: a, rgb, pal, None, 0, OFF)
    classed = call(rh, lambda a: a, rgb, pal, m.astype(np.uint8), 2, OFF)
    if name in ("remap", "runs", "segment", "moments", "remap_batch"):                                   # the index width follows K
        assert plain[0].dtype == classed[0].dtype == (torch.uint8 if K <= 256 else torch.int16)
    for form, t in _forms(rh).items():
        assert _same(call(rh, t, rgb, pal, None, 0, OFF), plain), (form, "no class map")
        for kind in (bool, np.uint8):
            cls = t(m.astype(kind))
            assert _same(call(rh, t, rgb, pal, cls if "batch" not in name else cls.reshape(-1), 2, OFF), classed), (form, kind.__name__)


# per wrapper: which outputs of an empty image are the (unchanged) palettes; every other output is empty or all zero
_ECHO = {"refine": 0, "refine_batch": 0}


@pytest.mark.parametrize("K", [3, 257])
@pytest.mark.parametrize("name", list(WRAPPERS))
def test_the_empty_image(rh, name, K):
    rgb, pal, m = _inputs(K, h=0)
    assert rgb.shape == (0, W, 3)
    for form, t in _forms(rh).items():
        for cls, nc in ((None, 0), (t(m), 2), (t(m.astype(np.uint8)), 2)):
            got = WRAPPERS[name](rh, t, rgb, pal, cls if cls is None or "batch" not in name else cls.reshape(-1), nc, [0, 0, 0])
            for i, g in enumerate(got):
                if _ECHO.get(name) == i:
                    assert np.array_equal(g.cpu().numpy(), pal if g.ndim == 2 else np.stack([pal, pal])), (form, nc)
                else:
                    assert g.is_cuda and not g.any(), (form, nc, i)
            if name in ("remap", "runs", "segment", "moments"):
                assert tuple(got[0].shape) == (0, W) and got[0].dtype == (torch.uint8 if K <= 256 else torch.int16)
                assert tuple(got[1].shape)[0] == nc + 1 and got[1].dtype == torch.int64 and got[1].numel() > 0
            if name == "remap_batch":
                assert tuple(got[0].shape) == (0,) and tuple(got[1].shape) == (2, nc + 1, 2)
