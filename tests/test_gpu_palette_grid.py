"""The candidate-grid search on the device (csrc/palette_grid.hip: Rhccq.palette_grid, Rhccq.palette_remap(grid=),
ImageEncoder.encode_with_palette / encode_sequence with search="grid"): the device grid against the host form byte for byte, the remap
through it against the brute-force reference of tests/remap_cases.py, the encoder's results against those of the full search.  GPU only."""
import numpy as np
import pytest

import grid_cases as G
import remap_cases as RM
import roimask_cases as RC
from test_gpu_palette_remap import _idx64, _same_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


@pytest.fixture(scope="module")
def enc(rh):
    from roibasedimagecompression_amd.image import ImageEncoder
    return ImageEncoder(rh)


@pytest.mark.parametrize("name", G.NAMES)
def test_device_grid_and_remap(rh, name):
    import torch
    rgb, pal, cls, nc, entries = G.CASES[name]
    want_idx, want_sums = G.reference(name)
    h_work, h_entries, h_stats = G.host_grid(name)
    grid = rh.palette_grid(pal, entries)                                       # None: sized by a first build, then built exactly
    assert grid.stats == dict(zip(("listed", "flagged", "entries", "longest"), (int(v) for v in h_stats)))
    assert grid.entries == (int(h_stats[2]) if entries is None else entries) and grid.K == len(pal)
    used = int(h_stats[2])
    for got, want in zip(G.pieces(grid.work.cpu().numpy(), grid.entries), G.pieces(h_work, h_entries)):
        small = len(got) != G.CELLS                                            # lists and row ids: the entries in use (the rest is never written)
        assert np.array_equal(got[:used] if small else got, want[:used] if small else want), name
    h_cells = G.pieces(h_work, h_entries)[0]
    px = rgb.astype(np.int64)
    flagged = int((h_cells[(px[:, 0] >> 3) << 10 | (px[:, 1] >> 3) << 5 | px[:, 2] >> 3, 1] == 0).sum())
    for _ in range(2):                                                         # the grid is reused; every call zeroes its own sums
        idx, sums = rh.palette_remap(rgb, pal, cls, nc, grid=grid)
        assert idx.dtype == (torch.uint8 if len(pal) <= 256 else torch.int16) and tuple(idx.shape) == (len(rgb),)
        assert np.array_equal(_idx64(idx), want_idx) and np.array_equal(sums.cpu().numpy(), want_sums), name
        assert int(grid.overflow.item()) == flagged, name
    # the C entry in every index width the palette allows
    d_rgb, d_pal, d_cls = rh.dev(rgb), rh.dev(pal), None if cls is None else rh.dev(cls)
    work = rh.empty((int(rh.lib.rhccq_palette_remap_grid_bytes(len(rgb))),), torch.uint8)
    for eb in RM.index_bytes(len(pal)):
        idx = torch.full((len(rgb),), 0x2B, dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[eb], device=rh.device)
        sums, over = torch.full((nc + 1, 2), 0x55, dtype=torch.int64, device=rh.device), torch.full((1,), 0x55, dtype=torch.int64, device=rh.device)
        rc = rh.lib.rhccq_palette_remap_grid(rh.ctx, rh._p(d_rgb), len(rgb), rh._p(d_pal), len(pal), rh._p(d_cls), nc, rh._p(grid.work), grid.entries,
                                             rh._p(idx), eb, rh._p(sums), rh._p(work), work.numel(), rh._p(over))
        assert rc == 0, (name, eb)
        assert np.array_equal(_idx64(idx), want_idx) and np.array_equal(sums.cpu().numpy(), want_sums) and int(over.item()) == flagged, (name, eb)


def test_encode_with_palette_search_grid(rh, enc):
    (q1, q2), img, mask = RC.case("photo96")
    pal = np.asarray(enc.encode(img, q1, q2)["palette"], np.uint8).reshape(-1, 3)
    for kw in ({}, {"roi_mask": mask}, {"refine": 2}):
        full, grid = enc.encode_with_palette(img, pal, **kw), enc.encode_with_palette(img, pal, search="grid", **kw)
        assert _same_result(full, grid) and full["stats"]["remap"] == grid["stats"]["remap"], kw
        assert "search" not in full["stats"] and grid["stats"].get("refine") == full["stats"].get("refine")
        row = grid["stats"]["search"]
        assert row["kind"] == "grid" and row["listed"] == G.CELLS and row["flagged"] == 0 and row["overflow_pixels"] == 0
        assert 1 <= row["longest"] <= len(pal) and row["entries"] >= G.CELLS
    given = rh.palette_grid(pal, 4000)                                         # a caller's grid: most cells flagged, the result the same
    out = enc.encode_with_palette(img, pal, search=given)
    assert _same_result(out, enc.encode_with_palette(img, pal)) and out["stats"]["search"]["overflow_pixels"] > 0
    with pytest.raises(ValueError, match="search must be"):
        enc.encode_with_palette(img, pal, search="fast")
    with pytest.raises(ValueError, match="serves the plain remap only"):
        enc.encode_with_palette(img, pal, search="grid", run_slack=3)
    with pytest.raises(ValueError, match="cannot be combined with refine or colours"):
        enc.encode_with_palette(img, pal, search=given, refine=1)


def test_encode_sequence_search_grid(enc):
    frames = RM.sequence_frames()
    q1, q2 = RM.SEQ_QUALITIES
    full = list(enc.encode_sequence(frames, q1, q2, RM.SEQ_MAX_DROP_DB))
    grid = list(enc.encode_sequence(frames, q1, q2, RM.SEQ_MAX_DROP_DB, search="grid"))
    assert [r["stats"]["key_frame"] for r in grid] == [True, False, True, False]
    for a, b in zip(full, grid):
        assert _same_result(a, b) and a["stats"]["psnr"] == b["stats"]["psnr"] and a["stats"].get("remap") == b["stats"].get("remap")
        assert ("search" in b["stats"]) == (not b["stats"]["key_frame"])
    with pytest.raises(ValueError, match='search must be "full" or "grid"'):
        list(enc.encode_sequence(frames, q1, q2, RM.SEQ_MAX_DROP_DB, search="lists"))
