"""The batched palette build path on the device (csrc/palette_batch.hip, Rhccq.palette_*_batch, ImageEncoder.quantize_batch): every
image of a batch against the per-image references of tests/build_cases.py, remap_cases.py and refine_cases.py, bit for bit, at the shapes
where batching can go wrong (an image that starts inside a chunk, empty images, tables that cannot reach K_target, more chains than
CUs, rows behind k_rows that must not be read, images that stop refining at different iterations), and quantize_batch against the loop of
quantize it replaces.  GPU only."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import build_cases as BC
import refine_cases as RF
import remap_cases as RM

pytestmark = pytest.mark.gpu

E_ARG, E_LIMIT = BC.E_ARG, BC.E_LIMIT
CELLS = 4 * 32 ** 3


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import default_context
    return default_context()


@pytest.fixture(scope="module")
def enc(rh):
    from roibasedimagecompression_amd.image import ImageEncoder
    return ImageEncoder(rh)


def _pixels(rh, images, maps=None, lead=1):
    """images back to back `lead` bytes into a device allocation -> (the buffer (kept alive), pointer to the first pixel, px_off host,
    px_off device, class maps device or None)"""
    import torch
    flat = np.concatenate([np.asarray(i, np.uint8).reshape(-1) for i in images])
    buf = torch.zeros(flat.size + lead + 3, dtype=torch.uint8, device=rh.device)
    buf[lead:lead + flat.size] = torch.from_numpy(flat).to(rh.device)
    off = np.concatenate([[0], np.cumsum([np.asarray(i).size // 3 for i in images])]).astype(np.int64)
    cls = None if maps is None else rh.dev(np.ascontiguousarray(np.concatenate([np.asarray(m, np.uint8).reshape(-1) for m in maps])))
    return buf, C.c_void_p(buf.data_ptr() + lead), off, rh.dev(off), cls


def _off(off):
    return C.c_void_p(off.ctypes.data)


# ---- cells -------------------------------------------------------------------------------------------------------------------------------
WEIGHTS = [0, 3, 2]


@functools.lru_cache(maxsize=None)
def cells_batch():
    """a chunk plus one pixel (the next image starts inside a chunk of the concatenation), one pixel, none, and 181 x 181 random pixels,
    with class maps over all of them -> (images, maps, the table of every image)"""
    rng = np.random.default_rng(20261102)
    images = [BC.pixel_case("chunk+1")[0], BC.pixel_case("1x1")[0], np.zeros((0, 3), np.uint8), BC.pixel_case("random_181x181")[0]]
    maps = [rng.choice(np.array([0, 1, 2, 3, 200], np.uint8), len(i)) for i in images]
    maps[1][:] = 1                                                          # (weight 3: the one pixel counts)
    return images, maps, [BC.cells_reference(i, m, 2, WEIGHTS) for i, m in zip(images, maps)]


@pytest.mark.parametrize("classes", [True, False])
def test_device_cells_batch_equals_the_per_image_reference(rh, classes):
    import torch
    images, maps, ref = cells_batch()
    buf, p_rgb, off, off_dev, cls = _pixels(rh, images, maps if classes else None)
    w = (C.c_int32 * 3)(*WEIGHTS)
    cells = torch.full((4,) + BC.SHAPE, 0x5555555555, dtype=torch.int64, device=rh.device)
    rc = rh.lib.rhccq_palette_cells_batch(rh.ctx, p_rgb, _off(off), rh._p(off_dev), 4, rh._p(cls), 2 if classes else 0,
                                          C.cast(w, C.c_void_p) if classes else C.c_void_p(0), rh._p(cells))
    assert rc == 0
    got = cells.cpu().numpy()
    for b in range(4):
        assert np.array_equal(got[b], ref[b] if classes else BC.cells_reference(images[b])), b
    # the Python surface: numpy arguments, device tables
    flat = np.concatenate(images)
    t = rh.palette_cells_batch(flat, off, np.concatenate(maps), 2, WEIGHTS) if classes else rh.palette_cells_batch(flat, off)
    assert t.is_cuda and t.dtype == torch.int64 and tuple(t.shape) == (4,) + BC.SHAPE and np.array_equal(t.cpu().numpy(), got)


def test_device_cells_batch_of_one_equals_the_single_call(rh):
    import torch
    rgb = BC.pixel_case("random_181x181")[0]
    buf, p_rgb, off, off_dev, _ = _pixels(rh, [rgb], lead=3)
    a = torch.full(BC.SHAPE, 0x5555555555, dtype=torch.int64, device=rh.device)
    b = torch.full(BC.SHAPE, 0x3333333333, dtype=torch.int64, device=rh.device)
    assert rh.lib.rhccq_palette_cells_batch(rh.ctx, p_rgb, _off(off), rh._p(off_dev), 1, C.c_void_p(0), 0, C.c_void_p(0), rh._p(a)) == 0
    assert rh.lib.rhccq_palette_cells(rh.ctx, p_rgb, len(rgb), C.c_void_p(0), 0, C.c_void_p(0), 0, rh._p(b)) == 0
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), BC.pixel_reference("random_181x181"))


def test_device_cells_batch_argument_errors(rh):
    import torch
    rgb, cells = rh.zeros((4, 3), torch.uint8), rh.zeros((2 * CELLS + 1,), torch.int64)
    off = np.array([0, 3, 4], np.int64)
    off_dev = rh.dev(off)

    def call(rgb_=rgb, off_=off, dev=off_dev, B=2, p_cells=cells.data_ptr()):
        return rh.lib.rhccq_palette_cells_batch(rh.ctx, rh._p(rgb_), _off(off_) if off_ is not None else C.c_void_p(0), rh._p(dev), B, C.c_void_p(0), 0,
                                                C.c_void_p(0), C.c_void_p(p_cells))
    assert call() == 0
    for bad, code in ((dict(B=0), E_ARG), (dict(off_=None), E_ARG), (dict(dev=None), E_ARG), (dict(off_=np.array([1, 3, 4], np.int64)), E_ARG),
                      (dict(off_=np.array([0, 3, 2], np.int64)), E_ARG), (dict(rgb_=None), E_ARG), (dict(p_cells=0), E_ARG),
                      (dict(p_cells=cells.data_ptr() + 4), E_ARG), (dict(off_=np.array([0, 3, 3 + (1 << 32)], np.int64)), E_LIMIT)):
        assert call(**bad) == code, bad
        assert rh._raw.rhccq_last_error(rh.ctx).decode().startswith("palette_cells")


# ---- build -------------------------------------------------------------------------------------------------------------------------------
def _raw_build_batch(rh, tables, K_target, want_boxes=True, want_splits=True, work="garbage"):
    """rhccq_palette_build_batch itself -> (rc, per image (k_out, palette, counts, boxes, splits)); outputs and workspace pre-filled"""
    import torch
    B = len(tables)
    d_cells = rh.dev(np.ascontiguousarray(np.stack([np.asarray(t).astype(np.uint64) for t in tables])).view(np.int64))
    nbytes = int(rh._raw.rhccq_palette_build_batch_bytes(B))
    assert nbytes == B * int(rh._raw.rhccq_palette_build_bytes())
    buf = torch.full((nbytes + 16,), 0xA7, dtype=torch.uint8, device=rh.device)
    ptr, given = buf.data_ptr(), nbytes
    if work is None:
        ptr = 0
    elif work == "odd":
        ptr += 4
    elif work == "short":
        given = nbytes - 1
    pal = torch.full((B, K_target, 3), 0xAB, dtype=torch.uint8, device=rh.device)
    counts = torch.full((B, K_target), 0x5555, dtype=torch.int64, device=rh.device)
    boxes = torch.full((B, K_target, 6), 0xCD, dtype=torch.uint8, device=rh.device) if want_boxes else None
    splits = torch.full((B, max(K_target - 1, 1), 3), 0x2B2B, dtype=torch.int32, device=rh.device) if want_splits else None
    k = torch.full((B,), 0x77, dtype=torch.int32, device=rh.device)
    rc = rh.lib.rhccq_palette_build_batch(rh.ctx, rh._p(d_cells), B, K_target, C.c_void_p(ptr), given, rh._p(pal), rh._p(counts), rh._p(boxes),
                                          rh._p(splits), rh._p(k))
    k, pal, counts = k.cpu().numpy(), pal.cpu().numpy(), counts.cpu().numpy()
    boxes = None if boxes is None else boxes.cpu().numpy()
    splits = None if splits is None else splits.cpu().numpy().reshape(B, -1)[:, :(K_target - 1) * 3].reshape(B, K_target - 1, 3)
    return rc, [(int(k[b]), pal[b], counts[b], None if boxes is None else boxes[b], None if splits is None else splits[b]) for b in range(B)]


def _same_build(got, ref, K_target):
    if ref in (E_ARG, E_LIMIT):                                             # the code in its own k_out, zero rows, -1 throughout splits
        k, pal, counts, boxes, splits = got
        assert k == ref and not pal.any() and not counts.any()
        assert (boxes is None or not boxes.any()) and (splits is None or (splits == -1).all())
    elif got[3] is not None and got[4] is not None:
        assert BC.same(got, ref, K_target)
    else:
        k, pal, counts = got[:3]
        assert k == ref["k"] and np.array_equal(pal[:k], ref["palette"]) and not pal[k:].any()
        assert np.array_equal(counts[:k], ref["counts"]) and not counts[k:].any()
    return True


K8 = 8


@functools.lru_cache(maxsize=None)
def build_tables():
    """tables of build_cases' chains around an all-zero one and one whose N adds up to 2^32 -> (tables, references at K_target = 8)"""
    tables = [BC.chain_case("three_cells_ask_8")[0], BC.chain_case("photo96_k64")[0], np.zeros(BC.SHAPE, np.int64), BC.chain_case("translated_copies")[0],
              BC.limit_table(), BC.chain_case("two_colours_one_cell")[0]]
    refs = [BC.build_reference(t, K8) for t in tables]
    assert refs[0]["k"] == 3 and refs[1]["k"] == K8 and refs[2] == E_ARG and refs[3]["k"] == K8 and refs[4] == E_LIMIT and refs[5]["k"] == 1
    return tables, refs


@pytest.mark.parametrize("optional", [True, False])
def test_device_build_batch_equals_the_per_image_reference(rh, optional):
    tables, refs = build_tables()
    rc, got = _raw_build_batch(rh, tables, K8, want_boxes=optional, want_splits=optional)
    assert rc == 0
    for b, ref in enumerate(refs):
        assert _same_build(got[b], ref, K8), b


def test_device_build_batch_of_one_and_the_python_surface(rh):
    import torch
    tables, refs = build_tables()
    rc, got = _raw_build_batch(rh, tables[1:2], K8)
    assert rc == 0 and _same_build(got[0], refs[1], K8)
    rc, got = _raw_build_batch(rh, tables[:1], 1)                           # K_target = 1: no split, an empty splits plane
    assert rc == 0 and got[0][0] == 1 and got[0][2].tolist() == [4]
    pal, counts, splits, boxes, k = rh.palette_build_batch(np.stack(tables[:4]), K8)
    assert pal.is_cuda and pal.dtype == torch.uint8 and tuple(pal.shape) == (4, K8, 3) and k.dtype == torch.int32
    assert tuple(counts.shape) == (4, K8) and tuple(splits.shape) == (4, K8 - 1, 3) and tuple(boxes.shape) == (4, K8, 6)
    for b in range(4):
        assert _same_build((int(k[b]), pal[b].cpu().numpy(), counts[b].cpu().numpy(), boxes[b].cpu().numpy(), splits[b].cpu().numpy()), refs[b], K8), b


def test_device_build_batch_of_more_chains_than_compute_units(rh):
    """300 tiny tables: more workgroups than the card has CUs, so chains queue behind one another; every one exact"""
    rng = np.random.default_rng(20261103)
    distinct = [BC.cells_reference(rng.integers(0, 256, (n, 3)).astype(np.uint8)) for n in (1, 2, 3, 5, 8, 13, 21, 34, 4, 6, 7, 40)]
    refs = [BC.build_reference(t, K8) for t in distinct]
    assert len({r["k"] for r in refs}) >= 6                                 # chains of different lengths side by side
    order = [(b * 7) % 12 for b in range(300)]
    rc, got = _raw_build_batch(rh, [distinct[j] for j in order], K8)
    assert rc == 0
    for b, j in enumerate(order):
        assert _same_build(got[b], refs[j], K8), b


@pytest.mark.parametrize("what,over,code", BC.BUILD_DEVICE_ERRORS + [("B = 0", {"B": 0}, E_ARG), ("B = 65536", {"B": 65536}, E_LIMIT)],
                         ids=[e[0] for e in BC.BUILD_DEVICE_ERRORS] + ["B = 0", "B = 65536"])
def test_device_build_batch_argument_errors(rh, what, over, code):
    import torch
    tables, _ = build_tables()
    if "B" in over:
        z = rh.zeros((2 * CELLS,), torch.int64)
        rc = rh.lib.rhccq_palette_build_batch(rh.ctx, rh._p(z), over["B"], 4, rh._p(z), 1 << 40, rh._p(z), rh._p(z), C.c_void_p(0), C.c_void_p(0), rh._p(z))
    else:
        rc, _ = _raw_build_batch(rh, tables[:2], over.get("K_target", 4), work=over.get("work", "garbage"))
    assert rc == code, what
    assert rh._raw.rhccq_last_error(rh.ctx).decode().startswith("palette_build")


# ---- remap -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def remap_batch(stride):
    """five images with k_rows = {5, stride, 1, 0, a negative code}; the rows behind k_rows[b] hold colours that occur in image b, so a
    kernel that read them would pick them -> (images, maps, palettes uint8[5, stride, 3], k_rows, references with and without classes)"""
    rng = np.random.default_rng(20261104 + stride)
    k_rows = np.array([5, stride, 1, 0, E_LIMIT], np.int32)
    sizes = [2048 + 301, 700, 67, 300, 129]
    pal = rng.integers(0, 256, (5, stride, 3)).astype(np.uint8)
    images, maps = [], []
    for b in range(5):
        k = max(int(k_rows[b]), 1)
        img = np.concatenate([RM._near(rng, pal[b, :k], sizes[b] - 40, spread=25), rng.integers(0, 256, (40, 3)).astype(np.uint8)])
        pal[b, k:] = np.resize(img, (stride - k, 3))
        images.append(img)
        maps.append(rng.integers(0, 4, sizes[b]).astype(np.uint8))
    with_cls = [RM.remap_reference(images[b], pal[b, :k_rows[b]], maps[b], 2) if k_rows[b] >= 1 else None for b in range(5)]
    without = [RM.remap_reference(images[b], pal[b, :k_rows[b]]) if k_rows[b] >= 1 else None for b in range(5)]
    assert (with_cls[0][0] != RM.remap_reference(images[0], pal[0])[0]).any()      # the padding rows would win
    return images, maps, pal, k_rows, with_cls, without


@pytest.mark.parametrize("elem,stride", [(1, 256), (2, 256), (2, RM.T + 1), (4, RM.T + 1)])
@pytest.mark.parametrize("classes", [True, False])
def test_device_remap_batch_equals_the_per_image_reference(rh, elem, stride, classes):
    import torch
    images, maps, pal, k_rows, with_cls, without = remap_batch(stride)
    buf, p_rgb, off, off_dev, cls = _pixels(rh, images, maps if classes else None)
    nc = 2 if classes else 0
    idx = torch.full((int(off[-1]),), 0x7B, dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[elem], device=rh.device)
    sums = torch.full((5, nc + 1, 2), 0x5555, dtype=torch.int64, device=rh.device)
    d_pal, d_k = rh.dev(pal), rh.dev(k_rows)
    rc = rh.lib.rhccq_palette_remap_batch(rh.ctx, p_rgb, _off(off), rh._p(off_dev), 5, rh._p(d_pal), stride, rh._p(d_k), rh._p(cls), nc, rh._p(idx), elem,
                                          rh._p(sums))
    assert rc == 0
    got = idx.cpu().numpy().view({1: np.uint8, 2: np.uint16, 4: np.uint32}[elem]).astype(np.int64)
    sums = sums.cpu().numpy()
    for b, ref in enumerate(with_cls if classes else without):
        mine = got[off[b]:off[b + 1]]
        if ref is None:                                                     # no rows: index 0 throughout, zero sums
            assert not mine.any() and not sums[b].any(), b
        else:
            assert np.array_equal(mine, ref[0]) and np.array_equal(sums[b], ref[1]), b
    if elem <= 2:                                                           # the Python surface chooses the width by the stride
        i2, s2 = rh.palette_remap_batch(np.concatenate(images), off, pal, k_rows, np.concatenate(maps) if classes else None, nc)
        assert i2.dtype == (torch.uint8 if stride <= 256 else torch.int16) and np.array_equal(s2.cpu().numpy(), sums)
        assert np.array_equal(i2.cpu().numpy().view(np.uint8 if stride <= 256 else np.uint16).astype(np.int64), got)


def test_device_remap_batch_argument_errors(rh):
    import torch
    rgb, pal, k = rh.zeros((4, 3), torch.uint8), rh.zeros((2, 300, 3), torch.uint8), rh.dev(np.array([3, 2, 0], np.int32))
    idx, sums = rh.zeros((5,), torch.int16), rh.zeros((5,), torch.int64)
    off = np.array([0, 3, 4], np.int64)
    off_dev = rh.dev(off)

    def call(B=2, dev=off_dev, K=3, p_k=k.data_ptr(), p_idx=idx.data_ptr(), elem=2, p_sums=sums.data_ptr(), off_=off):
        return rh.lib.rhccq_palette_remap_batch(rh.ctx, rh._p(rgb), _off(off_), rh._p(dev), B, rh._p(pal), K, C.c_void_p(p_k), C.c_void_p(0), 0,
                                                C.c_void_p(p_idx), elem, C.c_void_p(p_sums))
    assert call() == 0
    for bad, code in ((dict(B=0), E_ARG), (dict(dev=None), E_ARG), (dict(K=0), E_ARG), (dict(p_k=0), E_ARG), (dict(p_k=k.data_ptr() + 2), E_ARG),
                      (dict(p_idx=idx.data_ptr() + 1), E_ARG), (dict(p_sums=sums.data_ptr() + 4), E_ARG), (dict(elem=3), E_ARG),
                      (dict(K=257, elem=1), E_ARG), (dict(off_=np.array([0, 3, 2], np.int64)), E_ARG), (dict(K=65537), E_LIMIT)):
        assert call(**bad) == code, bad
        assert rh._raw.rhccq_last_error(rh.ctx).decode().startswith("palette_remap")


# ---- refine ------------------------------------------------------------------------------------------------------------------------------
REFINE_ITER = 3


@functools.lru_cache(maxsize=None)
def refine_batch(big):
    """an image whose palette is a fixed point already (one iteration), one that runs every iteration, an empty one and, with `big`, one
    of palette_refine_lds_rows() + 1 rows (the stride then puts every image's accumulators into the workspace) -> (images, maps, palettes
    uint8[B, stride, 3], k_rows, the references)"""
    from roibasedimagecompression_amd import synth
    rng = np.random.default_rng(20261105)
    photo = synth.photo(48, 64, 7).reshape(-1, 3)
    stride = RF.L + 1 if big else 40
    weights = [1, 4, 1]
    images = [photo[:2500], photo[500:3072], np.zeros((0, 3), np.uint8)]
    rows = [9, 33, 7]
    if big:
        images.append(rng.integers(0, 256, (3000, 3)).astype(np.uint8))
        rows.append(RF.L + 1)
    maps = [rng.integers(0, 3, len(i)).astype(np.uint8) for i in images]
    pal = np.full((len(images), stride, 3), 0xAB, np.uint8)
    for b, k in enumerate(rows):
        pal[b, :k] = rng.integers(0, 256, (k, 3)).astype(np.uint8) if b != 1 else images[1][rng.choice(len(images[1]), k, replace=False)]
    fixed, _, n = RF.refine_reference(images[0], pal[0, :rows[0]], maps[0], weights, 64)
    assert n < 64
    pal[0, :rows[0]] = fixed                                                # a fixed point: the first iteration changes nothing
    refs = [RF.refine_reference(images[b], pal[b, :k], maps[b], weights, REFINE_ITER) for b, k in enumerate(rows)]
    assert refs[0][2] == 1 and refs[1][2] == REFINE_ITER and refs[1][1][-1, 1] != 0 and refs[2][2] == 0
    return images, maps, pal, np.array(rows, np.int32), weights, refs


@pytest.mark.parametrize("big", [False, True], ids=["lds", "workspace"])
def test_device_refine_batch_equals_the_per_image_reference(rh, big):
    import torch
    images, maps, pal, k_rows, weights, refs = refine_batch(big)
    B, stride = len(images), pal.shape[1]
    buf, p_rgb, off, off_dev, cls = _pixels(rh, images, maps)
    d_pal, d_k = rh.dev(pal), rh.dev(k_rows)
    nbytes = int(rh._raw.rhccq_palette_refine_batch_bytes(B, stride))
    assert nbytes == B * stride * 32
    work = torch.full((nbytes + 8,), 0xA7, dtype=torch.uint8, device=rh.device)
    hist = torch.full((B, REFINE_ITER, 2), 0x5555, dtype=torch.int64, device=rh.device)
    nit = torch.full((B,), 0x77, dtype=torch.int32, device=rh.device)
    w = (C.c_int32 * 3)(*weights)

    def call(p_work=work.data_ptr(), given=nbytes, p_k=None):
        return rh.lib.rhccq_palette_refine_batch(rh.ctx, p_rgb, _off(off), rh._p(off_dev), B, rh._p(d_pal), stride, rh._p(d_k) if p_k is None else p_k,
                                                 rh._p(cls), 2, C.cast(w, C.c_void_p), REFINE_ITER, C.c_void_p(p_work), given, rh._p(hist), rh._p(nit))
    for bad in (dict(p_work=0), dict(p_work=work.data_ptr() + 4), dict(given=nbytes - 1), dict(p_k=C.c_void_p(0))):
        assert call(**bad) == E_ARG, bad
        assert rh._raw.rhccq_last_error(rh.ctx).decode().startswith("palette_refine_batch")
    assert call() == 0
    got, hist, nit = d_pal.cpu().numpy(), hist.cpu().numpy(), nit.cpu().numpy()
    for b, (want_pal, want_hist, want_n) in enumerate(refs):
        k = int(k_rows[b])
        assert nit[b] == want_n and np.array_equal(hist[b], want_hist), b
        assert np.array_equal(got[b, :k], want_pal) and np.array_equal(got[b, k:], pal[b, k:]), b
        assert (np.diff(hist[b, :want_n, 0]) <= 0).all(), b                 # E never rises
    # the Python surface returns new palettes
    p2, h2, n2 = rh.palette_refine_batch(np.concatenate(images), off, pal, k_rows, np.concatenate(maps), weights, max_iter=REFINE_ITER)
    assert np.array_equal(p2.cpu().numpy(), got) and np.array_equal(h2.cpu().numpy(), hist) and np.array_equal(n2.cpu().numpy(), nit)


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crops():
    """three crops of the committed Kodak pictures, of different sizes, the first with a ROI mask.  At colours = 300 the first two reach
    300 rows (406 and 1562 occupied cells) and the 1 x 7 strip ends with 6 (build_cases.build_reference)"""
    from PIL import Image

    def crop(n, y, x, h, w):
        img = np.asarray(Image.open(os.path.join(BC.GOLDEN, f"kodak_{n}.png")).convert("RGB"), dtype=np.uint8)
        return np.ascontiguousarray(img[y:y + h, x:x + w])
    images = [crop(1, 100, 200, 96, 128), crop(5, 50, 300, 64, 200), crop(22, 10, 10, 1, 7)]
    mask = np.zeros((96, 128), bool)
    mask[20:70, 30:101] = True
    for a in images + [mask]:
        a.setflags(write=False)
    return images, [mask, None, None]


def _same_result(a, b):
    import torch
    assert a["palette"].dtype == b["palette"].dtype and np.array_equal(a["palette"], b["palette"])
    assert a["indices"].dtype == b["indices"].dtype and tuple(a["indices"].shape) == tuple(b["indices"].shape) and torch.equal(a["indices"], b["indices"])
    assert a["indices_dtype"] == b["indices_dtype"] and a["shape"] == b["shape"] and a["top_left"] == b["top_left"]
    assert set(a["stats"]) == set(b["stats"])
    for key in a["stats"]:
        if key != "seconds":
            assert a["stats"][key] == b["stats"][key], key
    return True


@pytest.mark.parametrize("colours,refine", [(16, 0), (300, 2)])
def test_quantize_batch_equals_the_loop_of_quantize(enc, colours, refine):
    import torch
    images, masks = crops()
    loop = [enc.quantize(i, colours, refine=refine, roi_mask=m, roi_weight=4 if m is not None else 1) for i, m in zip(images, masks)]
    got = enc.quantize_batch(images, colours, refine=refine, roi_masks=masks, roi_weight=4)
    assert len(got) == 3
    for a, b in zip(got, loop):
        assert _same_result(a, b)
        assert ("refine" in a["stats"]) == bool(refine) and a["stats"]["build"]["asked"] == colours
    assert set(got[0]["stats"]["remap"]) == {"all", "roi", "nonroi"} and set(got[1]["stats"]["remap"]) == {"all"}
    if colours == 300:                                                      # one call, two index widths
        assert [r["stats"]["build"]["rows"] for r in got] == [300, 300, 6]
        assert [r["indices"].dtype for r in got] == [torch.int16, torch.int16, torch.uint8]
    again = enc.quantize_batch([enc.rh.dev(i) for i in images], colours, refine=refine, roi_masks=masks, roi_weight=4)     # device arguments
    assert all(_same_result(a, b) for a, b in zip(again, got))


def test_quantize_batch_tensor_form_and_files(enc, tmp_path):
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(BC.GOLDEN, "kodak_3.png")).convert("RGB"), dtype=np.uint8)
    frames = np.ascontiguousarray(np.stack([img[y:y + 40, x:x + 56] for y, x in ((0, 0), (100, 300), (400, 650))]))
    listed = enc.quantize_batch(list(frames), 32, refine=1)
    for form in (frames, enc.rh.dev(frames)):
        assert all(_same_result(a, b) for a, b in zip(enc.quantize_batch(form, 32, refine=1), listed))
    paths = [str(tmp_path / f"b{i}.rhccq") for i in range(3)]
    paths[1] = None
    with_files = enc.quantize_batch(frames, 32, refine=1, out_paths=paths, exact=True)
    assert all(_same_result(a, b) for a, b in zip(with_files, listed)) and not (tmp_path / "b1.rhccq").exists()
    for i in (0, 2):
        single = str(tmp_path / f"s{i}.rhccq")
        enc.quantize(frames[i], 32, refine=1, out_path=single, exact=True)
        assert open(paths[i], "rb").read() == open(single, "rb").read(), i


def test_quantize_batch_arguments(enc):
    from roibasedimagecompression_amd.ops import RhccqError
    images, masks = crops()
    for bad in (lambda: enc.quantize_batch([], 16), lambda: enc.quantize_batch(images, 0), lambda: enc.quantize_batch(images, 16, refine=65),
                lambda: enc.quantize_batch(images, 16, roi_weight=4), lambda: enc.quantize_batch(images, 16, roi_masks=masks[:2]),
                lambda: enc.quantize_batch(images, 16, out_paths=["a"]), lambda: enc.quantize_batch([images[0].astype(np.int32)], 16),
                lambda: enc.quantize_batch(images, 16, roi_masks=[masks[0][:5], None, None])):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: enc.quantize_batch(images, BC.CAP + 1), lambda: enc.quantize_batch([images[0], np.zeros((0, 5, 3), np.uint8)], 16)):
        with pytest.raises(RhccqError):
            bad()
