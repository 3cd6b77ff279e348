"""The host forms of the palette ladder (csrc/palette_ladder.hip: the device kernels' functions run serially) against numpy:
rhccq_palette_moments_host against bincount sums over the remap reference's indices, also on the search's constructed ties, rhccq_palette_curve_host against the error of
the pixels decoded through reduce_cases.reduce_reference's map and palette at every step, rhccq_palette_rung_host against
rhccq_palette_reduce_host at every target, the bound the curve is for, and the argument errors.  No GPU."""
import numpy as np
import pytest

import ladder_cases as LD
import reduce_cases as RD
import remap_cases as RM


def test_sizes_are_exported():
    from roibasedimagecompression_amd import _lib, ops
    lib = _lib.load()
    rows = [ops.palette_moments_lds_rows(n) for n in range(17)]
    assert all(x > y for x, y in zip(rows, rows[1:])) and rows[16] >= 1
    # (tables x K x 40 bytes) beside the 8 KiB tile within the 64 KiB a workgroup gets without an opt-in, and no row to spare
    assert all(r * 40 * (n + 1) + RM.T * 8 <= 64 * 1024 < (r + 1) * 40 * (n + 1) + RM.T * 8 + 1024 + 40 * (n + 1) for n, r in enumerate(rows))
    assert lib.rhccq_palette_moments_lds_rows(-1) == 0 and lib.rhccq_palette_moments_lds_rows(17) == 0
    assert lib.rhccq_palette_curve_bytes(3, 1) == (3 * 5 + 9) * 8 and lib.rhccq_palette_curve_bytes(0, 1) == 0 == lib.rhccq_palette_curve_bytes(3, 18)


@pytest.mark.parametrize("name", LD.names(pixels=False))
def test_moments_equal_bincount_sums(name):
    c = LD.case(name)
    want_idx, want_mom, _ = LD.reference(name)
    for width in (None,) + RM.index_bytes(len(c["pal"])):
        rc, idx, mom = LD.host_moments(c["rgb"], c["pal"], c["cls"], c["n_classes"], width)
        assert rc == 0, (name, width)
        assert np.array_equal(mom, want_mom), (name, width)
        assert (idx is None) == (width is None) and (idx is None or np.array_equal(idx, want_idx)), (name, width)
    n = c["rgb"].size // 3
    assert int(want_mom[-1, :, 0].sum()) == n and (n > 0 or not want_mom.any())
    if c["n_classes"] == 16:                                                    # values >= n_classes are in the last table alone
        assert int(want_mom[:-1, :, 0].sum()) < n


@pytest.mark.parametrize("name", LD.TIE_NAMES)
def test_moments_keep_the_lowest_row_on_a_tie(name):
    """the search's constructed ties, inside a tile and across a tile boundary: every legal index width and no index buffer"""
    c = LD.case(name)
    want_idx, want_mom, _ = LD.reference(name)
    assert want_idx.tolist() == c["expect"]
    for width in (None,) + RM.index_bytes(len(c["pal"])):
        rc, idx, mom = LD.host_moments(c["rgb"], c["pal"], None, 0, width)
        assert rc == 0, (name, width)
        assert np.array_equal(mom, want_mom), (name, width)
        assert (idx is None) == (width is None) and (idx is None or idx.tolist() == c["expect"]), (name, width)


def test_the_flat_cases_have_one_winner():
    for name in ("flat_K3", "flat_K3_roi7"):
        idx, mom, _ = LD.reference(name)
        assert (idx == 1).all() and (mom[-1, [0, 2]] == 0).all()


@pytest.mark.parametrize("name", LD.names())
def test_curve_equals_the_decoded_error_of_the_reduction(name):
    """curve[t][s] against the pixels shown through reduce_reference(target = rows in use - s)'s map and palette"""
    c = LD.case(name)
    idx, _, want_counts = LD.reference(name)
    counts, merges, curve, live = LD.host_ladder(name)
    assert np.array_equal(counts, want_counts)
    for s in LD.steps_to_check(live):
        pal, _, map_, ref_merges, k = RD.reduce_reference(c["pal"], counts, live - s)
        assert k == live - s and np.array_equal(ref_merges[:s], merges[:s])
        assert np.array_equal(curve[:, s], LD.decode_sse(c, idx, map_, pal)), (name, s)
    assert not curve[:, live:].any() and (curve >= 0).all()
    if name == "37x53_K300_roi7":                                               # the tables of a mask add up
        assert np.array_equal(curve[0] + curve[1], curve[2])


@pytest.mark.parametrize("name", LD.names())
def test_rung_equals_the_reduction(name):
    c = LD.case(name)
    K = len(c["pal"])
    counts, merges, _, live = LD.host_ladder(name)
    targets = range(1, K + 1) if K <= RD.NAIVE_MAX_K else sorted({1, 2, 3, live - 1, live, live + 1, K // 2, K - 1, K})
    for k in targets:
        if not 1 <= k <= K:
            continue
        rc, pal, cnt, map_, _, k_out = LD.host_reduce(c["pal"], counts, k)
        got = LD.host_rung(c["pal"], counts, merges, k)
        assert rc == 0 and got[0] == 0 and got[4] == k_out == min(k, live), (name, k)
        assert np.array_equal(got[1], pal) and np.array_equal(got[2], cnt) and np.array_equal(got[3], map_), (name, k)


def test_a_log_that_ends_early_gives_the_clusters_it_has():
    c = LD.case("37x53_K300_roi7")
    counts, merges, _, live = LD.host_ladder("37x53_K300_roi7")
    short = merges.copy()
    short[10:] = -1
    rc, pal, cnt, map_, k = LD.host_rung(c["pal"], counts, short, 5)
    want = LD.host_reduce(c["pal"], counts, live - 10)
    assert rc == 0 and k == live - 10 and np.array_equal(map_, want[3]) and np.array_equal(pal, want[1][:5]) and np.array_equal(cnt, want[2][:5])


@pytest.mark.parametrize("name", ["37x53_K300_roi7", "3x2731_K64_roi1"])
def test_curve_bounds_the_remap_onto_every_rung(name):
    """the nearest-row remap onto rung k can only lower the error the curve states for it, in every table"""
    c = LD.case(name)
    counts, merges, curve, live = LD.host_ladder(name)
    masks = LD.table_masks(c)
    px = c["rgb"].reshape(-1, 3).astype(np.int64)
    strict = 0
    for k in range(1, live + 1):
        rc, pal, _, _, k_out = LD.host_rung(c["pal"], counts, merges, k)
        assert rc == 0 and k_out == k
        idx, sums = RM.remap_reference(c["rgb"], pal[:k])
        d = ((px - pal[:k].astype(np.int64)[idx]) ** 2).sum(axis=1)
        got = np.array([int(d[m].sum()) for m in masks])
        assert got[-1] == int(sums[-1, 1]) and (got <= curve[:, live - k]).all(), (name, k)
        strict += int(got[-1] < curve[-1, live - k])
    assert strict > 0                                                           # and the bound is not trivially the remap's own sum


def _moments_error_call(over):
    from roibasedimagecompression_amd import _lib
    rgb, pal = np.zeros((4, 3), np.uint8), np.arange(9, dtype=np.uint8).reshape(3, 3)
    cls = np.zeros(4, np.uint8) if over.get("cls") else None
    idx, mom = np.zeros(6, np.uint16), np.zeros(2 * 3 * 5 + 1, np.uint64)
    p = {"rgb": LD.ptr(rgb), "palette": LD.ptr(pal), "idx_out": LD.ptr(idx, 1 if over.get("misalign") == "idx_out" else 0),
         "moments": LD.ptr(mom, 1 if over.get("misalign") == "moments" else 0)}
    for k in p:
        if k in over and over[k] is None:
            p[k] = LD.ptr(None)
    return _lib.load().rhccq_palette_moments_host(p["rgb"], over.get("n_pixels", 4), p["palette"], over.get("K", 3), LD.ptr(cls), over.get("n_classes", 0),
                                                  p["idx_out"], over.get("idx_elem_bytes", 2), p["moments"])


@pytest.mark.parametrize("what,over,code", LD.MOMENTS_ERRORS, ids=[e[0] for e in LD.MOMENTS_ERRORS])
def test_moments_argument_errors(what, over, code):
    assert _moments_error_call(over) == code, what


@pytest.mark.parametrize("what,over", LD.MOMENTS_ACCEPTED, ids=[e[0] for e in LD.MOMENTS_ACCEPTED])
def test_moments_accepts(what, over):
    assert _moments_error_call(over) == 0, what


def _chain_bufs():
    return {"palette": np.arange(9, dtype=np.uint8).reshape(3, 3), "counts": np.array([1, 2, 3, 0], np.uint64),
            "merges": np.array([[0, 1], [-1, -1], [-1, -1]], np.int32), "moments": np.ones(3 * 5 + 1, np.uint64), "curve": np.zeros(4, np.uint64),
            "palette_out": np.zeros((4, 3), np.uint8), "counts_out": np.zeros(5, np.uint64), "map": np.zeros(4, np.int32), "k_out": np.zeros(2, np.int32)}


def _pointers(bufs, over):
    out = {}
    for k, a in bufs.items():
        off = (1 if a.itemsize == 8 else 2) if over.get("misalign") == k else 0
        out[k] = LD.ptr(None) if k in over and over[k] is None else LD.ptr(a, off)
    return out


_HOST_CURVE = [e for e in LD.CURVE_ERRORS if e[3] == "both"]
_HOST_RUNG = [e for e in LD.RUNG_ERRORS if e[3] == "both"]


@pytest.mark.parametrize("what,over,code", [e[:3] for e in _HOST_CURVE], ids=[e[0] for e in _HOST_CURVE])
def test_curve_argument_errors(what, over, code):
    from roibasedimagecompression_amd import _lib
    p = _pointers(_chain_bufs(), over)
    fn = _lib.load().rhccq_palette_curve_host
    assert fn(p["palette"], p["counts"], over.get("K", 3), p["merges"], p["moments"], over.get("n_tables", 1), p["curve"]) == code, what


@pytest.mark.parametrize("what,over,code", [e[:3] for e in _HOST_RUNG], ids=[e[0] for e in _HOST_RUNG])
def test_rung_argument_errors(what, over, code):
    from roibasedimagecompression_amd import _lib
    p = _pointers(_chain_bufs(), over)
    fn = _lib.load().rhccq_palette_rung_host
    assert fn(p["palette"], p["counts"], over.get("K", 3), p["merges"], over.get("K_target", 2), p["palette_out"], p["counts_out"], p["map"],
              p["k_out"]) == code, what


def test_the_valid_calls_succeed():
    from roibasedimagecompression_amd import _lib
    lib, b = _lib.load(), _chain_bufs()
    p = _pointers(b, {})
    assert lib.rhccq_palette_curve_host(p["palette"], p["counts"], 3, p["merges"], p["moments"], 1, p["curve"]) == 0
    assert lib.rhccq_palette_rung_host(p["palette"], p["counts"], 3, p["merges"], 2, p["palette_out"], p["counts_out"], p["map"], p["k_out"]) == 0
    assert b["k_out"][0] == 2 and b["map"][:3].tolist() == [0, 0, 1] and b["counts_out"][:2].tolist() == [3, 3]
    assert b["curve"][2] == 0 and b["curve"][3] == 0                             # behind the one step; past the array untouched


@pytest.mark.parametrize("what,counts,code", LD.RUNG_DATA_ERRORS, ids=[e[0] for e in LD.RUNG_DATA_ERRORS])
def test_rung_data_errors(what, counts, code):
    assert LD.host_rung(np.zeros((3, 3), np.uint8), counts, [[0, 1], [-1, -1]], 2)[0] == code, what


def test_device_entry_points_raise_without_a_gpu():
    """no CPU fallback: ImageEncoder.ladder and the target keywords need the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError
    from roibasedimagecompression_amd.image import ImageEncoder
    img = np.zeros((4, 4, 3), np.uint8)
    img[2:] = 200
    pal = np.array([[0, 0, 0], [200, 200, 200], [201, 200, 200]], np.uint8)
    if torch.cuda.is_available():
        assert ImageEncoder().ladder(img, pal)["colours"] == [2, 1]
    else:
        with pytest.raises(RhccqError):
            ImageEncoder().ladder(img, pal)
        with pytest.raises(RhccqError):
            ImageEncoder().encode_with_palette(img, pal, target_psnr=30.0)
