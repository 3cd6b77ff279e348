"""rhccq_palette_segment_host (the device kernel's step functions run serially: csrc/palette_segment.h, csrc/palette_segment.hip) against
the numpy reference of tests/segment_cases.py, bit for bit: indices in every element width, the four sum columns, the properties the
rule implies, argument errors, and the value claim on a shipped artefact.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import remap_cases as RM
import segment_cases as SG

_DT = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def host_segment(rgb, pal, cls, n_classes, penalty, elem_bytes):
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    rgb = np.ascontiguousarray(rgb, np.uint8)
    H, W = rgb.shape[:2]
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 3)
    cls = None if cls is None else np.ascontiguousarray(cls, np.uint8).reshape(-1)
    table = np.array(SG.penalty_table(penalty, n_classes), np.uint32)
    idx = np.full(max(H * W, 1), 0xAB, _DT[elem_bytes])
    sums = np.full((n_classes + 1, 4), 0x5555, np.uint64)                  # (the call zeroes them)
    rc = lib.rhccq_palette_segment_host(_ptr(rgb if rgb.size else np.zeros(3, np.uint8)), H, W, _ptr(pal), len(pal), _ptr(cls), n_classes,
                                        _ptr(table), _ptr(idx), elem_bytes, _ptr(sums))
    return rc, idx[:H * W].astype(np.int64).reshape(H, W), sums.astype(np.int64)


def test_cap_and_tile_are_exported():
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    assert SG.CAP == 1024 and SG.COLS == 32
    assert lib.rhccq_palette_segment_bytes(2160, 3840, 230) == 2160 * 120 * (8 * 4 + 2) * 32        # (8 S + 2) bytes a pixel, S = 4
    assert lib.rhccq_palette_segment_bytes(1, 33, 65) == 2 * (8 * 2 + 2) * 32
    assert lib.rhccq_palette_segment_bytes(1, 1, SG.CAP + 1) == 0 and lib.rhccq_palette_segment_bytes(0, 5, 3) == 0


@pytest.mark.parametrize("name", SG.names())
def test_host_equals_reference(name):
    rgb, pal, cls, nc, penalty, _ = SG.case(name)
    want_out, want_sums, _ = SG.reference(name)
    for eb in SG.index_bytes(len(pal)):
        rc, out, sums = host_segment(rgb, pal, cls, nc, penalty, eb)
        assert rc == 0, (name, eb)
        assert np.array_equal(out, want_out), (name, eb)
        assert np.array_equal(sums, want_sums), (name, eb)


def test_host_form_takes_a_palette_above_the_device_cap():
    rng = np.random.default_rng(5)
    pal = RM._palette(rng, SG.CAP + 77)
    rgb = SG.RN._image(rng, pal, 3, 41, spread=15)
    want_out, want_sums, _ = SG.segment_reference(rgb, pal, 250)
    rc, out, sums = host_segment(rgb, pal, None, 0, 250, 2)
    assert rc == 0 and np.array_equal(out, want_out) and np.array_equal(sums, want_sums)


def test_larger_penalty_never_more_breaks_nor_less_error():
    SG.check_monotone(lambda rgb, pal, p: host_segment(rgb, pal, None, 0, p, 1)[1])


def test_segmentation_never_crosses_image_rows():
    """two image rows of one colour each, far apart: at the largest penalty the second row still takes its own row"""
    pal = np.array([[0, 0, 0], [255, 255, 255]], np.uint8)
    rgb = np.zeros((2, SG.COLS + 1, 3), np.uint8)
    rgb[1] = 255
    rc, out, sums = host_segment(rgb, pal, None, 0, SG.MAX_PENALTY, 1)
    assert rc == 0 and (out[0] == 0).all() and (out[1] == 1).all() and sums.tolist() == [[2 * (SG.COLS + 1), 0, 0, 0]]


@pytest.mark.parametrize("name,expect", [("tie_stays", [[1, 1, 1]]), ("one_above_the_tie", [[0, 1, 1]]), ("last_column_tie", [[0, 0]])])
def test_hand_written_ties(name, expect):
    rgb, pal, _, _, penalty, _ = SG.case(name)
    rc, out, sums = host_segment(rgb, pal, None, 0, penalty, 1)
    assert rc == 0 and out.tolist() == expect
    assert sums[0, 3] == sum(int(r[i] != r[i - 1]) for r in expect for i in range(1, len(r)))


@pytest.mark.parametrize("what,over,code", SG.ERRORS, ids=[e[0] for e in SG.ERRORS])
def test_host_argument_errors(what, over, code):
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    rgb, pal = np.zeros((4, 3), np.uint8), np.zeros((3, 3), np.uint8)
    cls = np.zeros(4, np.uint8) if over.get("cls") else None
    idx, sums = np.zeros(4, np.uint32), np.zeros((18, 4), np.uint64)
    penalty = over.get("penalty", [5])
    table = None if penalty is None else np.array(penalty, np.uint32)
    a = {"rgb": rgb, "palette": pal, "idx_out": idx, "sums": sums}
    a.update({k: v for k, v in over.items() if k in a})
    rc = lib.rhccq_palette_segment_host(_ptr(a["rgb"]), over.get("H", 2), over.get("W", 2), _ptr(a["palette"]), over.get("K", 3), _ptr(cls),
                                        over.get("n_classes", 0), _ptr(table), _ptr(a["idx_out"]), over.get("idx_elem_bytes", 2), _ptr(a["sums"]))
    assert rc == code, what


def test_host_accepts_the_valid_call_the_errors_vary():
    """the call every error case changes one argument of succeeds, with and without its class map; no pixels: zero sums"""
    rc, out, sums = host_segment(np.zeros((2, 2, 3), np.uint8), np.zeros((3, 3), np.uint8), None, 0, [5], 2)
    assert rc == 0 and out.tolist() == [[0, 0], [0, 0]] and sums.tolist() == [[4, 0, 0, 0]]
    rc, out, sums = host_segment(np.zeros((2, 2, 3), np.uint8), np.zeros((3, 3), np.uint8), np.array([0, 1, 255, 1], np.uint8), 2, [0, SG.MAX_PENALTY, 5], 2)
    assert rc == 0 and sums.tolist() == [[1, 0, 0, 0], [2, 0, 0, 0], [4, 0, 0, 0]]
    for h, w in ((0, 0), (0, 5), (5, 0)):
        rc, out, sums = host_segment(np.zeros((h, w, 3), np.uint8), np.zeros((3, 3), np.uint8), None, 0, [5], 1)
        assert rc == 0 and sums.tolist() == [[0, 0, 0, 0]], (h, w)


def test_value_claim_on_kodak_22():
    """the reference alone: on kodak_22 with the 139 rows of compressed_22.rhccq, penalty 128 against the greedy run-carrying map at
    slack 128: zlib-9 index bytes at most 0.93 x the greedy map's (132 767 / 147 253 = 0.902 in the numpy trial that proposed the rule)
    and a squared error no larger (29 513 667 against 30 601 885)"""
    img, pal, b, out, sums, greedy, greedy_sums = SG.kodak()
    seg_bytes, greedy_bytes = SG.index_bytes_zlib9(out), SG.index_bytes_zlib9(greedy)
    print(f"kodak_22: greedy {greedy_bytes} B, SSE {int(greedy_sums[-1, 1])}; segmentation {seg_bytes} B ({seg_bytes / greedy_bytes:.4f}), SSE {int(sums[-1, 1])}")
    assert seg_bytes <= SG.KODAK_MAX_BYTES_RATIO * greedy_bytes
    assert int(sums[-1, 1]) <= int(greedy_sums[-1, 1])


def test_host_equals_reference_on_kodak_22():
    img, pal, _, out, sums, _, _ = SG.kodak()
    rc, got, got_sums = host_segment(img, pal, None, 0, SG.KODAK_PENALTY, 1)
    assert rc == 0 and np.array_equal(got, out) and np.array_equal(got_sums, sums)


def test_device_entry_point_raises_without_a_gpu():
    """no CPU fallback: Rhccq.palette_segment and encode_with_palette(run_penalty=) need the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError
    from roibasedimagecompression_amd.image import ImageEncoder

    def run():
        return ImageEncoder().encode_with_palette(np.zeros((4, 4, 3), np.uint8), np.zeros((1, 3), np.uint8), run_penalty=0)
    if torch.cuda.is_available():
        assert run()["stats"]["runs"] == {"penalty": 0, "carried": {"all": 0}, "breaks": {"all": 0}, "pixels": 16}
    else:
        with pytest.raises(RhccqError):
            run()
