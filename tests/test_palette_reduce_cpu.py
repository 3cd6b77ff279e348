"""rhccq_palette_reduce_host (the device kernels' key / compare / scan / merge functions run serially: csrc/palette_reduce.hip)
against the numpy reference of tests/reduce_cases.py, bit for bit: palette_out, counts_out, map, merges, k_out; the argument errors;
the exported sizes; and the invariants of the definition.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import reduce_cases as RD


def _ptr(a, off=0):
    return C.c_void_p(a.ctypes.data + off) if a is not None else C.c_void_p(0)


def host_reduce(pal, counts, target, want_merges=True):
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    pal = np.ascontiguousarray(pal, np.uint8).reshape(-1, 3)
    counts = np.ascontiguousarray(counts, np.uint64)
    K = len(pal)
    pal_out = np.full((target, 3), 0x55, np.uint8)                           # (the call writes every element)
    cnt_out = np.full(target, 0x5555, np.uint64)
    map_ = np.full(K, -7, np.int32)
    merges = np.full((max(K - 1, 1), 2), -7, np.int32) if want_merges else None
    k_out = np.full(1, -7, np.int32)
    rc = lib.rhccq_palette_reduce_host(_ptr(pal), _ptr(counts), K, target, _ptr(pal_out), _ptr(cnt_out), _ptr(map_), _ptr(merges), _ptr(k_out))
    return rc, pal_out, cnt_out.astype(np.int64), map_, None if merges is None else merges[:K - 1], int(k_out[0])


def test_sizes_are_exported():
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    assert RD.CAP >= 4096 and RD.CAP >= RD.BLOCK
    sizes = [lib.rhccq_palette_reduce_bytes(K) for K in (1, 2, 3, 255, 256, 257, RD.CAP - 1, RD.CAP, 65536)]
    assert sizes[0] >= 24 + 8 + 2 and all(b % 8 == 0 for b in sizes) and all(x < y for x, y in zip(sizes, sizes[1:]))
    assert lib.rhccq_palette_reduce_bytes(0) == 0 and lib.rhccq_palette_reduce_bytes(-3) == 0


@pytest.mark.parametrize("name", RD.names())
def test_host_equals_reference(name):
    c = RD.case(name)
    want_pal, want_cnt, want_map, want_merges, want_k = RD.reference(name)
    rc, pal, cnt, map_, merges, k = host_reduce(c["pal"], c["counts"], c["target"])
    assert rc == 0 and k == want_k, name
    assert np.array_equal(merges, want_merges), (name, merges[:8].tolist(), want_merges[:8].tolist())
    assert np.array_equal(pal, want_pal) and np.array_equal(cnt, want_cnt) and np.array_equal(map_, want_map), name
    rc, pal2, cnt2, map2, none, k2 = host_reduce(c["pal"], c["counts"], c["target"], want_merges=False)      # merges == NULL
    assert rc == 0 and none is None and k2 == k and np.array_equal(pal2, pal) and np.array_equal(cnt2, cnt) and np.array_equal(map2, map_)


@pytest.mark.parametrize("name", RD.names())
def test_invariants(name):
    """The weight is kept, the map is onto the output rows over the non-empty rows, and a row nothing merged into keeps its bytes.
    Reducing to K_target and then further does NOT have to equal reducing directly: the second run starts from the rounded centres
    and its sums are n * centre, not the sums of the original rows.  What does hold is that the merge order does not depend on the
    target: the steps of this run are a prefix of the steps of the run to 1."""
    c = RD.case(name)
    K, counts = len(c["pal"]), c["counts"].astype(np.int64)
    rc, pal, cnt, map_, merges, k = host_reduce(c["pal"], c["counts"], c["target"])
    assert rc == 0
    live = counts > 0
    assert k == min(c["target"], int(live.sum())) and int(cnt.sum()) == int(counts.sum()) and (cnt[:k] > 0).all()
    assert not pal[k:].any() and not cnt[k:].any()
    assert (map_[~live] == -1).all() and sorted(set(map_[live].tolist())) == list(range(k))
    assert np.array_equal(np.array([counts[live][map_[live] == i].sum() for i in range(min(k, 64))]), cnt[:min(k, 64)])
    alone = np.nonzero(np.bincount(map_[live], minlength=k) == 1)[0]
    src = np.nonzero(live)[0]
    for i in alone[:64]:
        j = src[map_[live] == i][0]
        assert np.array_equal(pal[i], c["pal"][j]) and cnt[i] == counts[j], (name, i, j)
    steps = int(live.sum()) - k
    assert (merges[:steps] >= 0).all() and (merges[:steps, 0] < merges[:steps, 1]).all() and (merges[steps:] == -1).all()
    assert (np.diff(np.unique(map_[live], return_index=True)[1]) > 0).all()          # ascending id order: a cluster's id is its lowest row
    rc, _, _, _, to_one, _ = host_reduce(c["pal"], c["counts"], 1)
    assert rc == 0 and np.array_equal(to_one[:steps], merges[:steps]), name


def test_two_stage_reduction_differs_from_the_direct_one():
    """the statement of test_invariants' docstring on a case where it shows: 300 -> 64 -> 16 restarts from the rounded centres of the
    64 clusters (sums n * centre instead of the original rows' sums), and its 16 rows are not those of 300 -> 16"""
    c = RD.case("K300_to_16")
    _, pal64, cnt64, _, _, k64 = host_reduce(c["pal"], c["counts"], 64)
    _, pal16, cnt16, _, _, _ = host_reduce(pal64[:k64], cnt64[:k64], 16)
    _, direct, dcnt, _, _, _ = host_reduce(c["pal"], c["counts"], 16)
    assert np.array_equal(direct, RD.reference("K300_to_16")[0])
    assert int(cnt16.sum()) == int(dcnt.sum()) == int(c["counts"].sum())
    assert not np.array_equal(pal16, direct)


def _error_call(over, fn, device):
    """the valid call of reduce_cases.ERRORS with `over` applied; host memory (the device test has its own)"""
    K = RD.ERROR_K
    bufs = {"palette": np.arange(3 * K, dtype=np.uint8).reshape(K, 3), "counts_buf": np.zeros(K + 1, np.uint64),
            "palette_out": np.zeros((K + 1, 3), np.uint8), "counts_out": np.zeros(K + 2, np.uint64), "map": np.zeros(K + 1, np.int32),
            "merges": np.zeros((K, 2), np.int32), "k_out": np.zeros(2, np.int32)}
    bufs["counts_buf"][:K] = np.array(over.get("counts", [1, 2, 3]), np.uint64)
    for k in list(bufs):
        if k in over:
            bufs[k] = over[k]
    off = {k: 0 for k in bufs}
    if over.get("misalign") in off:
        off[over["misalign"]] = 1 if over["misalign"] in ("counts_buf", "counts_out") else 2
    rc = fn(_ptr(bufs["palette"]), _ptr(bufs["counts_buf"], off["counts_buf"]), over.get("K", K), over.get("K_target", 2),
            _ptr(bufs["palette_out"]), _ptr(bufs["counts_out"], off["counts_out"]), _ptr(bufs["map"], off["map"]),
            _ptr(bufs["merges"], off["merges"]), _ptr(bufs["k_out"], off["k_out"]))
    return rc, bufs


_HOST_ERRORS = [e for e in RD.ERRORS if e[3] != "device"]


@pytest.mark.parametrize("what,over,code", [e[:3] for e in _HOST_ERRORS], ids=[e[0] for e in _HOST_ERRORS])
def test_host_argument_errors(what, over, code):
    from roibasedimagecompression_amd import _lib
    assert _error_call(over, _lib.load().rhccq_palette_reduce_host, False)[0] == code, what


@pytest.mark.parametrize("what,over", RD.ACCEPTED, ids=[a[0] for a in RD.ACCEPTED])
def test_host_accepts(what, over):
    from roibasedimagecompression_amd import _lib
    rc, bufs = _error_call(over, _lib.load().rhccq_palette_reduce_host, False)
    assert rc == 0 and bufs["k_out"][0] == over.get("K_target", 2), what


def test_host_takes_more_rows_than_the_device_form():
    """K = 65536, the host form's limit, with three rows of weight"""
    pal = np.zeros((65536, 3), np.uint8)
    pal[[5, 40000, 65535]] = [[10, 0, 0], [11, 0, 0], [200, 0, 0]]
    counts = np.zeros(65536, np.uint64)
    counts[[5, 40000, 65535]] = [1, 1, 4]
    rc, out, cnt, map_, merges, k = host_reduce(pal, counts, 2)
    assert rc == 0 and k == 2 and out.tolist() == [[11, 0, 0], [200, 0, 0]] and cnt.tolist() == [2, 4]
    assert merges[0].tolist() == [5, 40000] and (merges[1:] == -1).all() and map_[[5, 40000, 65535]].tolist() == [0, 0, 1] and (map_ == -1).sum() == 65533


def test_device_entry_points_raise_without_a_gpu():
    """no CPU fallback: Rhccq.palette_reduce and encode_with_palette(colours=N) need the device"""
    import torch
    from roibasedimagecompression_amd import RhccqError
    from roibasedimagecompression_amd.image import ImageEncoder

    def run():
        img = np.zeros((4, 4, 3), np.uint8)
        img[2:] = 200
        return ImageEncoder().encode_with_palette(img, np.array([[0, 0, 0], [200, 200, 200], [201, 200, 200]], np.uint8), colours=2)
    if torch.cuda.is_available():
        out = run()
        assert out["palette"].tolist() == [[0, 0, 0], [200, 200, 200]] and out["stats"]["reduce"] == {"from": 3, "to": 2, "empty": 1, "steps": 0}
    else:
        with pytest.raises(RhccqError):
            run()
