"""CPU-side checks of the boundary: the C-ABI library loads and exports every symbol include/rhccq.h
declares; host-only entry points agree with the oracle; the mirror modules import under the
reference's names; the container code (host side) is byte-exact against the reference's files."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_header_symbols_exported_and_bound():
    from roibasedimagecompression_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rhccq.h")).read()
    declared = set(re.findall(r"\b(rhccq_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"rhccq_ctx", "rhccq_mbk_problem"}
    lib = _lib.load()
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/rhccq.h but not exported"
        assert name in _lib.PROTOTYPES, f"{name} has no ctypes prototype"
    assert set(_lib.PROTOTYPES) <= declared
    assert lib.rhccq_abi_version() == 1


def test_params_and_eps_threshold_match_oracle():
    from oracle import rhccq_oracle as O
    from roibasedimagecompression_amd import ops
    for n, q, eps_hex, ms, mc in json.load(open(os.path.join(G, "g2_params.json"))):
        e, m, c = ops.clustering_params(n, q)
        assert float(e).hex() == eps_hex and m == ms and c == mc
    with pytest.raises(ZeroDivisionError):
        ops.clustering_params(10, 0)
    for q in list(range(1, 101)) + [12.5, 33.3]:
        eps = 128 - 1.28 * q
        if eps == 0:
            eps = 1
        thr, bnd, r2 = ops.eps_threshold(eps)
        assert (thr, bnd) == O.eps_threshold(eps)
        assert r2 == (np.float64(eps) / np.float64(255.0)) ** 2
    for eps in (1.0, 3.0, 32.0, 64.0, 96.0, 12.8, 0.5):
        assert ops.eps_threshold(eps)[:2] == O.eps_threshold(eps)


def test_no_cpu_fallback_without_gpu():
    import torch
    from roibasedimagecompression_amd import RhccqError
    from roibasedimagecompression_amd.ops import Rhccq
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RhccqError):
        Rhccq(0)


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "roibasedimagecompression_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, os.path.join(d, f)
    for top in ("encoder", "decoder"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(".py"):
                    assert "oracle" not in open(os.path.join(d, f)).read()


def test_reference_import_surface():
    from encoder.compression.clustering import compute_clustering_params, cluster_palette_colors_parallel, get_all_unique_colors  # noqa: F401
    from encoder.compression.merging import merge_region_components_simple, visualize_merged_result  # noqa: F401
    from encoder.compression.subregions import subregion_quantization  # noqa: F401
    from encoder.compression.regions import region_quantization  # noqa: F401
    from encoder.compression.image import quantize_image  # noqa: F401
    from encoder.compression.compression import (save_compressed, compress_palette, compress_indices_simple_optimized,  # noqa: F401
                                                 lossless_compress_optimized, optimize_compressed_dtype)
    from decoder.uncompression.uncompression import (lossless_decompress, load_compressed, decompress_color_quantization,  # noqa: F401
                                                     partial_decompress_color_quantization)
    from encoder.ROI.edges import compute_local_density, suggest_automatic_threshold, get_edge_map  # noqa: F401
    from encoder.ROI.roi import extract_regions, extract_roi_nonroi  # noqa: F401
    from encoder.subregions.split_score import calculate_split_score, normalize_result  # noqa: F401
    from encoder.subregions.slic import visualize_split_analysis, enhanced_slic_with_texture, extract_slic_segment_boundaries  # noqa: F401
    from encoder.enhancer.clahe import get_enhanced_image  # noqa: F401
    assert compute_clustering_params(2274, 20, color_space="lab") == (102.4, 1, 91)
    assert get_all_unique_colors(np.zeros((0, 0, 3), np.uint8), (0, 0)) is None
    assert merge_region_components_simple([], (0, 0, 4, 4)) == []
    from encoder.ROI.roi import get_regions, process_and_unify_borders, visualize_roi_nonroi_comparison
    from encoder.ROI.small_regions import remove_small_regions, connect_by_closing_fast, connect_nearby_pixels
    from encoder.ROI.small_gaps import bridge_small_gaps_fast, bridge_small_gaps
    from encoder.ROI.thin_regions2 import remove_thin_structures_optimized
    assert extract_regions.__module__ == "roibasedimagecompression_amd.api.roi" and extract_roi_nonroi.__module__ == extract_regions.__module__
    assert get_edge_map.__module__ == "roibasedimagecompression_amd.api.edges" and compute_local_density.__module__ == get_edge_map.__module__
    for fn in (get_regions, process_and_unify_borders, remove_small_regions, connect_by_closing_fast, bridge_small_gaps_fast, remove_thin_structures_optimized):
        assert fn.__module__ == "roibasedimagecompression_amd.api.roi_chain"
    for helper in (visualize_roi_nonroi_comparison, connect_nearby_pixels, bridge_small_gaps):   # matplotlib / unused variants: the reference's own
        with pytest.raises(NotImplementedError):
            helper(None)
    assert calculate_split_score.__module__ == "roibasedimagecompression_amd.api.split_score"
    assert enhanced_slic_with_texture.__module__ == "roibasedimagecompression_amd.api.slic"
    with pytest.raises(NotImplementedError):
        visualize_split_analysis(None, 0, 0, 0, 1)          # matplotlib helper: the reference's own, when it is on sys.path


def test_reference_tree_behind_the_repository_is_not_shadowed(tmp_path):
    """INTEGRATION.md section 1 "shadow on PYTHONPATH": with this repository FIRST on sys.path and a reference checkout behind
    it, the hot-path modules resolve here while every other module of `encoder` / `decoder` (stages this build does not
    replace, files it does not know) resolves to the reference's own file -- placeholders step aside."""
    import subprocess
    import textwrap
    ref = tmp_path / "reference"
    for d in ("encoder/ROI", "encoder/subregions", "encoder/enhancer", "decoder/uncompression", "other"):
        (ref / d).mkdir(parents=True)
    (ref / "encoder/ROI/small_gaps.py").write_text("def bridge_small_gaps(*a):\n    return 'reference small_gaps'\n")
    (ref / "encoder/ROI/brand_new.py").write_text("VALUE = 41\n")
    (ref / "encoder/enhancer/clahe.py").write_text("def get_enhanced_image(*a):\n    return 'reference clahe'\n")
    (ref / "decoder/uncompression/comparison.py").write_text("def plot_comparison(*a):\n    return 'reference plot'\n")
    (ref / "encoder/compression").mkdir()
    (ref / "encoder/compression/clustering.py").write_text("raise RuntimeError('the hot-path module must come from the repository')\n")
    (ref / "encoder/compression/image.py").write_text("def fill_black_holes_vectorized(*a):\n    return 'reference filler'\n"
                                                      "def quantize_image(*a, **k):\n    return 'reference quantize_image'\n")
    (ref / "other/jpeg.py").write_text("Q = 3\n")
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r}); sys.path.append({str(ref)!r})
        from encoder.ROI.small_gaps import bridge_small_gaps
        from encoder.ROI.brand_new import VALUE
        from encoder.enhancer.clahe import get_enhanced_image
        from decoder.uncompression.comparison import plot_comparison, calculate_quality_metrics
        import encoder.compression.clustering as c
        from encoder.compression.image import fill_black_holes_vectorized, quantize_image     # an unused variant / the hot path
        assert fill_black_holes_vectorized() == 'reference filler' and quantize_image.__module__.startswith('roibasedimagecompression_amd')
        import other.jpeg
        assert bridge_small_gaps() == 'reference small_gaps' and VALUE == 41 and get_enhanced_image() == 'reference clahe'
        assert plot_comparison() == 'reference plot' and calculate_quality_metrics.__module__.startswith('roibasedimagecompression_amd')
        assert c.__file__.startswith({ROOT!r}) and other.jpeg.Q == 3
        print('ok')
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env={**os.environ, "PYTHONDONTWRITEBYTECODE": "1"})
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_index_list_behaves_like_a_list():
    from roibasedimagecompression_amd.segment import IndexList
    a = IndexList(np.array([3, 1, 1, 2, 1], np.int32))
    assert len(a) == 5 and a.count(1) == 3 and a[0] == 3 and list(a) == [3, 1, 1, 2, 1]
    assert np.array(a).reshape(1, 5).tolist() == [[3, 1, 1, 2, 1]] and a == [3, 1, 1, 2, 1] and a.tolist() == [3, 1, 1, 2, 1]
    assert max(a) == 3 and a[1:3].tolist() == [1, 1]


def test_container_bytes_and_safe_loader(tmp_path):
    from encoder.compression.compression import lossless_compress_optimized, save_compressed, optimize_compressed_dtype
    from decoder.uncompression.uncompression import load_compressed, lossless_decompress
    g = np.load(os.path.join(G, "g7_container.npz"))
    pal = [[int(v) for v in r] for r in g["pal"]]
    idx = g["idx"].tolist()
    pkg = lossless_compress_optimized(pal, idx, tuple(int(v) for v in g["shape"]))
    assert pkg["p"] == g["p"].tobytes() and pkg["i"] == g["i"].tobytes() and pkg["d"] == str(g["d"]) and pkg["l"] == int(g["l"])
    fn = tmp_path / "x.rhccq"
    size = save_compressed(pkg, str(fn))
    raw = open(os.path.join(G, "g7_lenna64.rhccq"), "rb").read()
    assert fn.read_bytes() == raw and size == len(raw) - 1       # reference returns len + 8 for a 9-byte header
    back = load_compressed(os.path.join(G, "g7_lenna64.rhccq"))
    p2, i2, s2 = lossless_decompress(back)
    assert [list(c) for c in p2] == pal and i2 == idx and tuple(s2) == tuple(g["shape"])
    assert optimize_compressed_dtype({"indices": idx, "palette": pal})["indices_dtype"] == "uint8"
    with pytest.raises(TypeError):
        lossless_compress_optimized(pal, (1, 2, 3), (1, 3))
    import pickle, struct, zlib
    evil = zlib.compress(pickle.dumps(os.getcwd))
    bad = tmp_path / "evil.rhccq"
    bad.write_bytes(b"RHCCQ" + struct.pack("<I", len(evil)) + evil)
    with pytest.raises(Exception):
        load_compressed(str(bad))


def test_decoder_kat_files():
    import hashlib
    from decoder.uncompression.uncompression import load_compressed, lossless_decompress
    from test_oracle_golden import committed_artefacts
    arte = committed_artefacts()
    assert len(arte) == 35, len(arte)                 # every committed artefact of the reference
    for f, _, rec in arte:
        pal, idx, shape = lossless_decompress(load_compressed(os.path.join(G, f)))
        assert [int(v) for v in shape] == rec["shape"] and len(pal) == rec["l"], f
        assert hashlib.sha256(np.array(pal, np.uint8).tobytes()).hexdigest() == rec["palette_sha256"], f
        assert hashlib.sha256(np.array(idx, np.dtype(rec["d"])).tobytes()).hexdigest() == rec["indices_sha256"], f


def _mt_words_host(lib, count):
    w = np.empty(count, np.uint32)
    assert lib.rhccq_mt_words_host(0, count, w.ctypes.data) == 0
    return w


def _mt_randint(lib, pos, n, size):
    """RandomState.randint(0, n, size) at word `pos` from the library's own words: (values, words consumed)"""
    out = np.empty(size, np.int32)
    win = 2 * size + 1024
    while True:
        w = _mt_words_host(lib, pos + win)
        used = lib.rhccq_mt_randint_host(w.ctypes.data, len(w), pos, n, size, out.ctypes.data)
        if used >= 0:
            return out, used
        assert used == -1
        win *= 2


def test_mt_replay_equals_numpy_randomstate():
    """The library's replay (csrc/mt_replay.h: its own MT19937 words, rhccq_mt_randint_host, rhccq_mt_double_host) against
    RandomState(42).randint / random_sample / uniform: the draws of MiniBatchKMeans' init (validation indices, init sample, first
    centre, k-means++ uniforms) for several sizes, including power-of-two boundaries of the rejection mask and the one-value
    range that consumes nothing."""
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    for n, size, count in ((1500000, 90000, 1000), (10000, 3000, 50), (65536, 70000, 10), (65537, 100, 5), (3, 10, 4), (1, 5, 3),
                           (2 ** 31 - 5, 1000, 7), (30000, 30000, 12)):
        rs = np.random.RandomState(42)
        a, b = rs.randint(0, n, size), rs.randint(0, n, size)
        u0, u = rs.random_sample(), rs.uniform(size=count)
        pos = 0
        v1, used = _mt_randint(lib, pos, n, size)
        pos += used
        v2, used = _mt_randint(lib, pos, n, size)
        pos += used
        assert np.array_equal(a, v1) and np.array_equal(b, v2), n
        assert lib.rhccq_mt_double_host(pos) == u0
        assert np.array_equal([lib.rhccq_mt_double_host(pos + 2 + 2 * i) for i in range(count)], u)
    assert lib.rhccq_mt_double_host(-1) == -1.0
    assert lib.rhccq_mt_words_host(-1, 1, v1.ctypes.data) == -1 and lib.rhccq_mt_words_host(0, 1, None) == -1


def test_native_randint_replay_equals_numpy_randomstate():
    """rhccq_mt_randint_host (the host loop of the k-means++ set-up) against RandomState(42) itself, over the generator's raw words as
    numpy gives them: values, words consumed, the position-only form, a table that ends one word early."""
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    # (full-range uint32 draws are the raw 32-bit outputs, one word each)
    w = np.random.RandomState(42).randint(0, 1 << 32, size=1 << 19, dtype=np.uint32)
    assert np.array_equal(w, _mt_words_host(lib, len(w)))
    for n, size in ((1500000, 90000), (10000, 3000), (65536, 70000), (65537, 100), (3, 10), (1, 5), (2 ** 31 - 5, 1000), (30000, 30000)):
        rs = np.random.RandomState(42)
        a, b = rs.randint(0, n, size), rs.randint(0, n, size)
        o1, o2 = np.empty(size, np.int32), np.empty(size, np.int32)
        u1 = lib.rhccq_mt_randint_host(w.ctypes.data, len(w), 0, n, size, o1.ctypes.data)
        assert u1 >= 0 and lib.rhccq_mt_randint_host(w.ctypes.data, len(w), 0, n, size, None) == u1
        u2 = lib.rhccq_mt_randint_host(w.ctypes.data, len(w), u1, n, size, o2.ctypes.data)
        assert u2 >= 0 and np.array_equal(a, o1) and np.array_equal(b, o2), n
        p = u1 + u2                                        # the words consumed are numpy's own: its next double comes from there
        assert rs.random_sample() == (float(int(w[p]) >> 5) * 67108864.0 + float(int(w[p + 1]) >> 6)) / 9007199254740992.0
        if u1:
            assert lib.rhccq_mt_randint_host(w.ctypes.data, u1 - 1, 0, n, size, None) == -1
    assert lib.rhccq_mt_randint_host(None, 10, 0, 5, 5, None) == -2
    assert lib.rhccq_mt_randint_host(w.ctypes.data, len(w), 0, 0, 5, None) == -2


def test_native_palette_merge_equals_the_numpy_statement():
    """rhccq_merge_palettes_host (frame._merge) against the numpy statement of merge_region_components_simple in palette space
    it replaced: components painted in reversed order, entries by first position, first appearance numbers the colours, the
    smallest first position survives; black and unseen entries map to the canvas."""
    from roibasedimagecompression_amd import frame
    from roibasedimagecompression_amd.hostsort import _stable_order, _unique_first_inverse
    NONE = int(frame._FP_NONE)

    def numpy_merge(comps):
        seqs, sel = [], []
        for c in reversed(comps):
            valid = np.nonzero((c.keys != 0) & (c.fp < NONE))[0]
            v = valid[_stable_order(c.fp[valid])]
            sel.append(v)
            seqs.append(c.keys[v])
        allk = np.concatenate(seqs)
        u, first, inv = _unique_first_inverse(allk)
        order = np.argsort(first)
        gkeys = np.concatenate([np.zeros(1, np.uint32), u[order]])
        rank = np.empty(len(u), np.int64)
        rank[order] = np.arange(1, len(u) + 1)
        gidx = rank[inv.reshape(-1)]
        gfp = np.full(len(gkeys), NONE, np.int64)
        maps, off = {}, len(allk)
        for c, v in zip(comps, reversed(sel)):
            off -= len(v)
            lut = np.zeros(len(c.keys), np.int32)
            lut[v] = gidx[off:off + len(v)]
            np.minimum.at(gfp, lut[v], c.fp[v])
            for job, m in c.maps.items():
                maps[job] = lut[m]
        return gkeys, gfp, maps

    rng = np.random.default_rng(9)
    for trial in range(6):
        comps = []
        for j in range(int(rng.integers(2, 5))):
            K = int(rng.integers(1, 4000))
            keys = rng.integers(0, 3000 if trial % 2 else 1 << 24, K).astype(np.uint32)
            keys = np.unique(keys)                                   # a palette: distinct colours (possibly black)
            rng.shuffle(keys)
            fp = rng.permutation(1 << 22)[:len(keys)].astype(np.int64)
            fp[rng.random(len(keys)) < 0.1] = NONE                   # entries no pixel shows
            comps.append(frame._Comp(keys, fp, (0, 0), (1, 1), {j: rng.integers(0, len(keys), 500).astype(np.int32)}, False))
        got = frame._merge(comps, (0, 0, 10, 10))
        gk, gf, maps = numpy_merge(comps)
        assert np.array_equal(got.keys, gk) and np.array_equal(got.fp, gf)
        assert set(got.maps) == set(maps) and all(np.array_equal(got.maps[j], maps[j]) for j in maps)


def test_native_cluster_plan_equals_the_numpy_statement():
    """rhccq_cluster_plan_host (palette._cluster_resident) against the numpy passes it replaced: floor means of the non-empty
    clusters in label order behind the black rows, the uint16-valued label -> index table, -1 when a cluster needs the split."""
    from roibasedimagecompression_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(3)
    seen_split = seen_plan = 0
    for trial in range(40):
        k = int(rng.integers(1, 5000))
        nblack = int(rng.integers(0, 2))
        mc = int(rng.integers(5, 400))
        cnt = rng.integers(0, 60, k).astype(np.uint64) * (rng.random(k) < 0.8)
        sums = np.zeros((k, 4), np.uint64)
        sums[:, 3] = cnt
        for ch in range(3):
            sums[:, ch] = np.minimum(rng.integers(0, 256, k).astype(np.uint64) * cnt + rng.integers(0, 50, k).astype(np.uint64) % np.maximum(cnt, 1), 255 * cnt)
        s64, c = sums.astype(np.int64), sums[:, 3].astype(np.int64)
        nk, lut = np.empty(nblack + k, np.uint32), np.empty(k, np.int32)
        got = lib.rhccq_cluster_plan_host(sums.ctypes.data, k, mc, nblack, nk.ctypes.data, lut.ctypes.data)
        if (c > mc).any():
            assert got == -1
            seen_split += 1
            continue
        present = c > 0
        leaf = np.zeros(k, np.int64)
        leaf[present] = np.arange(int(present.sum()))
        cc = np.maximum(c[present], 1)
        means = ((s64[present, 0] // cc) << 16) | ((s64[present, 1] // cc) << 8) | (s64[present, 2] // cc)
        assert got == int(present.sum())
        assert np.array_equal(nk[:nblack + got], np.concatenate([np.zeros(nblack, np.uint32), means.astype(np.uint32)]))
        assert np.array_equal(lut, ((nblack + leaf) & 0xFFFF).astype(np.int32))
        seen_plan += 1
    assert seen_split and seen_plan
    assert lib.rhccq_cluster_plan_host(None, 3, 5, 0, nk.ctypes.data, lut.ctypes.data) == -2
    # more than 65 536 entries: the table wraps exactly like the reference's uint16 mapping_array (clustering.py:373) ...
    k = 70001
    sums = np.ones((k, 4), np.uint64)
    nk, lut = np.empty(1 + k, np.uint32), np.empty(k, np.int32)
    assert lib.rhccq_cluster_plan_host(sums.ctypes.data, k, 5, 1, nk.ctypes.data, lut.ctypes.data) == k
    want = np.zeros(1 + k, np.uint16)
    want[1:] = (1 + np.arange(k)).astype(np.uint16)                   # numpy's own uint16 store, as the reference does it
    assert np.array_equal(lut, want[1:].astype(np.int32)) and lut.max() == 65535 and lut[65535] == 0


def test_wrapped_mapping_is_flagged(caplog):
    """... and the Python side says so: info["mapping_wrapped"] + a warning on the `rhccq` logger"""
    import logging
    from roibasedimagecompression_amd.palette import _flag_wrap
    with caplog.at_level(logging.WARNING, logger="rhccq"):
        assert "mapping_wrapped" not in _flag_wrap({}, 65536)
        assert not caplog.records
        assert _flag_wrap({}, 65537)["mapping_wrapped"] is True
    assert any("65535" in r.getMessage() and "clustering.py:373" in r.getMessage() for r in caplog.records)


def test_native_scatter_min_equals_numpy():
    """rhccq_scatter_min_host (frame._scatter_min: first positions carried through a clustering) against np.minimum.at"""
    from roibasedimagecompression_amd import frame
    rng = np.random.default_rng(2)
    for _ in range(10):
        n, m = int(rng.integers(1, 3000)), int(rng.integers(0, 9000))
        idx, val = rng.integers(0, n, m), rng.integers(0, 1 << 22, m)
        want = np.full(n, int(frame._FP_NONE), np.int64)
        np.minimum.at(want, idx, val)
        assert np.array_equal(frame._scatter_min(n, idx, val), want)
    with pytest.raises(IndexError):
        frame._scatter_min(3, np.array([0, 3]), np.array([1, 2]))


def test_hostsort_helpers_equal_numpy():
    """hostsort._stable_order / _unique_first_inverse (one unstable sort of key<<32|position composites) against
    np.argsort(kind="stable") / np.unique(return_index, return_inverse), duplicates included"""
    from roibasedimagecompression_amd.hostsort import _stable_order, _unique_first_inverse
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 5, 1000, 70000):
        k = rng.integers(0, 1 << 24, n).astype(np.uint32)
        if n > 10:
            k[::7] = k[3]
        u, f, inv = np.unique(k, return_index=True, return_inverse=True)
        u2, f2, inv2 = _unique_first_inverse(k)
        assert np.array_equal(u, u2) and np.array_equal(f, f2) and np.array_equal(np.asarray(inv).reshape(-1), inv2), n
        lab = rng.integers(0, 50, n)
        assert np.array_equal(np.argsort(lab, kind="stable"), _stable_order(lab)), n
        fp = rng.permutation(max(n, 1) * 3)[:n].astype(np.int64) + (1 << 30)
        assert np.array_equal(np.argsort(fp, kind="stable"), _stable_order(fp)), n


def test_segment_that_fills_its_box_is_dropped_like_find_contours_does():
    """encoder/subregions/slic.py:188-193: skimage's find_contours(mask, 0.5) returns no contour for a CONSTANT mask, and the reference
    then appends nothing for that segment -- a segment filling its whole region box (>= 2 x 2) silently disappears; boxes thinner than
    two pixels take the reference's point-boundary branch and stay.  (Round 2 kept such segments: VERDICT r2 'missing' 3.)"""
    import numpy as np
    from encoder.subregions.slic import extract_slic_segment_boundaries
    full = np.ones((5, 6), bool)
    seg = np.ones((5, 6), np.int32)
    assert extract_slic_segment_boundaries(seg, full) == []
    seg[0, 0] = 2
    out = extract_slic_segment_boundaries(seg, full)
    assert [d["segment_id"] for d in out] == [1, 2] and [d["area"] for d in out] == [29, 1]
    assert [d["segment_id"] for d in extract_slic_segment_boundaries(np.ones((1, 6), np.int32), np.ones((1, 6), bool))] == [1]
    holed = full.copy()
    holed[2, 3] = False                                      # the segment covers its whole MASK but not the box: a contour exists
    assert [d["segment_id"] for d in extract_slic_segment_boundaries(np.ones((5, 6), np.int32), holed)] == [1]
