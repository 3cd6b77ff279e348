"""HIP kernels (through the C ABI) vs the CPU oracle, primitive by primitive.  GPU only."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def rh():
    import torch
    from roibasedimagecompression_amd.ops import Rhccq
    assert torch.cuda.is_available()
    return Rhccq(0)


@pytest.fixture(scope="module")
def O():
    from oracle import rhccq_oracle
    return rhccq_oracle


def load(name):
    return np.load(os.path.join(G, name), allow_pickle=False)


def test_unique_colors_golden_and_random(rh, O):
    import torch
    g = load("g1_unique.npz")
    imgs = [g[f"img{i}"] for i in range(int(g["n"]))]
    rng = np.random.default_rng(1)
    imgs.append(rng.integers(0, 256, (201, 303, 3), dtype=np.uint8))          # ragged, n_px % 4 != 0
    imgs.append(rng.integers(0, 3, (64, 64, 3), dtype=np.uint8))              # heavy duplicates incl. black
    imgs.append(np.full((5, 7, 3), 255, np.uint8))
    for im in imgs:
        keys, idx = rh.unique_colors(torch.from_numpy(im.copy()).to(rh.device))
        pal, oidx = O.unique_colors(im)
        assert np.array_equal(keys.cpu().numpy().astype(np.uint32), O.pack_rgb(pal))
        assert np.array_equal(idx.cpu().numpy(), oidx)


def test_eps_components_golden(rh):
    g = load("g3_dbscan.npz")
    eps = [float(e) for e in g["eps"]]
    from roibasedimagecompression_amd.ops import pack_rgb
    keys, es, want = [], [], []
    for name in g["names"]:
        P = g[f"pal_{name}"]
        for ei, e in enumerate(eps):
            keys.append(pack_rgb(P)); es.append(e); want.append(g[f"lab_{name}_{ei}"])
    labs, nc = rh.eps_components(keys, es)
    for i, (l, w) in enumerate(zip(labs, want)):
        assert np.array_equal(l, w), (i, es[i])
        assert nc[i] == w.max() + 1


def test_eps_components_random_vs_oracle(rh, O):
    from eps_cases import reference_labels
    rng = np.random.default_rng(7)
    keys, es = [], []
    for n, hi in ((1, 256), (2, 256), (700, 256), (5000, 256), (10240, 256), (9000, 40), (3000, 12)):
        P = np.unique(rng.integers(0, hi, (n, 3)).astype(np.uint8), axis=0)
        P = P[rng.permutation(len(P))]                      # merged palettes are NOT sorted
        for e in (1.0, 2.0, 5.0, 12.8, 25.6, 27.0, 32.0, 51.2, 102.4):
            keys.append(O.pack_rgb(P)); es.append(e)
    labs, _ = rh.eps_components(keys, es)
    for k, e, l in zip(keys, es, labs):
        if len(k) > 6000 and e < 25:                         # oracle too slow there: the exact reference of tests/eps_cases.py
            assert np.array_equal(l, reference_labels(O.unpack_rgb(k), e)), (len(k), e)
            continue
        assert np.array_equal(l, O.eps_components(O.unpack_rgb(k), e)), (len(k), e)


def test_eps_components_oversize_global_path(rh, O):
    rng = np.random.default_rng(3)
    P = np.unique(rng.integers(0, 256, (12000, 3)).astype(np.uint8), axis=0)
    labs, nc = rh.eps_components([O.pack_rgb(P)], [6.0])
    assert np.array_equal(labs[0], O.eps_components(P, 6.0))


def test_kmeans_split_vs_oracle(rh, O):
    g = load("g3_dbscan.npz")
    cases = []
    for name, ks in (("lenna64", (2, 12, 25, 67)), ("rand500", (2, 3, 25, 150, 500)), ("lenna_final", (5, 67, 146)),
                     ("dark", (5, 25, 150)), ("lattice", (5, 67)), ("rand3000", (12, 150)), ("gapped", (2, 41))):
        P = g[f"pal_{name}"]
        for k in ks:
            cases.append((P, k))
    labs, info = rh.kmeans_split([O.pack_rgb(P) for P, _ in cases], [k for _, k in cases], return_info=True)
    for (P, k), l, inf in zip(cases, labs, info):
        ol, oi = O.kmeans_labels(P, k, return_info=True)
        assert np.array_equal(l, ol), (len(P), k, inf, oi["n_iter"], (l == ol).mean())
        assert inf[0] == oi["n_iter"] and bool(inf[1]) == oi["strict"] and inf[2] == oi["relocated"]


def test_kmeans_split_large_k_and_global_path(rh, O):
    rng = np.random.default_rng(11)
    P = np.unique(rng.integers(0, 256, (2600, 3)).astype(np.uint8), axis=0)       # k > 1024: centres in global memory
    P2 = np.unique(rng.integers(0, 64, (11000, 3)).astype(np.uint8), axis=0)      # n > LDS max: points in global memory
    labs = rh.kmeans_split([O.pack_rgb(P), O.pack_rgb(P2)], [1300, 7])
    assert np.array_equal(labs[0], O.kmeans_labels(P, 1300))
    assert np.array_equal(labs[1], O.kmeans_labels(P2, 7))


def test_cluster_means(rh, O):
    import torch
    rng = np.random.default_rng(5)
    P = rng.integers(0, 256, (5000, 3)).astype(np.uint8)
    lab = rng.integers(-1, 37, 5000).astype(np.int32)
    keys = torch.from_numpy(O.pack_rgb(P).astype(np.int32)).to(rh.device)
    means, sums = rh.cluster_means(keys, torch.from_numpy(lab).to(rh.device), 37)
    want = np.stack([P[lab == j].astype(np.int64).sum(0) // max((lab == j).sum(), 1) for j in range(37)])
    assert np.array_equal(O.unpack_rgb(means.cpu().numpy()), want.astype(np.uint8))


@pytest.mark.parametrize("estep", ["tiles", "tiles/2", "tiles/4", "tiles/8", "grid", "tiles/weights_in_global_memory"])
def test_minibatch_vs_oracle_bit_exact(rh, O, estep):
    """Both batch E-step variants (tiled brute force for few problems; per-step re-binned centre grid when a batch
    of frames puts many problems in flight) against the oracle: step count, centres and labels bit-exact."""
    g = load("g10_minibatch.npz")
    pal, _ = O.unique_colors(g["img"])
    pal = pal[~np.all(pal == 0, axis=1)]
    rng = np.random.default_rng(2)
    P2 = np.unique(rng.integers(0, 256, (30000, 3)).astype(np.uint8), axis=0)
    P3 = np.unique(rng.integers(0, 48, (14000, 3)).astype(np.uint8), axis=0)
    # k = 40: ~25 batch rows per centre -> the update walks the batch instead of the per-centre member lists
    cases = [(pal, int(np.ceil(len(pal) * 0.2 / 10))), (pal, int(np.ceil(len(pal) * 0.1 / 10))), (P2, 450), (P3, 40)]
    # (the reassignment sweeps of k > 30 720 read the weights from global memory: here forced for small k, which the oracle can check)
    glob = estep.endswith("weights_in_global_memory")
    if glob:
        rh.set_option(rh.OPT_REASSIGN_LDS, 0)
    try:
        labs, info = rh.minibatch_kmeans([O.pack_rgb(P) for P, _ in cases], [k for _, k in cases], return_info=True, estep=estep.split("/")[0],
                                          estep_split=int(estep.split("/")[1]) if "/" in estep and not glob else 1)
    finally:
        rh.set_option(rh.OPT_REASSIGN_LDS, 1)
    for i, ((P, k), l) in enumerate(zip(cases, labs)):
        ol, oi = O.minibatch_kmeans_labels(P, k, return_info=True)
        st = info["state"][i]
        assert int(st[5]) == oi["n_steps"], (st, oi["n_steps"])
        c = info["centres"][info["koff"][i]:info["koff"][i + 1], :3]
        assert np.array_equal(c, oi["centers"]), np.abs(c - oi["centers"]).max()
        assert np.array_equal(l, ol), (l == ol).mean()


def test_npysort_head_equals_numpy_scalar_argsort(rh, O):
    """csrc/k8_npysort.h (the parallel emulation of numpy's scalar aquicksort_<double>, restricted to the partitions that straddle
    slot `cap`) against np.argsort ITSELF under the scalar setting (g15_npysort.npz, generated by numpy) and, for other caps,
    depth limits and sizes beyond 30 720, against the CPU restatement of the same sort (oracle/npy_argsort.c, itself pinned by
    g15): the SET of the first `cap` entries must be identical."""
    g = load("g15_npysort.npz")
    n_checked = 0
    for i in range(int(g["n"])):
        w = g[f"w{i}"].astype(np.float64)
        k = len(w)
        if k < 3 or w.min() < 0 or not np.array_equal(w, np.floor(w)):
            continue                                            # (the kernel takes the path's weights: integer counts)
        order = g[f"o{i}"].astype(np.int64)
        for cap in sorted({1, 2, k // 3, min(500, k - 1), k - 1} - {0}):
            want = np.zeros(k, bool)
            want[order[:cap]] = True
            assert np.array_equal(rh.npysort_head(w, cap), want), (i, k, cap)
            if k > 64:
                assert np.array_equal(rh.npysort_head(w, cap, use_lds=False), want), (i, k, cap, "global memory throughout")
            n_checked += 1
    assert n_checked >= 300, n_checked
    rng = np.random.default_rng(15)
    for k, draws, depth0 in ((100, 30, 0), (5000, 700, 1), (30128, 1000, 2), (30128, 29000, 3), (70001, 2000, -1), (70001, 150000, 4),
                             (200003, 1000, -1), (20771, 3000, 0), (4097, 4097, 2)):
        w = np.zeros(k)
        np.add.at(w, rng.integers(0, k, draws), 1.0)
        order = O.npy_argsort_scalar(w, depth0)
        for cap in (500 if k > 501 else 17, k // 2):
            want = np.zeros(k, bool)
            want[order[:cap]] = True
            assert np.array_equal(rh.npysort_head(w, cap, depth0), want), (k, draws, depth0, cap)
            assert np.array_equal(rh.npysort_head(w, cap, depth0, use_lds=False), want), (k, draws, depth0, cap, "global memory throughout")


@pytest.mark.parametrize("order", ["npysort", "stable"])
def test_minibatch_equals_sklearn_golden(rh, O, order):
    """HIP MiniBatchKMeans against scikit-learn ITSELF on 8 inputs up to 790 421 colours / k = 15 809 -- whole Lenna and whole
    Kodak frames as one segment, the bench generator's 1 Mpx photo: k-means++ picks, step count, centres bit for bit and labels
    (hash).  No oracle in between.
      npysort (the default, RHCCQ_OPT_REASSIGN_ORDER = 1): scikit-learn's UNTOUCHED fit_predict under numpy's scalar sort kernels
        (g11_scalar.*, make_golden_npysort.py) -- the reference's own result on such a host, at every k;
      stable (rounds 1-3): the fit with the one np.argsort of _mini_batch_step forced stable (g11_mbk_sklearn.*).
    For the cases with k < 500 (no capped reassignment) both are the reference's untouched result on every host."""
    from test_oracle_golden import check_against_g11, g11_cases, g11_palette, g11_scalar
    cases = g11_cases()
    g = load("g11_mbk_sklearn.npz")
    scases, sg = g11_scalar()
    names = list(cases)
    pals = [g11_palette(n, cases[n]) for n in names]
    rh.set_option(rh.OPT_REASSIGN_ORDER, 1 if order == "npysort" else 0)
    try:
        labs, info = rh.minibatch_kmeans([O.pack_rgb(P) for P in pals], [cases[n]["k"] for n in names], return_info=True)
    finally:
        rh.set_option(rh.OPT_REASSIGN_ORDER, 1)
    untouched = load("g11_untouched.npz")          # sklearn's untouched fit where it is identical under every host setting (make_stability.py)
    assert len(untouched.files) >= 3
    for i, n in enumerate(names):
        a, b = info["koff"][i], info["koff"][i + 1]
        if order == "npysort":
            check_against_g11(n, scases[n], sg, info["chosen"][a:b], info["state"][i][5], info["centres"][a:b, :3], labs[i], record="scalar")
        else:
            check_against_g11(n, cases[n], g, info["chosen"][a:b], info["state"][i][5], info["centres"][a:b, :3], labs[i])
        if n in untouched.files:
            assert np.array_equal(labs[i], untouched[n]), (n, "HIP labels vs the untouched scikit-learn fit")


def test_minibatch_overlapped_steps_equal_the_classic_sequence(rh, O):
    """A lone problem whose centres all carry weight runs rhccq_mbk_steps_overlapped (k8_overlap.h): the E-step of step t + 1 beside
    the update of step t -- untouched centres speculatively, touched ones at their new values afterwards.  State (steps, EWA
    values, MT cursor), centres, weights and labels must equal the classic three-launch sequence bit for bit; the cases put
    reassignment steps (every 10 k / 1000 steps) inside the overlapped range, k below and above one speculative tile, a
    ragged last tile, and n < 1000 rows per batch is covered by the classic path only (k >= 1024 is required)."""
    cls = type(rh)
    rng = np.random.default_rng(77)
    g = load("g10_minibatch.npz")
    pal, _ = O.unique_colors(g["img"])
    pal = pal[~np.all(pal == 0, axis=1)]
    cases = [(np.unique(rng.integers(0, 256, (90000, 3)).astype(np.uint8), axis=0), 1100),
             (np.unique(rng.integers(0, 256, (260000, 3)).astype(np.uint8), axis=0), 4321),
             (np.unique((rng.normal(128, 40, (500000, 3))).clip(0, 255).astype(np.uint8), axis=0), 16400),
             (pal, max(1024, len(pal) // 40))]
    total = 0
    for P, k in cases:
        keys = O.pack_rgb(P)
        out = {}
        for overlap in (False, True):
            cls.MBK_OVERLAP = overlap
            try:
                out[overlap] = rh.minibatch_kmeans([keys], [k], return_info=True)
            finally:
                cls.MBK_OVERLAP = True
        (l0, i0), (l1, i1) = out[False], out[True]
        assert i0["overlapped_launches"] == 0
        total += i1["overlapped_launches"]
        s0, s1 = i0["state"][0], i1["state"][0]
        par = int(s0[5]) & 1
        live = [0, 1, 2, 4, 5, 6, 7, 11] + ([12, 13] if par else [3, 8])     # (the cursor may sit one batch ahead)
        assert np.array_equal(s0[live], s1[live]), (k, s0, s1)
        assert np.array_equal(i0["centres"], i1["centres"]), (k, int(s0[5]))
        assert np.array_equal(i0["weights"], i1["weights"]), k
        assert np.array_equal(l0[0], l1[0]), k
    assert total >= 300, total                                # the overlapped sequence did run


@pytest.mark.parametrize("order", ["npysort", "stable"])
def test_minibatch_overlapped_equals_sklearn_golden(rh, O, order):
    """The overlapped sequence against scikit-learn itself: the g11 fixtures with every problem on a lane of its own (a lone
    problem is what rhccq_mbk_steps_overlapped takes), under both tie orders of the reassignment (see above)."""
    from test_oracle_golden import check_against_g11, g11_cases, g11_palette, g11_scalar
    cases = g11_cases()
    g = load("g11_mbk_sklearn.npz")
    scases, sg = g11_scalar()
    names = list(cases)
    pals = [g11_palette(n, cases[n]) for n in names]
    rh.set_option(rh.OPT_REASSIGN_ORDER, 1 if order == "npysort" else 0)
    try:
        labs, info = rh.minibatch_kmeans([O.pack_rgb(P) for P in pals], [cases[n]["k"] for n in names], return_info=True, lanes=len(names))
    finally:
        rh.set_option(rh.OPT_REASSIGN_ORDER, 1)
    assert info["overlapped_launches"] > 0
    for i, n in enumerate(names):
        a, b = info["koff"][i], info["koff"][i + 1]
        if order == "npysort":
            check_against_g11(n, scases[n], sg, info["chosen"][a:b], info["state"][i][5], info["centres"][a:b, :3], labs[i], record="scalar")
        else:
            check_against_g11(n, cases[n], g, info["chosen"][a:b], info["state"][i][5], info["centres"][a:b, :3], labs[i])


def test_minibatch_more_than_256_problems(rh, O):
    """the Morton sort names the problem in 8 bits of its key -- rhccq_mbk_order chunks by 256 problems.
    300 small problems in one call (a batch of 65+ 4K frames has that many segments), spot-checked against the oracle."""
    rng = np.random.default_rng(77)
    pals = [np.unique(rng.integers(0, 40 + (i % 7) * 30, (1500, 3)).astype(np.uint8), axis=0) for i in range(300)]
    ks = [3 + (i % 5) for i in range(300)]
    labs, info = rh.minibatch_kmeans([O.pack_rgb(P) for P in pals], ks, return_info=True)
    for i in (0, 1, 255, 256, 257, 299):
        ol, oi = O.minibatch_kmeans_labels(pals[i], ks[i], return_info=True)
        assert int(info["state"][i][5]) == oi["n_steps"], i
        assert np.array_equal(info["centres"][info["koff"][i]:info["koff"][i + 1], :3], oi["centers"]), i
        assert np.array_equal(labs[i], ol), i


def test_merge_kernels_and_remap_decode(rh, O):
    import torch
    g = load("g5_merge.npz")
    from roibasedimagecompression_amd.palette import merge_components
    for name in g["names"]:
        comps = []
        for ci in range(int(g[f"{name}_n"])):
            m = g[f"{name}_c{ci}_meta"]
            comps.append({"top_left": (int(m[0]), int(m[1])), "shape": (int(m[2]), int(m[3])),
                          "palette": g[f"{name}_c{ci}_pal"], "indices": g[f"{name}_c{ci}_idx"]})
        out = merge_components(rh, comps, tuple(int(v) for v in g[f"{name}_bbox"]))
        assert np.array_equal(np.asarray(out["palette"]).reshape(-1, 3), g[f"{name}_out_pal"]), name
        assert np.array_equal(np.asarray(out["indices"]).reshape(-1), g[f"{name}_out_idx"]), name
    rng = np.random.default_rng(9)
    idx = rng.integers(0, 500, 100003).astype(np.int32)
    lut = rng.integers(0, 9999, 500).astype(np.int32)
    got = rh.remap(torch.from_numpy(idx).to(rh.device), torch.from_numpy(lut).to(rh.device)).cpu().numpy()
    assert np.array_equal(got, lut[idx])
    pal = rng.integers(0, 256, (500, 3)).astype(np.uint8)
    for dt in (np.uint8, np.int16, np.int32):
        ii = (idx % (200 if dt == np.uint8 else 500)).astype(dt)
        rec = rh.decode(torch.from_numpy(ii).to(rh.device), torch.from_numpy(pal).to(rh.device)).cpu().numpy()
        assert np.array_equal(rec, pal[ii.astype(np.int64)])


@pytest.mark.parametrize("block", [8, 16])
def test_dct_quant_extension(rh, O, block):
    """EXTENSION (no reference counterpart): vs scipy.fft.dctn(type=2, norm='ortho').  Tolerance:
    coefficients within 1e-5 relative to the block DC scale (255*block); quantised integers exact."""
    import torch
    rng = np.random.default_rng(4)
    rgb = rng.integers(0, 256, (112, 176, 3), dtype=np.uint8)     # not a multiple of the 32x32 staging tile
    roi = np.zeros((112, 176), np.uint8)
    roi[20:50, 30:100] = 1
    luma, qstep = rh.luma_qstep(torch.from_numpy(rgb).to(rh.device), torch.from_numpy(roi).to(rh.device), block, 4.0, 16.0)
    r, gch, b = (rgb[..., i].astype(np.float32) for i in range(3))
    want_luma = (np.float32(0.299) * r + np.float32(0.587) * gch) + np.float32(0.114) * b
    assert np.array_equal(luma.cpu().numpy(), want_luma)
    tiles = roi.reshape(112 // block, block, 176 // block, block).max(axis=(1, 3))
    want_q = np.where(tiles > 0, 4.0, 16.0).astype(np.float32)
    assert np.array_equal(qstep.cpu().numpy(), want_q)
    coef, q = rh.dct_quant(luma, block, qstep)
    oc, oq = O.dct_quant_blocks(want_luma, block, want_q.astype(np.float64))
    assert np.abs(coef.cpu().numpy() - oc).max() <= 1e-5 * 255 * block
    assert np.array_equal(q.cpu().numpy(), oq)


@pytest.mark.parametrize("path", ["default", "register_chain", "third_generation", "tiny_work_list", "small_work_list", "one_candidate_per_wave", "two_candidates_per_wave", "three_candidates_per_wave",
                                  "three_candidates_per_wave_small_work_list", "second_generation", "second_generation_tiny_work_list",
                                  "first_generation", "first_generation_tiny_work_list", "global_tables", "in_wave", "in_wave_small_work_list"])
def test_minibatch_init_chain_many_cases(rh, O, path):
    """The k-means++ chains (mbk_init3_kernel: leaves of 16 samples under three box levels, 64-ary candidate search, quad
    evaluation with the samples kept in registers for the commit, brute force when the work list overflows -- the default up
    to 98 304 init samples; mbk_init2_kernel: the second generation, blocks of 64, up to 262 144; mbk_init_kernel: the first
    generation beyond) against the oracle's exact-integer k-means++ on the same init sample in sklearn's draw order, for
    several shapes -- every pick must be identical (this is the kernel where a reduction race once hid behind lucky timing).
    `tiny_work_list` / `small_work_list` / `global_tables` lower the thresholds (rhccq_ctx_set_int) so that the paths of the
    first picks and of very large problems -- brute force / per-candidate evaluation when the shared work list overflows, the
    re-read commit when it exceeds the registers, block tables in global memory -- run on inputs the oracle can check."""
    if path == "global_tables":
        rh.set_option(rh.OPT_INIT_LDS_BLOCKS, 8)
    if path.endswith("tiny_work_list"):
        rh.set_option(rh.OPT_INIT_MAX_ITEMS, 24)
    if path.endswith("small_work_list"):
        rh.set_option(rh.OPT_INIT_MAX_ITEMS, 200)
    cw = {"one": 1, "two": 2, "three": 3}.get(path.split("_")[0])
    if cw:
        rh.set_option(rh.OPT_INIT_CANDS_PER_WAVE, cw)
    if path.startswith("first_generation"):
        rh.set_option(rh.OPT_INIT_KERNEL, 1)
    if path.startswith("second_generation"):
        rh.set_option(rh.OPT_INIT_KERNEL, 2)
    if path == "third_generation":                         # (option 3: the same choice as the default)
        rh.set_option(rh.OPT_INIT_KERNEL, 3)
    if path.startswith("in_wave"):                         # round 4: every candidate evaluated by the wave that found it (opt-in: measured slower)
        rh.set_option(rh.OPT_INIT_KERNEL, 5)
    if path == "register_chain":                           # kpp_flat.h (the chain KMeans uses): opt-in for the MiniBatch init
        rh.set_option(rh.OPT_INIT_KERNEL, 4)
    try:
        _init_chain_cases(rh, O, small_only=path == "register_chain")
    finally:
        rh.set_option(rh.OPT_INIT_LDS_BLOCKS, 4096)
        rh.set_option(rh.OPT_INIT_MAX_ITEMS, 12288)
        rh.set_option(rh.OPT_INIT_KERNEL, 0)
        rh.set_option(rh.OPT_INIT_CANDS_PER_WAVE, DEFAULT_CANDS_PER_WAVE)


DEFAULT_CANDS_PER_WAVE = 1


@pytest.mark.parametrize("shards", [2, 8])
def test_minibatch_init_chain_sharded(rh, O, shards):
    """The sharded k-means++ chain (mbk_init2_kernel<true>): C workgroups per problem, each with its own draw range and Morton
    index, candidate colours and partial improvements exchanged through tagged 8-byte granules.  Exact integers everywhere, so
    every pick must equal the one-workgroup chain's = sklearn's.  Opt-in (measured slower than one workgroup); one launch
    with two problems (the second one too small for 8 shards: the launcher falls back to 2 for both) and the pipelined
    per-problem launches."""
    rng = np.random.default_rng(321)
    cases = []
    for n, hi, k in ((140000, 256, 11000), (90000, 200, 3000)):
        P = np.unique(rng.integers(0, hi, (n, 3)).astype(np.uint8), axis=0)
        cases.append((P, k))
    rh.set_option(rh.OPT_INIT_SHARDS, shards)
    try:
        for lanes in (1, None):
            labs, info = rh.minibatch_kmeans([O.pack_rgb(P) for P, _ in cases], [k for _, k in cases], return_info=True, lanes=lanes)
            for i, (P, k) in enumerate(cases):
                want, _ = O.kmeanspp_picks_native(P, k)
                got = info["chosen"][info["koff"][i]:info["koff"][i + 1]]
                assert np.array_equal(got, want), (shards, lanes, i, int(np.argmax(got != want)))
                cen = info["init_centres"][info["koff"][i]:info["koff"][i + 1]] if "init_centres" in info else None
                assert cen is None or np.array_equal(cen[:, :3], P[info["init_idx"][i]][want].astype(np.float64))
    finally:
        rh.set_option(rh.OPT_INIT_SHARDS, 1)


def _init_chain_cases(rh, O, small_only=False):
    import math
    rng = np.random.default_rng(123)
    cases = []
    for n, hi, k in ((12000, 256, 130), (30000, 256, 900), (45000, 96, 2500), (20000, 40, 400), (70000, 256, 4200), (400000, 256, 9000),
                     (26000, 256, 2730), (16000, 30, 1001)):
        P = np.unique(rng.integers(0, hi, (n, 3)).astype(np.uint8), axis=0)
        if len(P) >= 10000 and (not small_only or max(3000, 3 * k) <= 8192):
            cases.append((P, k))
    # (small_only: one problem per call, so that every call is one the register chain takes -- 3 000 to 8 190 init samples)
    labs, info = rh.minibatch_kmeans([O.pack_rgb(P) for P, _ in cases], [k for _, k in cases], return_info=True,
                                      lanes=len(cases) if small_only else None)
    for i, (P, k) in enumerate(cases):
        n = len(P)
        if i == 0:                                         # the numpy statement once, the native one (same picks, G11) for the rest
            rs = np.random.RandomState(42)
            init_size = 3000 if 3000 >= k else 3 * k      # sklearn: 3 * batch_size, or 3 * k when that is < k
            init_size = min(init_size, n)
            rs.randint(0, n, init_size)
            ii = rs.randint(0, n, init_size) if init_size < n else np.arange(n)     # sklearn's draw order
            want = O.kmeanspp_int(P[ii].astype(np.int64), k, rs)
        else:
            want, _ = O.kmeanspp_picks_native(P, k)
        got = info["chosen"][info["koff"][i]:info["koff"][i + 1]]
        assert np.array_equal(got, want), (i, n, k, int(np.argmax(got != want)))


@pytest.mark.parametrize("case", [(2, 6.0, 1.0, 5), (1, 3.0, 0.0, 3), (3, 10.0, 2.0, 12), (4, 25.0, 0.5, 1), (0, 1.0, 1.0, 1)])
def test_pixel_space_dbscan_extension(rh, O, case):
    """EXTENSION (no reference counterpart, named by BASELINE.json's north_star): fixed-radius neighbour pass over
    (x, y, L, a, b) + union-find cluster expansion vs the brute-force restatement -- neighbour counts, core flags and
    labels bit-identical (float32 operations in a fixed order on both sides)."""
    import torch
    from roibasedimagecompression_amd import synth
    radius, eps, ws, min_pts = case
    lut = rh.px_tables()
    for H, W, seed, kind in ((37, 53, 1, "photo"), (64, 130, 2, "poster"), (16, 64, 3, "photo"), (5, 3, 4, "photo")):
        img = synth.photo(H, W, seed, sigma=3.0) if kind == "photo" else synth.poster(H, W, seed)
        labels, core, count = rh.px_dbscan(torch.from_numpy(img).to(rh.device), radius, eps, ws, min_pts, want_count=True)
        ol, oc, on = O.px_dbscan(img, radius, eps, ws, min_pts, lut)
        assert np.array_equal(count.cpu().numpy(), on), (case, H, W)
        assert np.array_equal(core.cpu().numpy(), oc), (case, H, W)
        assert np.array_equal(labels.cpu().numpy(), ol), (case, H, W)
