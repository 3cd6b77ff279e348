"""CPU oracle for the RHCCQ encoder hot path  --  TEST INFRASTRUCTURE ONLY.

This module is a numpy restatement of the reference's palette-hierarchy encoder
(Riccardoalfieri2003/ROIBasedImageCompression, snapshot 2026-01-16).  It exists so
that the HIP path can be checked against it; it is *never* imported by the product
package.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
import it.

Parity pins (see DESIGN.md "Oracle"):
  * every function below is checked against golden vectors that were produced by
    importing and running the reference itself in the build container
    (tests/golden/make_golden.py; versions in tests/golden/versions.json);
  * integer / index work (unique colours, parameters, eps-components, floor-means,
    merge, remap, dtype choice, container bytes) is bit-exact against those vectors
    (Tier A);
  * the two k-means branches reach into scikit-learn 1.7.2 (unpinned by the reference, requirements.txt:6).  KMeans
    (oversize-cluster split): restated with the "KM64" arithmetic below; against scikit-learn itself it reproduces the
    same partition on most golden cases (Tier A when it does, Tier B = same palette size / equivalent PSNR otherwise).
    MiniBatchKMeans (every segment of >= 10 000 colours): restated operation for operation -- RandomState(42) consumed as
    sklearn consumes it, k-means++ in draw order, batch-ordered centre updates, sequential inertia, and its ONE
    host-dependent step (an unstable np.argsort over tied counts in _mini_batch_step) as numpy's scalar sort kernel runs
    it (npy_argsort.c) -- and pinned bit for bit against scikit-learn's UNTOUCHED fit_predict under that stated host
    setting (tests/golden/make_golden_npysort.py, G11-scalar / G15); the stable tie order of rounds 1-3 stays selectable
    and pinned to sklearn with that call forced stable (make_golden_mbk.py, G11); wherever the step does not trigger
    (k < 500) every host gives the same fit and it is reproduced.

  * PARITY UNPINNED (say so wherever these are cited): the stages UPSTREAM of the hot path lean on libraries that are absent
    from the build container -- scikit-image (split score, masked SLIC, SSIM: sk_* / slic_* / structural_similarity_win7) and
    OpenCV (the whole ROI stage: cv_* , get_edge_map, the clean-up chain, connected components and their numbering).  They
    are restated from the libraries' published algorithms; what pins them is (a) scipy, wherever the reference itself or
    scikit-image calls it (extract_roi_nonroi's dilations, resize's gaussian_filter / zoom), (b) known answers that need no
    library (tests/test_roi_cpu.py), and (c) Tier B end to end (all 25 + 8 artefact pairs, tests/test_gpu_notebook.py; the r02 figure follows): the whole script flow lands within 0.15 dB / 3.2 % of four
    artefacts the reference ships and within 0.6 dB / 6.3 % of two more (tests/test_gpu_notebook.py).

Canonical k-means arithmetic "KM64" (shared with csrc/):
  * points are integer colours p in [0,255]^3;
  * k-means++ works on EXACT integer squared distances between data points
    (sklearn: the same quantities in float64, |err| ~ 1e-11), so cumulative sums,
    potentials and argmins are order-independent;
  * random draws follow numpy's legacy MT19937 RandomState(42) stream exactly as
    sklearn consumes it (choice(p=uniform) for the first centre, uniform(size=T)
    per further centre, T = 2 + int(ln k));
  * Lloyd (KMeans): x = p - m with m = sum(p)/n (exact integer sum, one IEEE
    division); dist(i,j) = csq_j + (-2 * fma(x2, c2, fma(x1, c1, x0*c0))) with
    csq_j = (c0*c0 + c2*c2) + c1*c1 -- bit for bit what sklearn's E-step evaluates
    (OpenBLAS dgemm FMA chain over k, numpy-einsum two-lane row norms): on integer
    colour lattices exact real-arithmetic ties are common and these roundings decide
    them (oracle/km64_estep.c); every other operation is individually rounded;
    label = first arg-min; new centre = (exact integer sum of member p)/count - m;
    convergence exactly as sklearn._kmeans_single_lloyd (labels unchanged, or
    sum_j |dc_j|^2 <= tol with tol = 1e-4 * mean(var)), max_iter = 300.
  * MiniBatch: see minibatch_kmeans_labels() (numpy) and oracle/mbk_oracle.c (the same in C, for sizes numpy cannot reach).

Each function cites the reference lines it restates (paths relative to the reference
root).
"""
from __future__ import annotations

import io
import math
import pickle
import struct
import zlib

import numpy as np

__all__ = [
    "pack_rgb", "unpack_rgb", "unique_colors", "clustering_params", "eps_threshold",
    "eps_components", "kmeanspp_int", "kmeans_labels", "split_large_cluster",
    "minibatch_kmeans_labels", "minibatch_kmeans_native", "npy_argsort_scalar", "kmeanspp_picks_native", "cluster_palette", "merge_components", "segment_crop",
    "level1_region", "region_quantization", "quantize_image", "optimal_index_dtype",
    "encode_frame", "region_segment_count", "find_contours_drops", "kept_segments", "script_flow", "pack_container", "container_bytes", "load_container", "decode_container",
    "dct_quant_blocks", "adaptive_quality_metrics", "split_score", "normalize_result", "enhanced_slic", "slic_masked", "slic_sweeps", "slic_enforce_connectivity",
    "slic_mask_centroids", "sk_resize", "sk_rgb2lab", "sk_rgb2gray", "sk_sobel", "sk_lbp_uniform_8_1",
]

MINIBATCH_THRESHOLD = 10000  # clustering.py:205

_KM64 = None


def _km64_lib():
    """oracle/km64_estep.c + oracle/mbk_oracle.c built in place with gcc (the E-step needs a correctly rounded fma,
    which numpy does not expose; the native MiniBatchKMeans restatement serves the cases numpy is too slow for)."""
    global _KM64
    if _KM64 is not None:
        return _KM64
    import ctypes
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    srcs = [os.path.join(here, "km64_estep.c"), os.path.join(here, "mbk_oracle.c"), os.path.join(here, "npy_argsort.c")]
    out = os.path.join(here, "_build", "libkm64.so")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in srcs):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["gcc", "-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC", "-o", out] + srcs + ["-lm"])
    lib = ctypes.CDLL(out)
    lib.km64_estep.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    lib.km64_estep.restype = None
    lib.mbk_fit.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_int32,
                            ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mbk_fit.restype = ctypes.c_int
    lib.npy_argsort_f64.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.npy_argsort_f64.restype = None
    lib.npy_argsort_f64_depth.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int]
    lib.npy_argsort_f64_depth.restype = None
    lib.mbk_init_picks.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p,
                                   ctypes.c_void_p]
    lib.mbk_init_picks.restype = ctypes.c_int
    _KM64 = lib
    return lib


def _mbk_init_size(n, k, batch_size=1000):
    bs = min(batch_size, n)
    init_size = 3 * bs
    if init_size < k:
        init_size = 3 * k
    return min(init_size, n)


ARGSORT_KINDS = {"stable": 0, "npysort": 1}
DEFAULT_ARGSORT = "npysort"      # numpy's scalar aquicksort: the host setting of record (npy_argsort.c)


def npy_argsort_scalar(w, depth0=-1):
    """np.argsort(w) as numpy's scalar (non-SIMD) aquicksort_<double> orders it (oracle/npy_argsort.c); depth0 >= 0 lowers
    the introsort depth limit (numpy's: 2 floor(log2 n)) so that ordinary inputs reach the heapsort branch"""
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = np.empty(len(w), np.int64)
    _km64_lib().npy_argsort_f64_depth(w.ctypes.data, len(w), out.ctypes.data, int(depth0))
    return out


def minibatch_kmeans_native(points, k, seed=42, max_steps=None, threads=0, want_labels=True, argsort=None):
    """oracle/mbk_oracle.c: the same restatement as minibatch_kmeans_labels() in C (OpenMP over `threads` host cores,
    0 = all).  Returns (labels int32[n] or None, info) with info keys n_steps, centers, picks, init_indices, mt_words."""
    P = np.ascontiguousarray(np.asarray(points).reshape(-1, 3).astype(np.uint8))
    n = len(P)
    isz = _mbk_init_size(n, k)
    C = np.empty((k, 3), np.float64)
    lab = np.empty(n, np.int32) if want_labels else None
    picks = np.empty(k, np.int32)
    init_idx = np.empty(isz, np.int64)
    info = np.zeros(8, np.int64)
    rc = _km64_lib().mbk_fit(P.ctypes.data, n, int(k), int(seed), -1 if max_steps is None else int(max_steps), int(threads),
                             ARGSORT_KINDS[argsort or DEFAULT_ARGSORT], C.ctypes.data, lab.ctypes.data if want_labels else None, picks.ctypes.data, init_idx.ctypes.data,
                             info.ctypes.data)
    if rc:
        raise ValueError("mbk_fit: bad arguments")
    return lab, {"n_steps": int(info[0]), "centers": C, "picks": picks.astype(np.int64), "init_indices": init_idx,
                 "mt_words": int(info[2]), "n_reassigned": int(info[3])}


def kmeanspp_picks_native(points, k, seed=42, threads=0):
    """k-means++ picks of the MiniBatchKMeans init alone (positions in the init sample, draw order) + the sample rows."""
    P = np.ascontiguousarray(np.asarray(points).reshape(-1, 3).astype(np.uint8))
    n = len(P)
    picks = np.empty(k, np.int32)
    init_idx = np.empty(_mbk_init_size(n, k), np.int64)
    rc = _km64_lib().mbk_init_picks(P.ctypes.data, n, int(k), int(seed), int(threads), picks.ctypes.data, init_idx.ctypes.data)
    if rc:
        raise ValueError("mbk_init_picks: bad arguments")
    return picks.astype(np.int64), init_idx


def km64_estep(X, C, want_dist=False):
    """first arg-min_j of ||c_j||^2 + (-2) fma(x2,c2,fma(x1,c1,x0*c0)), ||c||^2 = (c0^2+c2^2)+c1^2."""
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)
    C = np.ascontiguousarray(C, dtype=np.float64).reshape(-1, 3)
    lab = np.empty(len(X), np.int32)
    dist = np.empty(len(X), np.float64) if want_dist else None
    _km64_lib().km64_estep(X.ctypes.data, len(X), C.ctypes.data, len(C), lab.ctypes.data, dist.ctypes.data if want_dist else None)
    return (lab, dist) if want_dist else lab



# --------------------------------------------------------------------------------------
# K1: unique colours  (encoder/compression/clustering.py:21-48)
# --------------------------------------------------------------------------------------
def pack_rgb(rgb):
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3).astype(np.uint32)
    return (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]


def unpack_rgb(keys):
    keys = np.asarray(keys, dtype=np.uint32)
    return np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], axis=1).astype(np.uint8)


def unique_colors(image):
    """palette = rows of np.unique(pixels, axis=0) (ascending lexicographic R,G,B);
    indices[p] = rank of pixel p's colour (clustering.py:21-48).  Returns
    (uint8[P,3], int32[h*w]); None for an empty image (clustering.py:9-10)."""
    image = np.asarray(image)
    if image.size == 0:
        return None
    keys = pack_rgb(image)
    u, inv = np.unique(keys, return_inverse=True)
    return unpack_rgb(u), inv.astype(np.int32).reshape(-1)


# --------------------------------------------------------------------------------------
# parameters  (clustering.py:108-135)
# --------------------------------------------------------------------------------------
def clustering_params(n_colors, quality):
    """eps = 128 - 1.28 q ; mc = ceil((-(q/100) n + n)/q); zeros -> 1; min_samples = 1.
    quality 0 raises ZeroDivisionError like the reference (clustering.py:129)."""
    eps = 128 - 1.28 * quality
    mc = math.ceil((-(quality / 100) * n_colors + n_colors) / quality)
    if eps == 0:
        eps = 1
    if mc == 0:
        mc = 1
    return eps, 1, mc


# --------------------------------------------------------------------------------------
# K3/K4: DBSCAN(min_samples=1) == connected components of the eps graph
# (clustering.py:204-205,233-235)
# --------------------------------------------------------------------------------------
def eps_threshold(eps):
    """Integer form of sklearn's float64 test sum((a/255-b/255)^2) <= (eps/255)^2.

    Returns (thr, boundary): pairs with integer d2 <= thr are neighbours; when
    `boundary` >= 0, pairs with d2 == boundary sit exactly on the radius and must be
    decided by the float64 expression (boundary_pair_is_neighbor)."""
    from fractions import Fraction
    exact = Fraction(float(eps)) ** 2                    # eps^2 in exact rational arithmetic
    if exact.denominator == 1:                          # integral: d2 == eps^2 sits on the radius
        b = int(exact)
        return b - 1, b
    return int(math.floor(exact)), -1


def boundary_pair_is_neighbor(a, b, eps):
    """The KD-tree leaf test of sklearn.neighbors (rdist <= r*r, sequential float64 sum)
    on the values the reference feeds it: c/255.0 and eps/255.0 (clustering.py:205,233)."""
    r = np.float64(eps) / np.float64(255.0)
    d = np.float64(0.0)
    for k in range(3):
        t = np.float64(a[k]) / np.float64(255.0) - np.float64(b[k]) / np.float64(255.0)
        d = d + t * t
    return bool(d <= r * r)


def eps_components(colors, eps):
    """Labels of sklearn DBSCAN(eps/255, min_samples=1) on colors/255: connected
    components of {d2 <= eps^2}; a component's label is the rank of its smallest member
    index (dbscan_inner visits points in index order).  int32[N]."""
    colors = np.asarray(colors, dtype=np.int64).reshape(-1, 3)
    n = len(colors)
    if n == 0:
        return np.zeros(0, np.int32)
    thr, boundary = eps_threshold(eps)
    f = colors.astype(np.float64) / np.float64(255.0)
    r = np.float64(eps) / np.float64(255.0)
    r2 = r * r
    lab = np.arange(n)
    B = 1024
    while True:                                           # min-label propagation + pointer jumping
        new = lab.copy()
        for s in range(0, n, B):
            a = colors[s:s + B]
            d2 = ((a[:, None, :] - colors[None, :, :]) ** 2).sum(-1)
            adj = d2 <= thr
            if boundary >= 0:
                bi, bj = np.nonzero(d2 == boundary)
                if len(bi):
                    t = f[s + bi] - f[bj]
                    d = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
                    adj[bi, bj] = d <= r2
            new[s:s + B] = np.where(adj, lab[None, :], n).min(1)
        while True:
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, lab):
            break
        lab = new
    # lab[i] = smallest member index of i's component; dense rank in order of that index
    roots, inv = np.unique(lab, return_inverse=True)
    return inv.astype(np.int32)


# --------------------------------------------------------------------------------------
# K7: KMeans(n_clusters=k, random_state=42, n_init='auto')  (clustering.py:751-752)
# --------------------------------------------------------------------------------------
def _choice_uniform(rs, n):
    """numpy legacy RandomState.choice(n, p=ones/n): cdf = cumsum(p); cdf /= cdf[-1];
    searchsorted(cdf, random_sample(), 'right')."""
    p = np.full(n, 1.0) / np.float64(n)
    cdf = np.cumsum(p)
    cdf /= cdf[-1]
    return int(np.searchsorted(cdf, rs.random_sample(), side="right"))


def kmeanspp_int(points, k, rs):
    """Greedy k-means++ (sklearn.cluster._kmeans._kmeans_plusplus) on integer points with
    exact integer squared distances.  Returns the chosen point indices int64[k]."""
    P = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    n = len(P)
    T = 2 + int(np.log(k))
    idx = np.empty(k, np.int64)
    first = min(_choice_uniform(rs, n), n - 1)
    idx[0] = first
    closest = ((P - P[first]) ** 2).sum(1)            # exact ints
    pot = int(closest.sum())
    for c in range(1, k):
        rand_vals = rs.uniform(size=T) * np.float64(pot)
        cum = np.cumsum(closest).astype(np.float64)   # exact (< 2^53)
        cand = np.searchsorted(cum, rand_vals)         # side='left'
        np.clip(cand, None, n - 1, out=cand)
        d = ((P[cand][:, None, :] - P[None, :, :]) ** 2).sum(-1)
        np.minimum(d, closest[None, :], out=d)
        pots = d.sum(1)
        b = int(np.argmin(pots))
        pot = int(pots[b])
        closest = d[b]
        idx[c] = cand[b]
    return idx


def _km64_dist(X, C):
    """dist(i,j) = csq_j + (-2*((x0*c0 + x1*c1) + x2*c2)), each op rounded once."""
    csq = (C[:, 0] * C[:, 0] + C[:, 1] * C[:, 1]) + C[:, 2] * C[:, 2]
    dot = (X[:, None, 0] * C[None, :, 0] + X[:, None, 1] * C[None, :, 1]) + X[:, None, 2] * C[None, :, 2]
    return csq[None, :] + (-2.0 * dot)


def _argmin_first(D):
    return np.argmin(D, axis=1).astype(np.int32)      # numpy argmin returns the first minimum


def kmeans_labels(points, k, seed=42, max_iter=300, return_info=False):
    """Restatement of KMeans(k, random_state=seed, n_init=1, algorithm='lloyd',
    tol=1e-4).fit_predict(points.astype(float)) in KM64 arithmetic.  int32[n]."""
    P = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    n = len(P)
    assert 1 <= k <= n
    rs = np.random.RandomState(seed)
    S = P.sum(0)
    m = S.astype(np.float64) / np.float64(n)
    X = P.astype(np.float64) - m
    # tol = mean(var(X, axis=0)) * 1e-4 ; var from exact integers: (n*sum(p^2) - sum(p)^2) / n^2
    num = n * (P * P).sum(0) - S * S
    var = num.astype(np.float64) / (np.float64(n) * np.float64(n))
    tol = ((var[0] + var[1]) + var[2]) / 3.0 * 1e-4
    init_idx = kmeanspp_int(P, k, rs)
    C = X[init_idx].copy()
    labels_old = np.full(n, -1, np.int32)
    strict = False
    n_iter = 0
    relocated = 0
    for it in range(max_iter):
        n_iter = it + 1
        labels = km64_estep(X, C)
        cnt = np.bincount(labels, minlength=k).astype(np.int64)
        Sj = np.zeros((k, 3), np.int64)
        np.add.at(Sj, labels, P)
        empty = np.nonzero(cnt == 0)[0]
        if len(empty):
            # sklearn _relocate_empty_clusters_dense: the n_empty points farthest from their
            # own centre are moved; canonical order = (distance desc, index asc).
            diff = X - C[labels]
            dist = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
            if dist.max() > 0:
                far = np.lexsort((np.arange(n), -dist))[:len(empty)]
                for e, f in zip(empty, far):
                    old = labels[f]
                    Sj[old] -= P[f]; cnt[old] -= 1
                    Sj[e] = P[f]; cnt[e] = 1
                    relocated += 1
        Cn = C.copy()
        nz = cnt > 0
        Cn[nz] = Sj[nz].astype(np.float64) / cnt[nz, None].astype(np.float64) - m
        if (~nz).any():                                # _average_centers: copy the heaviest centre
            Cn[~nz] = Cn[int(np.argmax(cnt))]
        dC = Cn - C
        shift = (dC[:, 0] * dC[:, 0] + dC[:, 1] * dC[:, 1]) + dC[:, 2] * dC[:, 2]
        C = Cn
        if np.array_equal(labels, labels_old):
            strict = True
            break
        tot = np.float64(0.0)
        for s in shift:                                # sequential sum over j
            tot = tot + s
        if tot <= tol:
            break
        labels_old = labels
    if not strict:
        labels = km64_estep(X, C)
    if return_info:
        return labels, {"n_iter": n_iter, "strict": strict, "relocated": relocated, "init_idx": init_idx}
    return labels


def split_large_cluster(colors, mc, kmeans=kmeans_labels):
    """clustering.py:720-775 -> list of index arrays (into `colors`), depth-first, child
    label order, each child <= mc unless it cannot be split (n <= 2)."""
    colors = np.asarray(colors).reshape(-1, 3)
    n = len(colors)
    me = np.arange(n)
    if n <= mc:
        return [me]
    n_splits = max(2, (n + mc - 1) // mc)
    n_splits = min(n_splits, n)
    if n <= 2 or n_splits < 2:
        return [me]
    labels = kmeans(colors, n_splits)
    out = []
    for i in range(n_splits):
        sub = me[labels == i]
        if len(sub) == 0:
            continue
        if len(sub) > mc:
            out.extend(sub[s] for s in split_large_cluster(colors[sub], mc, kmeans))
        else:
            out.append(sub)
    return out


# --------------------------------------------------------------------------------------
# K8: MiniBatchKMeans(k, batch_size=1000, random_state=42, n_init='auto')
# (clustering.py:207-230)
# --------------------------------------------------------------------------------------
def _mb_dist(Xb, C):
    """MiniBatch E-step distance on RAW coordinates (sklearn does not centre here)."""
    return _km64_dist(Xb, C)


def minibatch_kmeans_labels(points, k, seed=42, batch_size=1000, max_iter=100,
                            max_no_improvement=10, reassignment_ratio=0.01, return_info=False,
                            assign=None, max_steps=None, argsort=None):
    """Restatement of sklearn 1.7.2 MiniBatchKMeans(k, batch_size=1000, random_state=42, n_init='auto').fit
    (cluster/_kmeans.py; reference call site clustering.py:207-218), operation for operation, on integer colours:

      * RandomState(seed) is consumed exactly as sklearn consumes it: validation_indices = randint(0, n, init_size)
        (used for the stream position only: with n_init = 1 the validation inertia decides nothing), init_indices =
        randint(0, n, init_size), k-means++ over the init sample IN DRAW ORDER (choice(p=uniform) for the first centre,
        uniform(size=T) per further centre, exact integer distances -- kmeanspp_int), then per step
        randint(0, n, batch) and, when centres are reassigned, choice(batch, replace=False, size=n_reassign)
        (legacy permutation(batch)[:size]);
      * E-step: sklearn's chunked dgemm expression csq_j + (-2 * fma-chain dot) on raw 0..255 coordinates, first arg-min
        (km64_estep);
      * batch inertia (_inertia_dense): sum_i ((0 + d0^2) + d1^2) + d2^2 added SEQUENTIALLY in batch order -- what sklearn
        evaluates with one OpenMP thread (with more threads its partial sums are combined in arrival order: the last bits
        are not reproducible there; they only matter for the '<' of the EWA early-stopping rule);
      * centre update (_minibatch_update_dense / update_center_dense): per touched centre c*w, then += x for its batch
        members in batch order, w += count, c *= 1/w -- each operation rounded once, in that order;
      * reassignment (_mini_batch_step): to_reassign = w < ratio*max(w); when more than batch/2 qualify sklearn keeps
        np.argsort(w)[:batch/2] -- an UNSTABLE sort over massively tied counts whose tie order depends on which of
        numpy's three argsort kernels the host runs (AVX-512, AVX2, scalar).  `argsort` = "npysort" (default since round
        4): numpy's scalar aquicksort restated (npy_argsort.c) -- the whole fit then equals scikit-learn's UNTOUCHED
        fit_predict under NPY_DISABLE_CPU_FEATURES = <AVX512 family> AVX2 FMA3, the host setting of record (G11 "scalar");
        "stable" (rounds 1-3): the order (w asc, index asc) = sklearn with that one call forced to kind='stable';
      * early stopping: sklearn's EWA rule verbatim (tol = 0 => no centre-shift test).
    Returns labels int32[n] from a full E-step over all points (first arg-min)."""
    P = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    n = len(P)
    X = P.astype(np.float64)
    rs = np.random.RandomState(seed)
    bs = min(batch_size, n)
    init_size = 3 * bs
    if init_size < k:
        init_size = 3 * k
    init_size = min(init_size, n)
    rs.randint(0, n, init_size)                        # validation_indices (stream position only)
    init_indices = rs.randint(0, n, init_size) if init_size < n else np.arange(n)
    cidx = kmeanspp_int(P[init_indices], k, rs)        # sklearn's draw order
    C = X[init_indices[cidx]].copy()
    W = np.zeros(k, np.float64)
    ewa = None
    ewa_min = None
    no_impr = 0
    since = 0
    n_steps = (max_iter * n) // bs
    if max_steps is not None:
        n_steps = min(n_steps, max_steps)
    steps_done = 0
    n_reassigned = 0
    for s in range(n_steps):
        steps_done = s + 1
        bidx = rs.randint(0, n, bs)
        Xb = X[bidx]
        since += bs
        do_reassign = bool((W == 0).any() or since >= 10 * k)
        if do_reassign:
            since = 0
        lab = km64_estep(Xb, C)
        dd = Xb - C[lab]
        per = ((0.0 + dd[:, 0] * dd[:, 0]) + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
        inertia = np.add.accumulate(per)[-1]            # strictly sequential sum, batch order
        # update_center_dense, members in batch order: rank r of a batch row = number of earlier rows with its label
        order = np.argsort(lab, kind="stable")
        sl = lab[order]
        start = np.flatnonzero(np.concatenate([[True], sl[1:] != sl[:-1]]))
        seg_len = np.diff(np.concatenate([start, [len(sl)]]))
        rank = np.arange(len(sl)) - np.repeat(start, seg_len)
        touched = sl[start]
        Cn = C.copy()
        acc = C[touched] * W[touched, None]
        for r in range(int(seg_len.max())):
            m = rank == r
            rows = order[m]                              # one row per centre that has an r-th member
            tpos = np.searchsorted(touched, lab[rows])
            acc[tpos] = acc[tpos] + Xb[rows]
        W[touched] = W[touched] + seg_len.astype(np.float64)
        alpha = 1.0 / W[touched]
        Cn[touched] = acc * alpha[:, None]
        if do_reassign and reassignment_ratio > 0:
            to_re = W < reassignment_ratio * W.max()
            if to_re.sum() > 0.5 * bs:
                if (argsort or DEFAULT_ARGSORT) == "stable":
                    keep = np.argsort(W, kind="stable")[int(0.5 * bs):]
                else:                                                   # sklearn: np.argsort(W), numpy's scalar aquicksort
                    keep = npy_argsort_scalar(W)[int(0.5 * bs):]
                to_re[keep] = False
            nre = int(to_re.sum())
            if nre:
                new_centers = rs.choice(bs, replace=False, size=nre)
                Cn[to_re] = Xb[new_centers]
                n_reassigned += nre
            W[to_re] = np.min(W[~to_re])
        C = Cn
        # _mini_batch_convergence
        binert = inertia / bs
        if s + 1 == 1:
            continue
        if ewa is None:
            ewa = binert
        else:
            a = bs * 2.0 / (n + 1)
            a = min(a, 1)
            ewa = ewa * (1 - a) + binert * a
        if ewa_min is None or ewa < ewa_min:
            no_impr = 0
            ewa_min = ewa
        else:
            no_impr += 1
        if no_impr >= max_no_improvement:
            break
    if assign is None:
        labels = km64_estep(X, C)
    else:
        labels = assign(X, C)
    if return_info:
        return labels, {"n_steps": steps_done, "centers": C, "weights": W, "init_indices": init_indices, "picks": cidx,
                        "n_reassigned": n_reassigned, "mt_pos": mt_position(rs)}
    return labels


def mt_position(rs):
    """number of raw 32-bit MT19937 words a RandomState has consumed so far, assuming <= 2^31 (diagnostic: the GPU path
    reports its stream cursor, tests compare).  Derived from the generator state by replaying a twin from the seed is
    not possible in general, so this simply returns the in-block position; callers that need the absolute cursor
    count words themselves."""
    st = rs.get_state()
    return int(st[2])


# --------------------------------------------------------------------------------------
# cluster_palette_colors_parallel  (clustering.py:160-437)
# --------------------------------------------------------------------------------------
def dbscan_labels(colors, eps, min_samples):
    """sklearn DBSCAN(eps / 255, min_samples, 'euclidean').fit_predict(colors / 255) (clustering.py:233-235) for any min_samples:
    core points = at least min_samples points within eps, itself included; dbscan_inner seeds clusters at the core points in index
    order and grows them depth first through core points, labelling every point it reaches that has no label yet: clusters = the
    eps-components of the core points, numbered by their lowest core index; a non-core point is first reached from the cluster
    with the lowest number among its core neighbours; -1 = noise."""
    colors = np.asarray(colors, dtype=np.int64).reshape(-1, 3)
    n = len(colors)
    if n == 0:
        return np.zeros(0, np.int32)
    thr, boundary = eps_threshold(eps)
    f = colors.astype(np.float64) / np.float64(255.0)
    r = np.float64(eps) / np.float64(255.0)
    adj = np.zeros((n, n), bool)
    for s0 in range(0, n, 1024):
        a = colors[s0:s0 + 1024]
        d2 = ((a[:, None, :] - colors[None, :, :]) ** 2).sum(-1)
        blk = d2 <= thr
        if boundary >= 0:
            bi, bj = np.nonzero(d2 == boundary)
            if len(bi):
                t = f[s0 + bi] - f[bj]
                blk[bi, bj] = ((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]) <= r * r
        adj[s0:s0 + 1024] = blk
    core = adj.sum(1) >= min_samples
    labels = np.full(n, -1, np.int32)
    nxt = 0
    for i in range(n):                                        # dbscan_inner, literally
        if labels[i] != -1 or not core[i]:
            continue
        stack = [i]
        while stack:
            v = stack.pop()
            if labels[v] == -1:
                labels[v] = nxt
                if core[v]:
                    stack.extend(int(u) for u in np.nonzero(adj[v] & (labels == -1))[0])
        nxt += 1
    return labels


def cluster_palette(quality, palette, indices, eps, mc, kmeans=kmeans_labels,
                    minibatch=minibatch_kmeans_labels, return_info=False, min_samples=1):
    """Returns (new_palette uint8[K,3], new_indices int64[h*w]).

    Order of the new palette: black rows; clusters with size <= mc in
    ascending label order (floor-mean colour); then oversize clusters in ascending label order
    (reference: as_completed order, nondeterministic), each contributing its k-means children
    depth-first.  Old->new mapping for split children goes through the reference's
    find_color_index (first equal row, clustering.py:352-355,803-808), so a duplicated colour's
    later row is left unmapped (-> 0); mapping is stored in uint16 (clustering.py:373)."""
    palette = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
    indices = np.asarray(indices, dtype=np.int64).reshape(-1)
    P = len(palette)
    isblack = np.all(palette == 0, axis=1)
    black_idx = np.nonzero(isblack)[0]
    nb_idx = np.nonzero(~isblack)[0]
    info = {"branch": "none"}
    if len(nb_idx) == 0:                                   # clustering.py:197-199
        return (palette, indices, info) if return_info else (palette, indices)
    nb = palette[nb_idx]
    if len(nb) >= MINIBATCH_THRESHOLD:
        k = math.ceil(len(nb) * (quality / 100) / 10)
        labels = minibatch(nb, k)
        info["branch"] = "minibatch"
    else:
        labels = eps_components(nb, eps) if min_samples == 1 else dbscan_labels(nb, eps, min_samples)
        info["branch"] = "dbscan"
    new_pal = []
    mapping = np.zeros(P, np.uint16)                        # unmapped -> 0
    for b in black_idx:
        mapping[b] = len(new_pal) & 0xFFFF
        new_pal.append(palette[b])
    for rel in np.nonzero(labels == -1)[0]:                  # noise colours keep themselves (clustering.py:262-271)
        mapping[nb_idx[rel]] = len(new_pal) & 0xFFFF
        new_pal.append(palette[nb_idx[rel]])
    present = np.unique(labels[labels >= 0])
    keys = pack_rgb(palette)
    order = np.argsort(keys, kind="stable")
    sorted_keys = keys[order]

    def first_index_of(cols):
        """find_color_index: first palette row equal to the colour."""
        ck = pack_rgb(cols)
        # first occurrence in original order = smallest original index among equal keys
        pos = np.searchsorted(sorted_keys, ck, side="left")
        return order[pos]                                   # stable sort => smallest index first

    small, large = [], []
    for lab in present:
        rel = np.nonzero(labels == lab)[0]
        (large if len(rel) > mc else small).append(rel)
    info["n_clusters"] = len(present)
    info["n_large"] = len(large)
    for rel in small:
        cols = nb[rel].astype(np.int64)
        avg = (cols.sum(0) // len(rel)).astype(np.uint8)
        mapping[nb_idx[rel]] = len(new_pal) & 0xFFFF
        new_pal.append(avg)
    for rel in large:
        cols = nb[rel]
        for sub in split_large_cluster(cols, mc, kmeans):
            sc = cols[sub].astype(np.int64)
            avg = (sc.sum(0) // len(sub)).astype(np.uint8)
            mapping[first_index_of(cols[sub])] = len(new_pal) & 0xFFFF
            new_pal.append(avg)
    new_pal = np.array(new_pal, dtype=np.uint8).reshape(-1, 3)
    new_idx = mapping[indices].astype(np.int64)
    return (new_pal, new_idx, info) if return_info else (new_pal, new_idx)


# --------------------------------------------------------------------------------------
# K5: merge_region_components_simple  (merging.py:8-120)
# --------------------------------------------------------------------------------------
def merge_components(comps, bbox):
    """comps: list of dicts {top_left:(r,c), shape:(h,w), palette:uint8[K,3], indices:int[h*w]}.
    Returns None for an empty list, the single component (as-is, merging.py:16-21) for one, else
    {top_left, shape, palette, indices(int64 flat)} with black = index 0, colours in first-seen
    order scanning components last->first, each in raster order, earlier components winning."""
    if not comps:
        return None
    if len(comps) == 1:
        c = dict(comps[0])
        c["single"] = True
        return c
    minr, minc, maxr, maxc = (int(v) for v in bbox)
    H, W = maxr - minr, maxc - minc
    canvas = np.zeros((H, W), np.int64)
    colors = [0]                                           # packed keys, black first
    lut = {0: 0}
    for seg in reversed(comps):
        h, w = seg["shape"]
        pal = np.asarray(seg["palette"], dtype=np.uint8).reshape(-1, 3)
        idx = np.asarray(seg["indices"], dtype=np.int64).reshape(h, w)
        r0, c0 = seg["top_left"][0] - minr, seg["top_left"][1] - minc
        rr, cc = np.mgrid[0:h, 0:w]
        ok = (rr + r0 >= 0) & (rr + r0 < H) & (cc + c0 >= 0) & (cc + c0 < W) & (idx < len(pal)) & (idx >= 0)
        if len(pal) == 0:
            continue
        pk = pack_rgb(pal)[np.clip(idx, 0, len(pal) - 1)]
        ok &= pk != 0
        pkv = pk[ok]
        if pkv.size == 0:
            continue
        u, first = np.unique(pkv, return_index=True)
        for key in u[np.argsort(first)]:
            if int(key) not in lut:
                lut[int(key)] = len(colors)
                colors.append(int(key))
        gidx = np.array([lut[int(kk)] for kk in u])[np.searchsorted(u, pkv)]
        canvas[(rr + r0)[ok], (cc + c0)[ok]] = gidx
    return {"top_left": (minr, minc), "shape": (H, W), "palette": unpack_rgb(np.array(colors, dtype=np.uint32)),
            "indices": canvas.reshape(-1), "single": False}


# --------------------------------------------------------------------------------------
# K0/K0b + level-1 driver  (subregions.py:315-449,634-679)
# --------------------------------------------------------------------------------------
def segment_crop(region_image, segment_mask):
    """Tight bbox of the mask +-2 px clamped to the region, zero outside the mask, black pixels
    inside the mask replaced by the segment's non-black pixel of smallest R^2+G^2+B^2 (first in
    mask raster order) (subregions.py:338-421).  Returns (crop uint8[ch,cw,3], (r0,c0)) or None."""
    rows, cols = np.where(segment_mask)
    if len(rows) == 0:
        return None
    h, w = region_image.shape[:2]
    r0, r1 = max(0, rows.min() - 2), min(h - 1, rows.max() + 2)
    c0, c1 = max(0, cols.min() - 2), min(w - 1, cols.max() + 2)
    crop = region_image[r0:r1 + 1, c0:c1 + 1]
    m = segment_mask[r0:r1 + 1, c0:c1 + 1]
    out = np.zeros_like(crop)
    px = crop[m].copy()
    isb = np.all(px == 0, axis=1)
    if isb.any() and (~isb).any():
        nb = px[~isb].astype(np.int64)
        n2 = (nb * nb).sum(1)
        px[isb] = nb[int(np.argmin(n2))].astype(np.uint8)
    out[m] = px
    return out, (int(r0), int(c0))


def level1_region(image, bbox, bbox_mask, seglabels, quality, kmeans=kmeans_labels,
                  minibatch=minibatch_kmeans_labels):
    """One region of subregion_quantization (subregions.py:98-679) given its SLIC label map
    (0 = background, ids ascending as in extract_slic_segment_boundaries, slic.py:158-160).
    Returns the list the reference appends to subregions_components: [merged] or [components]."""
    minr, minc, maxr, maxc = bbox
    region_image = image[minr:maxr, minc:maxc]
    comps = []
    ids = np.unique(seglabels)
    for sid in ids[ids != 0]:
        segmask = (seglabels == sid) & bbox_mask
        res = segment_crop(region_image, segmask)
        if res is None:
            continue
        crop, (r0, c0) = res
        pal, idx = unique_colors(crop)
        eps, _, mc = clustering_params(len(pal), quality)
        npal, nidx = cluster_palette(quality, pal, idx, eps, mc, kmeans, minibatch)
        comps.append({"top_left": (r0 + minr, c0 + minc), "shape": crop.shape[:2], "palette": npal, "indices": nidx})
    if len(comps) > 1:
        return [merge_components(comps, (minr, minc, maxr, maxc))]
    return comps


def region_quantization(components, H, W, quality, kmeans=kmeans_labels, minibatch=minibatch_kmeans_labels):
    """regions.py:9-70: merge all components of one class on the full-image canvas, cluster."""
    merged = merge_components(components, (0, 0, H, W))
    if merged is None:
        raise IndexError("no components")                 # regions.py:43 regions_image[0]
    pal = np.asarray(merged["palette"], dtype=np.uint8).reshape(-1, 3)
    eps, _, mc = clustering_params(len(pal), quality)
    npal, nidx = cluster_palette(quality, pal, merged["indices"], eps, mc, kmeans, minibatch)
    return {"top_left": merged["top_left"], "shape": merged["shape"], "palette": npal, "indices": nidx}


def optimal_index_dtype(indices):
    """compression.py:360-372: by max index."""
    mx = int(np.max(indices)) if len(indices) else 0
    return "uint8" if mx < 256 else ("uint16" if mx < 65536 else "uint32")


def quantize_image(components, H, W, quality, kmeans=kmeans_labels, minibatch=minibatch_kmeans_labels):
    """image.py:243-286."""
    out = region_quantization(components, H, W, quality, kmeans, minibatch)
    out["indices_dtype"] = optimal_index_dtype(out["indices"])
    return out


def encode_frame(image, classes, qualities, kmeans=kmeans_labels, minibatch=minibatch_kmeans_labels):
    """Three-level chain of rhccq.ipynb:978-1039.

    classes: list (ROI first, then non-ROI) of lists of regions, each region a dict
    {bbox:(minr,minc,maxr,maxc), bbox_mask: bool[h,w], seglabels: int32[h,w] (0 = background)}.
    qualities: per-class level-1 quality.  Returns dict with per-level results."""
    H, W = image.shape[:2]
    lvl2 = []
    l1_all = []
    q2s = []
    for regions, q in zip(classes, qualities):
        l1 = []
        for reg in regions:
            l1.extend(level1_region(image, reg["bbox"], reg["bbox_mask"], reg["seglabels"], q, kmeans, minibatch))
        l1_all.append(l1)
        q2 = min(q * 2, 100)
        q2s.append(q2)
        try:
            lvl2.append(region_quantization(l1, H, W, q2, kmeans, minibatch))
        except IndexError:                                  # rhccq.ipynb:1009-1013 swallows
            pass
    q3 = min(sum(q2s), 100)
    fin = quantize_image(lvl2, H, W, q3, kmeans, minibatch)
    return {"level1": l1_all, "level2": lvl2, "final": fin}


# --------------------------------------------------------------------------------------
# The image -> .rhccq script flow (encoder/compression/test.py:77-151) and the glue of subregion_quantization between the
# upstream stages and level 1 (subregions.py:90-161,315-317,634-679; slic.py:143-214).  Stated from the oracle's own
# stage functions; the ROI and SLIC stages inherit their PARITY UNPINNED status.
# --------------------------------------------------------------------------------------
def region_segment_count(region_image, bbox_mask):
    """subregions.py:125-161: split score -> window -> ceil(normalize_result) -> at least 1.
    Returns (optimal_segments, normalize_result value, overall split score)."""
    overall = split_score(region_image, bbox_mask)[0]        # 0 below 100 masked pixels (split_score.py:25-27)
    size = region_image.size                                  # h * w * 3
    window = math.ceil(math.ceil(math.log(size, 10)) * math.log(size))
    nr = normalize_result(overall, window)
    optimal = math.ceil(nr)
    if optimal <= 0:
        optimal = 1
    return optimal, nr, overall


def find_contours_drops(segment_mask):
    """slic.py:164-206 for one segment mask of the region box's shape.  A box thinner than 2 px takes the tiny-segment branch
    and is always kept.  Otherwise skimage.measure.find_contours(mask, 0.5) finds a contour iff some neighbouring pixels
    differ; a mask without a level crossing is constant, i.e. (it is not empty) fills the box, and is skipped."""
    rows, cols = segment_mask.shape
    if rows < 2 or cols < 2:
        return False
    return bool(segment_mask.all())


def kept_segments(seglabels, bbox_mask):
    """extract_slic_segment_boundaries' ids in ascending order (slic.py:158-160), without empty and dropped segments.
    Returns (kept ids, dropped ids, label map restricted to the mask with only the kept ids left)."""
    seglabels = np.asarray(seglabels)
    bbox_mask = np.asarray(bbox_mask, bool)
    kept, dropped = [], []
    ids = np.unique(seglabels)
    for sid in ids[ids != 0]:
        m = (seglabels == sid) & bbox_mask
        if not m.any():
            continue
        (dropped if find_contours_drops(m) else kept).append(int(sid))
    out = np.where(bbox_mask & np.isin(seglabels, kept), seglabels, 0).astype(np.int32)
    return kept, dropped, out


def script_flow(image, roi_quality=20, nonroi_quality=10, kmeans=kmeans_labels, minibatch=minibatch_kmeans_labels):
    """encoder/compression/test.py:77-151: get_regions -> extract_regions -> subregion_quantization per class ->
    region_quantization per class (any exception of either call swallowed: the script's bare `except:`) -> quantize_image
    (not guarded: an image without any component raises here) -> lossless_compress_optimized -> save_compressed.

    Returns a dict of every intermediate: region_map, roi_regions / nonroi_regions (bbox, area, type, bbox_mask),
    per class and region the segment count, normalize_result value, kept / dropped SLIC ids and the label map after drops
    ("regions"), level1 per class (one list per region, as subregion_quantization returns it), level2 per class (None where
    region_quantization raised, with the exception's type name in level2_error), final, pkg and the file bytes."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    H, W = image.shape[:2]
    unified, region_map, _, _, roi_mask, non_mask = get_regions(image)
    roi_regions, nonroi_regions = extract_regions(image, roi_mask, non_mask)
    out = {"region_map": np.asarray(region_map), "roi_regions": roi_regions, "nonroi_regions": nonroi_regions}
    per_class, level1, level2, errors = [], [], [], []
    for regions, q in ((roi_regions, roi_quality), (nonroi_regions, nonroi_quality)):
        info, l1 = [], []
        for region in regions:
            minr, minc, maxr, maxc = region["bbox"]
            bbox_region = image[minr:maxr, minc:maxc]
            bbox_mask = np.asarray(region["bbox_mask"], bool)
            n_seg, nr, overall = region_segment_count(bbox_region, bbox_mask)
            seglabels = enhanced_slic(bbox_region, bbox_mask, n_segments=n_seg)
            kept, dropped, labels = kept_segments(seglabels, bbox_mask)
            info.append({"n_segments": n_seg, "normalize_result": nr, "split_score": overall, "kept": kept, "dropped": dropped,
                         "labels": labels})
            l1.append(level1_region(image, region["bbox"], bbox_mask, labels, q, kmeans, minibatch))
        per_class.append(info)
        level1.append(l1)
        q2 = min(q * 2, 100)
        try:
            level2.append(region_quantization([c for comps in l1 for c in comps], H, W, q2, kmeans, minibatch))
            errors.append(None)
        except Exception as e:                                   # noqa: BLE001  (test.py:128-132: bare except)
            level2.append(None)
            errors.append(type(e).__name__)
    out.update(regions=per_class, level1=level1, level2=level2, level2_error=errors)
    q3 = min(min(roi_quality * 2, 100) + min(nonroi_quality * 2, 100), 100)
    final = quantize_image([c for c in level2 if c is not None], H, W, q3, kmeans, minibatch)
    pkg = pack_container(final["palette"], final["indices"], final["shape"])
    out.update(final=final, pkg=pkg, file_bytes=container_bytes(pkg))
    return out


# --------------------------------------------------------------------------------------
# container  (compression.py:10-22,119-142,151-220 ; uncompression.py:58-150)
# --------------------------------------------------------------------------------------
def pack_container(palette, indices, shape):
    """lossless_compress_optimized: dict {s,l,p,i,d}."""
    palette = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
    indices = np.asarray(indices).reshape(-1)
    d = optimal_index_dtype(indices)
    return {"s": tuple(int(v) for v in shape), "l": len(palette),
            "p": zlib.compress(palette.tobytes(), 9),
            "i": zlib.compress(indices.astype(d).tobytes(), 9), "d": d}


def container_bytes(pkg):
    """save_compressed: b'RHCCQ' + <I len + zlib9(pickle5(pkg))."""
    body = zlib.compress(pickle.dumps(pkg, protocol=5), 9)
    return b"RHCCQ" + struct.pack("<I", len(body)) + body


class _SafeUnpickler(pickle.Unpickler):
    _OK = {("numpy._core.multiarray", "scalar"), ("numpy.core.multiarray", "scalar"), ("numpy", "dtype")}

    def find_class(self, module, name):
        if (module, name) in self._OK:
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"forbidden global {module}.{name}")


def load_container(raw):
    if raw[:5] != b"RHCCQ":
        raise ValueError("Invalid file format")
    n = struct.unpack("<I", raw[5:9])[0]
    return _SafeUnpickler(io.BytesIO(zlib.decompress(raw[9:9 + n]))).load()


def decode_container(pkg):
    h, w = int(pkg["s"][0]), int(pkg["s"][1])
    pal = np.frombuffer(zlib.decompress(pkg["p"]), np.uint8).reshape(-1, 3)
    idx = np.frombuffer(zlib.decompress(pkg["i"]), np.dtype(pkg.get("d", "uint16")))
    return pal, idx, (h, w)


# --------------------------------------------------------------------------------------
# EXTENSION (no reference counterpart; named by BASELINE.json's north_star only): pixel-space DBSCAN on
# (x, y, L, a, b).  Brute-force restatement of csrc/px_dbscan_ext.hip's definition: every float32 operation is
# written in the same order (and both sides read the same two tables), so counts, core flags and labels must be
# bit-identical.
# --------------------------------------------------------------------------------------
def px_lab(rgb, tables):
    """float32 Lab planes of a uint8 image with the operation order of px_lab() in px_dbscan_ext.hip;
    tables = float32[256 + 2048]: sRGB -> linear, then (f(i/1024), df) pairs interpolated linearly"""
    f = np.float32
    lin, fd = tables[:256], tables[256:].reshape(-1, 2)
    r, g, b = lin[rgb[..., 0]], lin[rgb[..., 1]], lin[rgb[..., 2]]
    X = ((f(0.4124564) * r + f(0.3575761) * g) + f(0.1804375) * b) * f(1.0521111)
    Y = (f(0.2126729) * r + f(0.7151522) * g) + f(0.0721750) * b
    Z = ((f(0.0193339) * r + f(0.1191920) * g) + f(0.9503041) * b) * f(0.9184170)

    def fn(t):
        u = t * f(1024.0)
        i = np.minimum(u.astype(np.int32), 1023)
        frac = u - i.astype(np.float32)
        return fd[i, 0] + frac * fd[i, 1]
    fx, fy, fz = fn(X), fn(Y), fn(Z)
    return f(116.0) * fy - f(16.0), f(500.0) * (fx - fy), f(200.0) * (fy - fz)


def px_dbscan(rgb, radius, eps, spatial_weight, min_pts, lut):
    """labels int32[H,W] (0 noise, else 1 + smallest pixel index of the cluster), core bool[H,W], counts"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.float32
    H, W = rgb.shape[:2]
    L, A, B = px_lab(rgb, np.asarray(lut, np.float32))
    eps2 = f(eps) * f(eps)
    ws2 = f(spatial_weight) * f(spatial_weight)
    offs = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)
            if dx * dx + dy * dy <= radius * radius and abs(dy) < H and abs(dx) < W]      # larger shifts leave the image
    idx = np.arange(H * W).reshape(H, W)
    near = {}
    count = np.zeros((H, W), np.int64)
    for dy, dx in offs:
        ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
        yq, xq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
        dL, dA, dB = L[ys, xs] - L[yq, xq], A[ys, xs] - A[yq, xq], B[ys, xs] - B[yq, xq]
        d2 = ((dL * dL + dA * dA) + dB * dB) + ws2 * f(dx * dx + dy * dy)
        m = np.zeros((H, W), bool)
        m[ys, xs] = d2 <= eps2
        near[(dy, dx)] = m
        count += m
    core = count >= min_pts
    rows, cols = [], []
    for (dy, dx), m in near.items():
        if (dy, dx) == (0, 0):
            continue
        ys, xs = np.nonzero(m & core)
        q_core = core[ys + dy, xs + dx]
        rows.append(idx[ys[q_core], xs[q_core]])
        cols.append(idx[ys[q_core] + dy, xs[q_core] + dx])
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    g = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(H * W, H * W))
    _, comp = connected_components(g, directed=False)
    root = np.full(comp.max() + 1, H * W, np.int64)
    np.minimum.at(root, comp, np.arange(H * W))
    name = (root[comp] + 1).reshape(H, W)
    labels = np.where(core, name, 0)
    best = np.full((H, W), np.iinfo(np.int64).max)
    for (dy, dx), m in near.items():
        if (dy, dx) == (0, 0):
            continue
        ys, xs = np.nonzero(m & ~core)
        q_core = core[ys + dy, xs + dx]
        ys, xs = ys[q_core], xs[q_core]
        np.minimum.at(best, (ys, xs), name[ys + dy, xs + dx])
    border = ~core & (best < np.iinfo(np.int64).max)
    labels = np.where(border, best, labels)
    return labels.astype(np.int32), core, np.minimum(count, 255).astype(np.uint8)


# --------------------------------------------------------------------------------------
# Quality metrics (decoder/uncompression/comparison.py:30-80).  PARITY UNPINNED for ssim / psnr: the
# reference calls scikit-image (absent from the build container, unpinned in requirements.txt), so these
# restate scikit-image's published algorithm with scipy.ndimage.uniform_filter (the routine it calls).
# --------------------------------------------------------------------------------------
def structural_similarity_win7(x, y):
    """skimage.metrics.structural_similarity(x, y, data_range=255, win_size=7) for one 2-D uint8 channel:
    uniform filter, sample covariance (cov_norm = NP / (NP - 1)), K1 = 0.01, K2 = 0.03, mean over the
    region a full window fits (crop by (win_size - 1) // 2)."""
    from scipy.ndimage import uniform_filter
    if min(x.shape) < 7:
        raise ValueError("win_size exceeds image extent")
    x = x.astype(np.float64)
    y = y.astype(np.float64)
    NP = 49
    cov_norm = NP / (NP - 1)
    ux = uniform_filter(x, size=7)
    uy = uniform_filter(y, size=7)
    uxx = uniform_filter(x * x, size=7)
    uyy = uniform_filter(y * y, size=7)
    uxy = uniform_filter(x * y, size=7)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    R = 255.0
    C1 = (0.01 * R) ** 2
    C2 = (0.03 * R) ** 2
    A1, A2, B1, B2 = (2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2)
    S = (A1 * A2) / (B1 * B2)
    pad = 3
    return S[pad:-pad, pad:-pad].mean(dtype=np.float64)


def quality_metrics(original, reconstructed):
    """calculate_quality_metrics (comparison.py:30-80): same keys, same dtypes (float32 statistics of float32
    arrays; float64 psnr / ssim as scikit-image returns them)."""
    of = original.astype(np.float32)
    rf = reconstructed.astype(np.float32)
    m = {}
    err = np.mean((original.astype(np.float64) - reconstructed.astype(np.float64)) ** 2, dtype=np.float64)
    with np.errstate(divide="ignore"):
        m["psnr"] = 10 * np.log10((255.0 ** 2) / err)            # skimage.metrics.peak_signal_noise_ratio
    try:
        m["ssim"] = np.mean([structural_similarity_win7(original[..., c], reconstructed[..., c]) for c in range(3)])
    except ValueError:
        m["ssim"] = np.float64(0.0)                              # comparison.py:51-61 falls back to zeros per channel
    m["mse"] = np.mean((of - rf) ** 2)
    m["rmse"] = np.sqrt(m["mse"])
    m["mae"] = np.mean(np.abs(of - rf))
    m["max_error"] = np.max(np.abs(of - rf))
    for i, ch in enumerate("rgb"):
        m[f"mse_{ch}"] = np.mean((of[..., i] - rf[..., i]) ** 2)
    return m


def adaptive_quality_metrics(original, reconstructed):
    """calculate_adaptive_quality_metrics (comparison.py:345-536), numpy statement for statement; SSIM through
    structural_similarity_win7 (scikit-image restated: parity unpinned)"""
    of, rf = original.astype(np.float32), reconstructed.astype(np.float32)
    abs_error = np.abs(of - rf)
    e = np.max(abs_error, axis=2).flatten()
    st = {"min": float(np.min(e)), "max": float(np.max(e)), "mean": float(np.mean(e)), "median": float(np.median(e)), "std": float(np.std(e)),
          "q75": float(np.percentile(e, 75)), "q90": float(np.percentile(e, 90)), "q95": float(np.percentile(e, 95)), "q99": float(np.percentile(e, 99))}
    q1, q3 = np.percentile(e, 25), np.percentile(e, 75)
    thr = {"iqr": q3 + 2.5 * (q3 - q1), "percentile": np.percentile(e, 99)}
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (e - st["mean"]) / st["std"]
    thr["adaptive"] = st["median"] + 3 * st["std"] if st["mean"] > st["median"] * 1.5 else st["mean"] + 2.5 * st["std"]
    masks = {"iqr": e > thr["iqr"], "zscore": np.abs(z) > 3.0, "percentile": e > thr["percentile"], "adaptive": e > thr["adaptive"]}
    thr["zscore"] = st["mean"] + 3.0 * st["std"]
    best_method, best = None, None
    for name, mk in masks.items():
        if 0.1 <= np.sum(mk) / len(e) * 100 <= 10.0:
            best_method, best = name, mk
            break
    if best_method is None:
        best_method, best = "adaptive", masks["adaptive"]
    oc = int(np.sum(best))
    m = {"error_distribution": st,
         "outlier_detection": {"method": best_method, "threshold": float(thr[best_method]), "outlier_count": oc,
                               "outlier_percentage": float(oc / len(e) * 100), "inlier_count": int(len(e) - oc),
                               "inlier_percentage": float(100 - oc / len(e) * 100)}}
    mse_all = np.mean((of - rf) ** 2)
    m["all_pixels"] = {"psnr": 10 * np.log10(255 * 255 / mse_all) if mse_all > 0 else float("inf"), "mse": float(mse_all),
                       "rmse": float(np.sqrt(mse_all)), "mae": float(np.mean(abs_error)), "max_error": st["max"], "pixel_count": int(len(e))}
    if 0 < oc < len(e):
        oi, ri = of.reshape(-1, 3)[~best], rf.reshape(-1, 3)[~best]
        mi = np.mean((oi - ri) ** 2)
        m["without_outliers"] = {"psnr": 10 * np.log10(255 * 255 / mi) if mi > 0 else float("inf"), "mse": float(mi), "rmse": float(np.sqrt(mi)),
                                 "mae": float(np.mean(np.abs(oi - ri))), "max_error": float(np.max(np.abs(oi - ri))), "pixel_count": int(len(oi))}
    for p in (99, 95, 90, 75):
        t = np.percentile(e, p)
        mk = e <= t
        op, rp = of.reshape(-1, 3)[mk], rf.reshape(-1, 3)[mk]
        if len(op) > 0:
            mp = np.mean((op - rp) ** 2)
            m[f"percentile_{p}"] = {"psnr": 10 * np.log10(255 * 255 / mp) if mp > 0 else float("inf"), "mse": float(mp),
                                    "max_error_included": float(t), "pixel_count": int(len(op)), "percentage": float(p)}
    try:
        m["ssim"] = {"full": float(np.mean([structural_similarity_win7(original[..., c], reconstructed[..., c]) for c in range(3)]))}
        if 0 < oc < len(e):
            h, w = original.shape[:2]
            om, rm = original.copy(), reconstructed.copy()
            om[best.reshape(h, w)] = 128
            rm[best.reshape(h, w)] = 128
            m["ssim"]["without_outliers"] = float(np.mean([structural_similarity_win7(om[..., c], rm[..., c]) for c in range(3)]))
    except ValueError:
        m["ssim"] = {"full": 0}
    hist, edges = np.histogram(e, bins=50)
    m["error_histogram"] = {"bins": hist.tolist(), "bin_edges": edges.tolist()}
    return m


# --------------------------------------------------------------------------------------
# Split score (encoder/subregions/split_score.py:15-142), SURVEY 8f-2.  PARITY UNPINNED: the reference calls
# scikit-image (rgb2lab, rgb2gray, filters.sobel, feature.local_binary_pattern), absent from the build container and unpinned
# in requirements.txt; these functions restate scikit-image's published algorithms.
# --------------------------------------------------------------------------------------
def sk_rgb2gray(rgb_u8):
    """skimage.color.rgb2gray on a uint8 image: img_as_float (v / 255) then the Rec. 709 weights 0.2125, 0.7154, 0.0721"""
    f = rgb_u8.astype(np.float64) / 255.0
    return (f[..., 0] * 0.2125 + f[..., 1] * 0.7154) + f[..., 2] * 0.0721


def sk_rgb2lab(rgb_u8):
    """skimage.color.rgb2lab (D65, 2 degree observer): sRGB companding, CIE RGB -> XYZ matrix, white-point scaling,
    f(t) = cbrt(t) above 0.008856 else 7.787 t + 16/116"""
    a = rgb_u8.astype(np.float64) / 255.0
    lin = np.where(a > 0.04045, np.power((a + 0.055) / 1.055, 2.4), a / 12.92)
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    xyz = [(M[i, 0] * r + M[i, 1] * g) + M[i, 2] * b for i in range(3)]
    white = (0.95047, 1.0, 1.08883)
    f = []
    for v, w in zip(xyz, white):
        t = v / w
        f.append(np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0))
    return np.stack([116.0 * f[1] - 16.0, 500.0 * (f[0] - f[1]), 200.0 * (f[1] - f[2])], axis=-1)


def sk_sobel(img):
    """skimage.filters.sobel of a 2-D float image: sqrt((h^2 + v^2) / 2), h / v = the [1,2,1]/4 smoothed central differences,
    borders by scipy.ndimage's 'reflect' (d c b a | a b c d | d c b a)"""
    p = np.pad(img, 1, mode="symmetric")
    sm_r = (p[:-2, :] + 2.0 * p[1:-1, :] + p[2:, :]) / 4.0          # smoothed along rows, for the column difference
    sm_c = (p[:, :-2] + 2.0 * p[:, 1:-1] + p[:, 2:]) / 4.0
    v = sm_r[:, 2:] - sm_r[:, :-2]
    h = sm_c[2:, :] - sm_c[:-2, :]
    return np.sqrt((h * h + v * v) / 2.0)


def sk_lbp_uniform_8_1(gray):
    """skimage.feature.local_binary_pattern(gray, 8, 1, method='uniform'): 8 points on the unit circle (coordinates rounded
    to 5 decimals), bilinear interpolation with zeros outside the image, bit = (value - centre >= 0); at most two 0/1
    transitions around the circle -> number of ones, else 9"""
    H, W = gray.shape
    pad = np.zeros((H + 4, W + 4))
    pad[2:-2, 2:-2] = gray
    bits = []
    for pnt in range(8):
        rp = np.round(-np.sin(2 * np.pi * pnt / 8), 5)
        cp = np.round(np.cos(2 * np.pi * pnt / 8), 5)
        r0, c0 = int(np.floor(rp)), int(np.floor(cp))
        r1, c1 = int(np.ceil(rp)), int(np.ceil(cp))
        dr, dc = rp - r0, cp - c0

        def px(dy, dx):
            return pad[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]
        top = (1 - dc) * px(r0, c0) + dc * px(r0, c1)
        bottom = (1 - dc) * px(r1, c0) + dc * px(r1, c1)
        val = (1 - dr) * top + dr * bottom
        bits.append((val - gray >= 0).astype(np.int32))
    bits = np.stack(bits)
    changes = sum(np.abs(bits[i] - bits[(i + 1) % 8]) for i in range(8))
    return np.where(changes <= 2, bits.sum(0), 9)


def split_stats(region_image, mask=None):
    """The masked statistics calculate_split_score reduces its scores from, in the order of csrc/split_score.hip:
    (sums[12] = count, sum L, L^2, A, A^2, B, B^2, gm, sg, sg^2, g, g^2; lbp_hist int64[10]; gray_hist int64[32]; abs_sums[12]).
    gm = the summed Lab gradient magnitude of split_score.py:47-50, sg = sobel(gray), g = gray; mask=None -> gray > 0.01.  Per-pixel
    terms in float64 from sk_rgb2gray / sk_rgb2lab / sk_sobel / sk_lbp_uniform_8_1, the sums in np.longdouble (rounded to float64
    once), so that they carry no summation-order error; abs_sums[q] = the sum of |term_q|, the scale of a summation error."""
    gray = sk_rgb2gray(region_image)
    if mask is None:
        mask = gray > 0.01
    mask = np.asarray(mask, bool)
    lab = sk_rgb2lab(region_image)
    gm = 0
    for c in range(3):
        s = sk_sobel(lab[:, :, c])
        gm = gm + np.sqrt(s ** 2 + s ** 2)
    sg = sk_sobel(gray)
    L, A, B = (lab[..., c][mask] for c in range(3))
    g, gm, sg = gray[mask], np.broadcast_to(gm, gray.shape)[mask], sg[mask]
    terms = [np.ones(len(g)), L, L * L, A, A * A, B, B * B, gm, sg, sg * sg, g, g * g]
    sums = np.array([np.sum(t.astype(np.longdouble)) for t in terms]).astype(np.float64)
    abs_sums = np.array([np.sum(np.abs(t).astype(np.longdouble)) for t in terms]).astype(np.float64)
    lbp_hist = np.bincount(sk_lbp_uniform_8_1(gray)[mask], minlength=10).astype(np.int64)
    gray_hist = np.histogram(g, bins=32, range=(0, 1))[0].astype(np.int64)
    return sums, lbp_hist, gray_hist, abs_sums


def split_score(region_image, mask=None):
    """calculate_split_score (split_score.py:15-142): (overall, colour, texture) in [0, 1]"""
    gray = sk_rgb2gray(region_image)
    if mask is None:
        mask = gray > 0.01
    mask = np.asarray(mask, bool)
    if mask.sum() < 100:
        return 0.0, 0.0, 0.0
    lab = sk_rgb2lab(region_image)
    stds = [np.std(lab[mask, c]) for c in range(3)]
    color_variance = (stds[0] / 100 + stds[1] / 128 + stds[2] / 128) / 3
    gm = 0
    for c in range(3):
        s = sk_sobel(lab[:, :, c])
        gm = gm + np.sqrt(s ** 2 + s ** 2)                   # split_score.py:47-50 takes the same filter for "x" and "y"
    gradient_score = np.mean(gm[mask]) / 3
    color_score = float(np.clip(0.7 * color_variance + 0.3 * gradient_score, 0, 1))
    lbp = sk_lbp_uniform_8_1(gray)[mask]
    hist, _ = np.histogram(lbp, bins=10, range=(0, 10), density=True)
    lbp_score = np.clip(-np.sum(hist * np.log2(hist + 1e-8)) / 3.0, 0, 1)
    grad_score = np.clip(np.var(sk_sobel(gray)[mask]) * 50, 0, 1)
    mg = gray[mask]
    hist, _ = np.histogram(mg, bins=32, range=(0, 1), density=True)
    entropy_score = np.clip(-np.sum(hist * np.log2(hist + 1e-8)) / 5.0, 0, 1)
    std_score = np.clip(np.std(mg) * 2, 0, 1)
    texture_score = float(np.clip((lbp_score + grad_score + entropy_score + std_score) / 4, 0, 1))
    return 0.4 * color_score + 0.6 * texture_score, color_score, texture_score


def normalize_result(score, window_size):
    """split_score.py:143-144"""
    return window_size / (1 + math.exp(-12 * (score - 0.5)))


# --------------------------------------------------------------------------------------
# Masked SLIC (encoder/subregions/slic.py:41-104 enhanced_slic_with_texture), SURVEY 8f-2.  PARITY UNPINNED: the reference
# calls scikit-image's transform.resize and segmentation.slic(mask=...) (absent from the build container); both are restated
# here from their published algorithms on top of scipy.ndimage / scipy.cluster, which scikit-image itself calls.
# --------------------------------------------------------------------------------------
def sk_resize(image, out_hw, order, anti_aliasing):
    """skimage.transform.resize(image, out_hw, order=order, mode='reflect', preserve_range=True, anti_aliasing=...): optional
    Gaussian (sigma = (factor - 1) / 2 per axis) then scipy.ndimage.zoom(grid_mode=True) with numpy-pad 'reflect' =
    ndimage 'mirror' borders, clipped to the input range"""
    from scipy import ndimage as ndi
    img = np.asarray(image)
    out_shape = tuple(out_hw) + img.shape[2:]
    work = img.astype(np.float64) if order > 0 else (img.astype(np.uint8) if img.dtype == bool else img)
    factors = np.divide(img.shape, out_shape)
    if anti_aliasing:
        sigma = np.maximum(0, (factors - 1) / 2)
        work = ndi.gaussian_filter(work, sigma, cval=0, mode="mirror")
    out = ndi.zoom(work, [1 / f for f in factors], order=order, mode="mirror", cval=0, grid_mode=True)
    if order > 0:
        out = np.clip(out, img.min(), img.max())
    return out


def slic_mask_centroids(mask3, n_centroids):
    """skimage.segmentation.slic._get_mask_centroids: RandomState(123) picks n_centroids seed pixels and 100 x as many sample
    pixels inside the mask, five k-means sweeps (scipy.cluster.vq.kmeans2) move the seeds; steps = mean distance, per axis,
    to the nearest other centroid"""
    from scipy.cluster.vq import kmeans2
    from scipy.spatial.distance import pdist, squareform
    coord = np.array(np.nonzero(mask3), dtype=float).T
    rng = np.random.RandomState(123)
    idx_full = np.arange(len(coord), dtype=int)
    idx = np.sort(rng.choice(idx_full, min(n_centroids, len(coord)), replace=False))
    n_dense = int((10 ** 2) * n_centroids)
    idx_dense = np.sort(rng.choice(idx_full, min(n_dense, len(coord)), replace=False))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        centroids, _ = kmeans2(coord[idx_dense], coord[idx], iter=5)
    if len(centroids) > 1:
        dist = squareform(pdist(centroids))
        np.fill_diagonal(dist, np.inf)
        closest = dist.argmin(-1)
        steps = abs(centroids - centroids[closest, :]).mean(0)
    else:
        steps = np.array([1.0, float(mask3.shape[1]), float(mask3.shape[2])])
    return centroids, steps


def slic_sweeps(image, mask, segments, step, max_num_iter, ignore_color):
    """skimage.segmentation._slic._slic_cython for a 2-D image (depth 1, unit spacing, start_label 1), in place on `segments`
    [k][y, x, c0, c1, c2]: every masked pixel takes the centroid with the smallest spatial / step^2 (+ colour) distance among
    those whose window [c - 2 step, c + 2 step] holds it -- the first one on ties --, then the centroids become the means of
    their pixels, sums in raster order.  Returns int64 labels (0 outside the mask or unassigned)."""
    H, W = mask.shape
    K = len(segments)
    yy, xx = np.mgrid[0:H, 0:W]
    inv = 1.0 / (step * step)
    labels = np.zeros((H, W), np.int64)
    for it in range(max_num_iter):
        dist = np.full((H, W), np.finfo(np.float64).max)
        labels = np.zeros((H, W), np.int64)
        change = False
        for k in range(K):
            cy, cx = segments[k, 0], segments[k, 1]
            y0, y1 = int(max(cy - 2 * step, 0)), int(min(cy + 2 * step + 1, H))
            x0, x1 = int(max(cx - 2 * step, 0)), int(min(cx + 2 * step + 1, W))
            if y1 <= y0 or x1 <= x0:
                continue
            sl = (slice(y0, y1), slice(x0, x1))
            d = ((cy - yy[sl]) ** 2 + (cx - xx[sl]) ** 2) * inv        # dz = 0
            if not ignore_color:
                dc = np.zeros_like(d)
                for c in range(3):
                    dc = dc + (image[sl][..., c] - segments[k, 2 + c]) ** 2
                d = d + dc
            upd = mask[sl] & (dist[sl] > d)
            if upd.any():
                change = True
                dist[sl][upd] = d[upd]
                labels[sl][upd] = k + 1
        if not change:
            break
        lab = labels[mask] - 1
        ok = lab >= 0
        lab = lab[ok]
        cnt = np.bincount(lab, minlength=K).astype(np.float64)
        feats = [yy[mask][ok].astype(np.float64), xx[mask][ok].astype(np.float64)] + [image[..., c][mask][ok] for c in range(3)]
        with np.errstate(invalid="ignore", divide="ignore"):
            for f, v in enumerate(feats):
                segments[:, f] = np.bincount(lab, weights=v, minlength=K) / cnt        # bincount adds in raster order
    return labels


def slic_enforce_connectivity(labels, min_size, max_size):
    """skimage.segmentation._slic._enforce_label_connectivity_cython (2-D, start_label 1, 0 = outside the mask): raster scan,
    breadth-first flood of every unvisited component of equal label (4-neighbours, capped at max_size pixels); components
    smaller than min_size take the label of the last already-relabelled neighbour met, the others the next new label"""
    H, W = labels.shape
    out = np.zeros((H, W), np.int64)
    new = 1
    ddy, ddx = (0, 0, 1, -1), (1, -1, 0, 0)
    for y in range(H):
        for x in range(W):
            if out[y, x] >= 1 or labels[y, x] == 0:
                continue
            adjacent = 0
            label = labels[y, x]
            out[y, x] = new
            comp = [(y, x)]
            visited = 0
            while visited < len(comp) < max_size:
                cy, cx = comp[visited]
                for i in range(4):
                    ny, nx = cy + ddy[i], cx + ddx[i]
                    if 0 <= ny < H and 0 <= nx < W:
                        if labels[ny, nx] == label and out[ny, nx] == 0:
                            out[ny, nx] = new
                            comp.append((ny, nx))
                            if len(comp) >= max_size:
                                break
                        elif out[ny, nx] >= 1 and out[ny, nx] != new:
                            adjacent = out[ny, nx]
                visited += 1
            if len(comp) < min_size:
                for cy, cx in comp:
                    out[cy, cx] = adjacent
            else:
                new += 1
    return out


def slic_masked(image_u8, mask, n_segments, compactness=10.0, sigma=1.0, max_num_iter=10):
    """skimage.segmentation.slic(image, n_segments, compactness, sigma=1, channel_axis=2, mask=mask) for a uint8 RGB image"""
    from scipy import ndimage as ndi
    mask = np.asarray(mask, bool)
    lab = sk_rgb2lab(image_u8)
    centroids, steps = slic_mask_centroids(mask[None], n_segments)
    lab = ndi.gaussian_filter(lab[None], [sigma, sigma, sigma, 0], mode="reflect")[0]
    K = len(centroids)
    segments = np.concatenate([centroids[:, 1:], np.zeros((K, 3))], axis=-1)      # (y, x, c0, c1, c2); z = 0 throughout
    step = float(max(steps))
    img = np.ascontiguousarray(lab * (1.0 / compactness))
    slic_sweeps(img, mask, segments, step, max_num_iter, ignore_color=True)
    labels = slic_sweeps(img, mask, segments, step, max_num_iter, ignore_color=False)
    seg_size = mask.sum() / K
    return slic_enforce_connectivity(labels, int(0.5 * seg_size), int(3 * seg_size))


def enhanced_slic(image_u8, mask, n_segments=100, compactness=10):
    """enhanced_slic_with_texture (slic.py:41-104) -> int32 label map (0 = outside the region mask)"""
    scale = round(500 / max(image_u8.shape), 1)
    if scale > 1:
        scale = 1
    h, w = image_u8.shape[:2]
    nh, nw = int(h * scale), int(w * scale)
    small = sk_resize(image_u8, (nh, nw), 1, True).astype(np.uint8)
    small_mask = sk_resize(np.asarray(mask, bool), (nh, nw), 0, False).astype(bool)
    n_seg = math.ceil(n_segments * scale * scale)
    masked = small.copy()
    masked[~small_mask] = 0
    seg_small = slic_masked(masked, small_mask, n_seg, compactness)
    return sk_resize(seg_small, (h, w), 0, False).astype(np.int32)


# --------------------------------------------------------------------------------------
# SURVEY 8f-1, region extraction of the ROI stage (encoder/ROI/roi.py:45-103,285-360,685-718).  extract_roi_nonroi is
# numpy + scipy.ndimage in the reference too (pinned: same library calls).  Connected components: the PARTITION is pinned
# by scipy.ndimage.label; OpenCV's NUMBERING is PARITY UNPINNED (cv2 absent here): restated from its published
# algorithms -- connectedComponentsWithStats(connectivity=8) runs a 2x2-block scan (Grana's BBDT, Bolelli's Spaghetti from
# 4.5.2; also their row-striped parallel forms), provisional labels are created in block-raster order, unions keep the
# smaller one and flattenL renumbers in increasing provisional order => components are numbered by their first 2x2 block
# in block-raster order; connectivity=4 scans pixel by pixel => by first pixel.
# --------------------------------------------------------------------------------------
def cv_connected_components_with_stats(mask, connectivity=8, numbering="opencv"):
    """-> (num_labels, labels int32[H,W], stats int32[num_labels,5] = LEFT, TOP, WIDTH, HEIGHT, AREA); label 0 = background"""
    from scipy import ndimage
    m = np.asarray(mask) != 0
    H, W = m.shape
    st = np.ones((3, 3), bool) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    lab, n = ndimage.label(m, structure=st)                     # numbered by first pixel in raster order
    lab = lab.astype(np.int32)
    ys, xs = np.nonzero(lab)
    l = lab[ys, xs]
    if n and connectivity == 8 and numbering == "opencv":
        big = np.iinfo(np.int64).max
        top = np.full(n + 1, big)
        np.minimum.at(top, l, ys)
        sel = (ys >> 1) == (top[l] >> 1)                        # pixels in the component's first block row
        bx = np.full(n + 1, big)
        np.minimum.at(bx, l[sel], xs[sel] >> 1)
        key = (top[1:] >> 1) * ((W + 1) >> 1) + bx[1:]
        order = np.argsort(key, kind="stable")
        rank = np.zeros(n + 1, np.int32)
        rank[order + 1] = np.arange(1, n + 1, dtype=np.int32)
        lab = rank[lab]
        l = lab[ys, xs]
    stats = np.zeros((n + 1, 5), np.int32)
    by, bx_ = np.nonzero(lab == 0)
    groups = [(0, by, bx_)] if len(by) else []
    if n:
        o = np.argsort(l, kind="stable")
        cuts = np.searchsorted(l[o], np.arange(1, n + 2))
        groups += [(k + 1, ys[o[cuts[k]:cuts[k + 1]]], xs[o[cuts[k]:cuts[k + 1]]]) for k in range(n)]
    for k, gy, gx in groups:
        stats[k] = (gx.min(), gy.min(), gx.max() - gx.min() + 1, gy.max() - gy.min() + 1, len(gy))
    return n + 1, lab, stats


def extract_connected_regions_fast(mask, original_image):
    """roi.py:285-360: one dict per component, in label order; 'coords' in raster order (the reference's come out of an
    unstable argsort over the labels: any order within a region)."""
    num, labels, stats = cv_connected_components_with_stats(np.asarray(mask).astype(np.uint8), 8)
    out = []
    for lab in range(1, num):
        x, y, w, h, area = (int(v) for v in stats[lab])
        single = labels == lab
        coords = np.column_stack(np.nonzero(single))
        full = np.zeros_like(original_image)
        full[single] = original_image[single]
        out.append({"mask": single, "full_image": full, "bbox_image": original_image[y:y + h, x:x + w], "bbox_mask": single[y:y + h, x:x + w],
                    "bbox": (y, x, y + h, x + w), "area": area, "coords": coords, "label": lab})
    return out


def roi_min_region_size(image_rgb):
    """roi.py:47-49 (the SIZE of the array: H * W * 3)"""
    return math.ceil(image_rgb.size / math.pow(10, math.ceil(math.log(image_rgb.size, 10)) - 3))


def extract_regions(image_rgb, roi_mask, nonroi_mask):
    """roi.py:45-103: components of both masks; ROI components below the minimum size move to the END of the non-ROI list"""
    mn = roi_min_region_size(image_rgb)
    roi = extract_connected_regions_fast(roi_mask, image_rgb)
    non = extract_connected_regions_fast(nonroi_mask, image_rgb)
    small = [r for r in roi if r["area"] < mn]
    if small:
        for r in small:
            r["type"] = "nonroi"
        non.extend(small)
        roi = [r for r in roi if r["area"] >= mn]
    return roi, non


def extract_roi_nonroi(original_image, region_map, buffer_size=3):
    """roi.py:685-718"""
    from scipy import ndimage
    roi_core, non_core = region_map == 1, region_map == 0
    buffer_zone = ndimage.binary_dilation(roi_core, iterations=buffer_size) & ndimage.binary_dilation(non_core, iterations=buffer_size)
    roi_mask, non_mask = roi_core | buffer_zone, non_core | buffer_zone
    roi_image, non_image = original_image.copy(), original_image.copy()
    roi_image[~roi_mask] = 0
    non_image[~non_mask] = 0
    return roi_image, non_image, roi_mask, non_mask


# --------------------------------------------------------------------------------------
# SURVEY 8f-1, edge front end of the ROI stage (encoder/ROI/edges.py).  PARITY UNPINNED: OpenCV is absent from the build
# container; cvtColor / Sobel / threshold(OTSU) / Canny / filter2D are restated from OpenCV's published implementation (all
# integer arithmetic but the box filter); everything the reference does in numpy is done in numpy here too.
# --------------------------------------------------------------------------------------
def cv_rgb2gray(rgb_u8):
    """cvtColor(RGB2GRAY) on 8-bit data: fixed point, 14 fractional bits"""
    r, g, b = (rgb_u8[..., i].astype(np.int64) for i in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def cv_sobel3(plane, border):
    """3x3 Sobel (dx, dy) of an integer plane as int64; border 'reflect' = BORDER_REFLECT_101 (cv2.Sobel's default),
    'edge' = BORDER_REPLICATE (what cv2.Canny uses)"""
    p = np.pad(plane.astype(np.int64), 1, mode=border)
    a, b, c = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]
    d, f = p[1:-1, :-2], p[1:-1, 2:]
    g, h, i = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
    return (c + 2 * f + i) - (a + 2 * d + g), (g + 2 * h + i) - (a + 2 * b + c)


def cv_otsu(gray_u8):
    """threshold(THRESH_OTSU)'s threshold value (getThreshVal_Otsu_8u)"""
    h = np.bincount(gray_u8.ravel(), minlength=256).astype(np.float64)
    scale = 1.0 / gray_u8.size
    mu = float((np.arange(256) * h).sum()) * scale
    mu1 = q1 = 0.0
    max_sigma = max_val = 0.0
    eps = float(np.finfo(np.float32).eps)
    for i in range(256):
        p_i = h[i] * scale
        mu1 *= q1
        q1 += p_i
        q2 = 1.0 - q1
        if min(q1, q2) < eps or max(q1, q2) > 1.0 - eps:
            continue
        mu1 = (mu1 + i * p_i) / q1
        mu2 = (mu - q1 * mu1) / q2
        sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
        if sigma > max_sigma:
            max_sigma, max_val = sigma, float(i)
    return max_val


def cv_canny_nms(img_u8):
    """the threshold-independent half of cv2.Canny(img, low, high) (aperture 3, L1 gradient): magnitude |dx| + |dy| of the
    channel with the largest one (first on ties) where the pixel is a local maximum along its gradient direction, else 0"""
    planes = [img_u8] if img_u8.ndim == 2 else [img_u8[..., c] for c in range(img_u8.shape[2])]
    grads = [cv_sobel3(pl, "edge") for pl in planes]
    mags = np.stack([np.abs(gx) + np.abs(gy) for gx, gy in grads])
    best = np.argmax(mags, axis=0)                                   # first maximum
    mag = np.take_along_axis(mags, best[None], 0)[0]
    dx = np.take_along_axis(np.stack([g[0] for g in grads]), best[None], 0)[0]
    dy = np.take_along_axis(np.stack([g[1] for g in grads]), best[None], 0)[0]
    m = np.pad(mag, 1)                                               # magnitudes outside the image: 0
    H, W = mag.shape
    c = m[1:-1, 1:-1]
    ax, ay = np.abs(dx), np.abs(dy) << 15
    tg22x = ax * 13573
    tg67x = tg22x + (ax << 16)
    horiz = ay < tg22x
    vert = ~horiz & (ay > tg67x)
    s = np.where((dx ^ dy) < 0, -1, 1)
    yy, xx = np.mgrid[1:H + 1, 1:W + 1]
    is_max = np.where(horiz, (c > m[1:-1, :-2]) & (c >= m[1:-1, 2:]),
                      np.where(vert, (c > m[:-2, 1:-1]) & (c >= m[2:, 1:-1]), (c > m[yy - 1, xx - s]) & (c > m[yy + 1, xx + s])))
    return np.where(is_max & (mag > 0), mag, 0).astype(np.uint16)


def cv_canny(img_u8, low, high, nm=None):
    """cv2.Canny(img, low, high): hysteresis = the 8-connected components of {nm > low} that hold a pixel with nm > high"""
    from scipy import ndimage
    if nm is None:
        nm = cv_canny_nms(img_u8)
    low, high = math.floor(low), math.floor(high)
    if low > high:
        low, high = high, low
    lab, n = ndimage.label(nm > low, structure=np.ones((3, 3)))
    strong = np.zeros(n + 1, bool)
    strong[np.unique(lab[nm > high])] = True
    strong[0] = False
    return np.where(strong[lab], 255, 0).astype(np.uint8)


def adaptive_canny_thresholds(gray, method="otsu", sensitivity=1.0):
    """edges.py:88-169"""
    def grad_mag():
        gx, gy = cv_sobel3(gray, "reflect")
        return np.sqrt(gx.astype(np.float64) ** 2 + gy.astype(np.float64) ** 2)
    if method == "otsu":
        o = cv_otsu(gray)
        lo, hi = max(10, int(o * 0.5 * sensitivity)), min(255, int(o * 1.5 * sensitivity))
    elif method == "percentile":
        g = grad_mag()
        nz = g[g > 0]
        if len(nz) > 0:
            lp, hp = np.percentile(nz, 70) * sensitivity, np.percentile(nz, 90) * sensitivity
        else:
            lp, hp = 50 * sensitivity, 150 * sensitivity
        lo, hi = max(10, int(lp)), min(255, int(hp))
    elif method == "gradient":
        g = grad_mag()
        mean, std = np.mean(g), np.std(g)
        lo, hi = max(10, int((mean - 0.5 * std) * sensitivity)), min(255, int((mean + 0.5 * std) * sensitivity))
    elif method == "hybrid":
        o = cv_otsu(gray)
        mean = np.mean(grad_mag())
        lo = max(10, int((o * 0.5 + mean * 0.5) * sensitivity))
        hi = min(255, int((o * 1.5 + mean * 1.0) * sensitivity))
    else:
        lo, hi = 50, 150
    lo = max(10, min(200, lo))
    hi = max(lo + 10, min(255, hi))
    return lo, hi


def edge_quality(edges, gray):
    """edges.py:73-86: mean size of the 8-connected edge components x standard deviation of the gray values on the edges"""
    from scipy import ndimage
    lab, n = ndimage.label(edges > 0, structure=np.ones((3, 3)))
    sizes = np.bincount(lab.ravel())
    with np.errstate(all="ignore"):
        avg = np.mean(sizes[1:]) if n else float("nan")
    vals = gray[edges > 0]
    contrast = np.std(vals) if len(vals) > 0 else 0
    return avg * contrast


def find_best_edges_by_quality(image_rgb):
    """edges.py:40-71 -> (best_edges, best_low, best_high, best_method)"""
    gray = cv_rgb2gray(image_rgb)
    nm = cv_canny_nms(gray)
    best = (-1, None, None, None, None)
    for method in ("otsu", "percentile", "gradient", "hybrid"):
        for sens in (0.5, 0.7, 1.0, 1.3, 1.5):
            lo, hi = adaptive_canny_thresholds(gray, method, sens)
            edges = cv_canny(gray, lo, hi, nm)
            score = edge_quality(edges, gray)
            if score > best[0]:
                best = (score, edges, lo, hi, method)
    if best[1] is None:
        raise UnboundLocalError("no threshold pair produced an edge (the reference fails on its unset best_low too)")
    return best[1], best[2], best[3], best[4]


def get_edge_map(image_rgb):
    """edges.py:35-38: the winning thresholds applied to the COLOUR image"""
    _, lo, hi, _ = find_best_edges_by_quality(image_rgb)
    return cv_canny(image_rgb, lo, hi)


def get_edge_map_fast(image_rgb):
    """edges.py:200-233 with compute_fast_canny_thresholds('percentile_fast') (edges.py:235-255,292-298)"""
    gray = cv_rgb2gray(image_rgb)
    low = max(10, min(100, int(np.percentile(gray, 25) * 0.7)))
    high = max(50, min(200, int(np.percentile(gray, 75) * 1.3)))
    if high < low * 2:
        high = low * 2
    if high > 255:
        high = 255
    low = max(10, min(100, low))
    high = max(low * 2, min(200, high))
    gx, gy = cv_sobel3(gray, "reflect")
    mag = np.sqrt(gx.astype(np.float64) ** 2 + gy.astype(np.float64) ** 2)
    nz = mag[mag > 0]
    if len(nz) > 0:
        low = int((low + np.percentile(nz, 10)) / 2)
        high = int((high + np.percentile(nz, 90)) / 2)
    return cv_canny(gray, low, high)


def box_counts(binary_map, kernel_size):
    """number of non-zero pixels in the k x k window around every pixel, BORDER_REFLECT_101"""
    nz = np.pad(np.asarray(binary_map) != 0, kernel_size // 2, mode="reflect").astype(np.int64)
    H, W = np.shape(binary_map)
    cnt = np.zeros((H, W), np.int64)
    for dy in range(kernel_size):
        for dx in range(kernel_size):
            cnt += nz[dy:dy + H, dx:dx + W]
    return cnt


def local_density(binary_map, kernel_size=15):
    """edges.py:173-195: filter2D(float32 map, normalised box kernel), BORDER_REFLECT_101.  Kernels up to 11 x 11 run through
    OpenCV's direct filter: a float32 accumulator over the taps in row-major order (restated literally); larger kernels go through
    its DFT path, whose rounding noise (~1e-7) has no closed form: float32(count) * float32(1 / k^2) here."""
    bm = np.asarray(binary_map)
    if bm.max() > 1:
        bm = bm / 255.0
    kernel = np.ones((kernel_size, kernel_size), np.float32)
    kernel /= kernel.sum()
    H, W = bm.shape
    if kernel_size * kernel_size < 130:
        src = np.pad(bm.astype(np.float32), kernel_size // 2, mode="reflect")
        acc = np.zeros((H, W), np.float32)
        for dy in range(kernel_size):
            for dx in range(kernel_size):
                acc = (acc + kernel[dy, dx] * src[dy:dy + H, dx:dx + W]).astype(np.float32)
        return acc
    # DFT path: (window sum of the map's values) * float32(1 / k^2); for a 0 / 255 map the sum of value / 255 is the count
    raw = np.asarray(binary_map)
    pad = np.pad(raw.astype(np.int64), kernel_size // 2, mode="reflect")
    ssum = np.zeros((H, W), np.int64)
    for dy in range(kernel_size):
        for dx in range(kernel_size):
            ssum += pad[dy:dy + H, dx:dx + W]
    vals = ssum / 255.0 if raw.max() > 1 else ssum.astype(np.float64)
    return vals.astype(np.float32) * kernel[0, 0]


def region_mean_density(labels, num, binary_map, kernel_size):
    """per label the mean box density over its pixels, DFT-path kernel sizes: (exact sum of the window counts) * float32(1 / k^2) / area
    (the reference averages the float32 map in float64: the same number up to the last bits)"""
    counts = np.bincount(labels.ravel(), minlength=num)
    if kernel_size * kernel_size < 130:                             # direct-path sizes: the float32 densities themselves, summed exactly
        dens = local_density(binary_map, kernel_size).astype(np.float64)
        sums = np.bincount(labels.ravel(), weights=dens.ravel(), minlength=num)      # (multiples of 2^-30 below 2^23 pixels: exact in float64)
        out = np.zeros(num)
        out[counts > 0] = sums[counts > 0] / counts[counts > 0]
        return out
    term = float((np.ones((kernel_size, kernel_size), np.float32) / np.float32(kernel_size * kernel_size))[0, 0])
    sums = np.bincount(labels.ravel(), weights=box_counts(binary_map, kernel_size).ravel(), minlength=num)
    out = np.zeros(num)
    out[counts > 0] = sums[counts > 0] * term / counts[counts > 0]
    return out


def suggest_automatic_threshold(edge_density_map, edge_map, method="mean"):
    """edges.py:4-32"""
    vals = edge_density_map[edge_map > 0]
    if len(vals) == 0:
        return 0.1
    if method == "median":
        return np.median(vals)
    if method == "percentile":
        return np.percentile(vals, 70)
    return np.mean(vals)


# --------------------------------------------------------------------------------------
# SURVEY 8f-1, clean-up chain of the ROI stage (encoder/ROI/{roi,small_regions,small_gaps,thin_regions2}.py).  PARITY UNPINNED:
# cv2.morphologyEx / dilate / getStructuringElement / distanceTransform / connectedComponentsWithStats / filter2D restated
# (scipy.ndimage for the morphology, literal raster passes for the chamfer distance); the numpy logic follows the reference.
# --------------------------------------------------------------------------------------
def cv_ellipse_half_widths(ksize):
    """getStructuringElement(MORPH_ELLIPSE, (ksize, ksize)): per row the half-width of the set run around the centre column"""
    r = c = ksize // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    out = []
    for i in range(ksize):
        dy = i - r
        dx = int(np.rint(c * math.sqrt((r * r - dy * dy) * inv_r2)))          # saturate_cast<int>: round half to even
        out.append(min(dx, c))
    return out


def _footprint(half_widths):
    k = len(half_widths)
    fp = np.zeros((k, k), bool)
    for i, hw in enumerate(half_widths):
        if hw >= 0:
            fp[i, k // 2 - hw:k // 2 + hw + 1] = True
    return fp


def cv_dilate(mask, half_widths):
    from scipy import ndimage
    return ndimage.binary_dilation(np.asarray(mask) != 0, structure=_footprint(half_widths), border_value=0)


def cv_erode(mask, half_widths):
    from scipy import ndimage
    return ndimage.binary_erosion(np.asarray(mask) != 0, structure=_footprint(half_widths), border_value=1)


def cv_close(mask, half_widths):
    return cv_erode(cv_dilate(mask, half_widths), half_widths)


def cv_dilate_rect(mask, ksize, erode=False):
    """cv2.dilate / cv2.erode by a ksize x ksize rectangle with OpenCV's default anchor (ksize // 2, ksize // 2):
    dst(y, x) = max / min over dy, dx in [-(ksize // 2), ksize - 1 - ksize // 2] of src(y + dy, x + dx); pixels outside the image do not
    take part (border value -inf for dilate, +inf for erode).  Even sizes included: the window reaches one pixel further up / left."""
    m = np.asarray(mask) != 0
    if erode:
        m = ~m
    a, b = ksize // 2, ksize - 1 - ksize // 2
    H, W = m.shape
    pad = np.zeros((H + a + b + 1, W + a + b + 1), np.int64)
    pad[a + 1:a + 1 + H, a + 1:a + 1 + W] = m
    ii = pad.cumsum(0).cumsum(1)                                   # ii[i, j] = sum of pad[:i + 1, :j + 1]; window rows y .. y + a + b of pad[1:]
    cnt = ii[a + b + 1:, a + b + 1:] - ii[:H, a + b + 1:] - ii[a + b + 1:, :W] + ii[:H, :W]
    out = cnt > 0
    return ~out if erode else out


def cv_close_rect(mask, ksize):
    return cv_dilate_rect(cv_dilate_rect(mask, ksize), ksize, erode=True)


def cv_dist_chamfer3(mask):
    """distanceTransform(mask, DIST_L2, 3) in OpenCV's fixed point (a = round(0.955 * 2^16), b = round(1.3693 * 2^16)): the
    two raster passes of distanceTransform_3x3, literally (int64; the float32 result is value / 65536)"""
    m = np.asarray(mask) != 0
    H, W = m.shape
    a, b, big = 62587, 89738, (2 ** 31 - 1) >> 2
    t = np.full((H + 2, W + 2), big, np.int64)
    for y in range(1, H + 1):
        for x in range(1, W + 1):
            if not m[y - 1, x - 1]:
                t[y, x] = 0
            else:
                t[y, x] = min(t[y - 1, x - 1] + b, t[y - 1, x] + a, t[y - 1, x + 1] + b, t[y, x - 1] + a, big * 2)
    for y in range(H, 0, -1):
        for x in range(W, 0, -1):
            v = t[y, x]
            if v > a:
                v = min(v, t[y + 1, x + 1] + b, t[y + 1, x] + a, t[y + 1, x - 1] + b, t[y, x + 1] + a)
            t[y, x] = v
    return np.minimum(t[1:-1, 1:-1], big)


def _density_count_threshold(kernel_size, threshold, dtype):
    """smallest window count whose density (local_density's value for that count) exceeds `threshold` compared in `dtype`"""
    k2 = kernel_size * kernel_size
    term = (np.ones((kernel_size, kernel_size), np.float32) / np.float32(k2))[0, 0]
    if k2 < 130:
        table = np.zeros(k2 + 1, np.float32)
        for m in range(1, k2 + 1):
            table[m] = np.float32(table[m - 1] + term)
    else:
        table = (np.arange(k2 + 1, dtype=np.float32) * term).astype(np.float32)
    thr = dtype(threshold)
    above = np.flatnonzero(table.astype(dtype) > thr)
    return int(above[0]) if len(above) else k2 + 1, table


def identify_thin_regions(binary_image, min_region_size=10, thinness_threshold=0.3):
    """thin_regions2.py:158-242"""
    num, labels, stats = cv_connected_components_with_stats(binary_image, 8)
    if num <= 1:
        return np.zeros(np.shape(binary_image), bool)
    dist = cv_dist_chamfer3(binary_image)
    sums = np.bincount(labels.ravel(), weights=dist.ravel() / 65536.0, minlength=num)
    counts = np.bincount(labels.ravel(), minlength=num)
    avg = np.zeros(num)
    avg[counts > 0] = sums[counts > 0] / counts[counts > 0]
    max_dims = np.maximum(stats[1:, 2], stats[1:, 3])
    norm = np.zeros(num - 1)
    ok = max_dims > 0
    norm[ok] = avg[1:][ok] * 2 / max_dims[ok]
    is_thin = ((1.0 - norm) > thinness_threshold) & (stats[1:, 4] >= min_region_size)
    return np.isin(labels, np.flatnonzero(is_thin) + 1)


def remove_thin_structures(binary_image, density_threshold=0.2, thinness_threshold=0.3, window_size=25, min_region_size=10, connectivity=8):
    """thin_regions2.py:14-99 (the thin-region test runs with ITS OWN defaults there: min_region_size 10, thinness 0.3)"""
    binary_image = np.asarray(binary_image)
    if np.sum(binary_image > 0) == 0:
        return binary_image
    num, labels, _ = cv_connected_components_with_stats(binary_image, connectivity)
    thin = identify_thin_regions(binary_image)
    thin_ids = np.unique(labels[thin])
    dens = region_mean_density(labels, num, binary_image, window_size).astype(np.float32)
    remove = thin_ids[dens[thin_ids] < density_threshold]
    out = binary_image.copy()
    out[np.isin(labels, remove)] = 0
    return out


def _remove_small_density_aware(binary_image, min_size, density_source, window_size, density_threshold):
    """roi.py:1025-1093 with the return the reference's function forgets (it falls off its end after building cleaned_image)"""
    num, labels, stats = cv_connected_components_with_stats(binary_image == 255, 8)
    if num <= 1:
        return binary_image.copy()
    dens = region_mean_density(labels, num, density_source, window_size)
    ids = np.arange(1, num)[(stats[1:, 4] < min_size) & (dens[1:] < density_threshold)]
    out = binary_image.copy()
    out[np.isin(labels, ids)] = 0
    return out


def remove_small_noise_regions(binary_image, min_size=5, density_threshold=0.2, window_size=15):
    """roi.py:925-968"""
    binary_image = np.asarray(binary_image)
    white = _remove_small_density_aware(binary_image, min_size, binary_image, window_size, density_threshold)
    black = _remove_small_density_aware(255 - white, min_size, binary_image, window_size, density_threshold)   # (the ORIGINAL image's density)
    return 255 - black


def connect_by_closing(binary_image, connection_distance, min_region_size=None):
    """small_regions.py:175-194"""
    return np.where(cv_close(binary_image, cv_ellipse_half_widths(connection_distance * 2 + 1)), 255, 0).astype(np.uint8)


def bridge_small_gaps(binary_image, max_gap=3, density_threshold=0.3, local_window=5, regional_window=25):
    """small_gaps.py:221-319: the one-directional kernels reach min(max_gap, local_window) pixels; their filter2D response is
    positive exactly when a set pixel lies on the ray (BORDER_REFLECT_101); the DFT path's rounding noise around 0 is not restated"""
    b = np.asarray(binary_image)
    out = b.copy()
    cand = (b == 0) & (local_density(b, regional_window) > density_threshold)
    if not cand.any():
        return out
    reach = min(max_gap, local_window)
    H, W = b.shape
    src = np.pad(b != 0, reach, mode="reflect")

    def ray(dx, dy):
        acc = np.zeros((H, W), bool)
        for t in range(1, reach + 1):
            acc |= src[reach + dy * t:reach + dy * t + H, reach + dx * t:reach + dx * t + W]
        return acc
    gaps = np.zeros((H, W), bool)
    for (ax, ay), (bx, by) in (((-1, 0), (1, 0)), ((0, -1), (0, 1)), ((-1, -1), (1, 1)), ((-1, 1), (1, -1))):
        gaps |= cand & ray(ax, ay) & ray(bx, by)
    out[gaps] = 255
    return out


def detect_meaningful_borders(binary_image, sensitivity=0.7):
    """roi.py:784-822"""
    b = np.asarray(binary_image)
    if len(np.unique(b[b != 0])) > 1:
        raise ValueError("a two-valued image is expected")
    # the normalised magnitude does not depend on the one non-zero value (the notebook's cell 6 passes 0 / 1 planes): taken at 1
    gx, gy = cv_sobel3((b != 0).astype(np.int64), "reflect")
    mag = np.sqrt(gx.astype(np.float32) ** 2 + gy.astype(np.float32) ** 2)
    if mag.max() > 0:
        mag = mag / mag.max()
    strong = mag > sensitivity * 0.5
    rect3 = [1, 1, 1]
    enhanced = cv_close(strong, rect3)
    return cv_dilate(enhanced, [2] * 5)                             # two 3x3 dilations = one 5x5


def protect_border_regions(binary_image, border_mask, kernel_size=18):
    """roi.py:824-857 (the function's own default kernel is 18 x 18, the pipeline passes 15)"""
    b = np.asarray(binary_image)
    closed = cv_close_rect(b > 0, kernel_size)
    out = b.copy()
    out[(b == 0) & closed & ~np.asarray(border_mask, bool)] = 255
    return out


def fill_closed_regions(binary_image, min_hole_size=10, max_hole_size=1000, connectivity=4):
    """roi.py:881-918"""
    b = np.asarray(binary_image)
    if b.max() <= 1:
        b = (b * 255).astype(np.uint8)
    num, labels, stats = cv_connected_components_with_stats(255 - b, connectivity)
    fill = np.zeros(num, bool)
    fill[1:] = (stats[1:, 4] >= min_hole_size) & (stats[1:, 4] <= max_hole_size)
    return np.where(fill[labels], 255, b).astype(np.uint8) | b


def remove_small_regions(binary_image, min_size=10, remove_thin_lines=False, kernel_size=3):
    """small_regions.py:4-21 (a 3x3 closing whatever kernel_size says, then the components of at least min_size pixels)"""
    closed = cv_close(binary_image, [1, 1, 1])
    num, labels, stats = cv_connected_components_with_stats(closed, 8)
    keep = np.zeros(num, bool)
    keep[1:] = stats[1:, 4] >= min_size
    return np.where(keep[labels], 255, 0).astype(np.uint8)


def directional_region_unification(binary_image, border_sensitivity=0.3, min_region_size=30, max_gap_to_bridge=50):
    """roi.py:720-782 (its own parameters are ignored there in favour of fixed ones)"""
    b = np.asarray(binary_image)
    if b.max() <= 1:
        b = (b * 255).astype(np.uint8)
    border = detect_meaningful_borders(b, 0.5)
    protected = protect_border_regions(b, border, 15)
    bridged = bridge_small_gaps(protected, 25, 0.2, 15, 25)
    closed = fill_closed_regions(bridged, 10, 10000, 4)
    cleaned = remove_small_regions(closed, 5, True, 30)
    return cleaned, (cleaned > 0).astype(np.uint8)


def process_and_unify_borders(edge_map, edge_density, original_image, density_threshold=0.3, min_region_size=30):
    """roi.py:527-607"""
    borders = edge_map.copy()
    borders[~(edge_density > density_threshold)] = 0
    binary = (borders > 0).astype(np.uint8) * 255
    thinless = remove_thin_structures(binary, 0.10, 0.3, 25, 25)
    noiseless = remove_small_noise_regions(thinless, 75)
    pre = connect_by_closing(noiseless, 5, 25)
    connected = bridge_small_gaps(pre, 100, 0.2, 15, 25)
    unified, region_map = directional_region_unification(connected)
    return (unified, region_map) + extract_roi_nonroi(original_image, region_map)


def get_regions(image_rgb):
    """roi.py:14-40"""
    edge_map = get_edge_map(image_rgb)
    density = local_density(edge_map, 3)
    threshold = suggest_automatic_threshold(density, edge_map, "mean") / 100
    return process_and_unify_borders(edge_map, density, image_rgb, density_threshold=threshold, min_region_size=roi_min_region_size(image_rgb))


# --------------------------------------------------------------------------------------
# EXTENSION (no reference counterpart): block DCT-II + per-region quantisation
# --------------------------------------------------------------------------------------
def dct_quant_blocks(plane, block, qstep_map):
    """Orthonormal 2-D DCT-II on non-overlapping block x block tiles of a float32 plane
    (scipy.fft.dctn(type=2, norm='ortho') semantics), then q = rint(coef / qstep) where
    qstep_map holds one step per tile.  Returns (coef float32[H,W], q int16[H,W])."""
    from scipy.fft import dctn
    H, W = plane.shape
    assert H % block == 0 and W % block == 0
    t = plane.astype(np.float32).reshape(H // block, block, W // block, block).transpose(0, 2, 1, 3)
    c = dctn(t.astype(np.float64), type=2, norm="ortho", axes=(2, 3))
    q = np.rint(c / qstep_map[:, :, None, None]).astype(np.int16)
    c = c.transpose(0, 2, 1, 3).reshape(H, W).astype(np.float32)
    q = q.transpose(0, 2, 1, 3).reshape(H, W)
    return c, q
