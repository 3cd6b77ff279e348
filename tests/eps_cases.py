"""Shared cases of the eps-components regime tests (tests/test_eps_cases_cpu.py, tests/test_gpu_eps_regimes.py): a plain helper
module, not a conftest.

`reference_labels` is an exact statement of rhccq_eps_components that does not share the oracle's min-label propagation loop:
candidate pairs (chunked brute force, or scipy's cKDTree on the integer coordinates), the exact predicate on every candidate
(integer d2 <= thr, or d2 == boundary and the sequential float64 expression of oracle.boundary_pair_is_neighbor, vectorised),
scipy.sparse.csgraph.connected_components, components numbered by their smallest member index.  The KD-tree only proposes
candidates: its radius sqrt(reach2) + 0.5 is larger than every distance the predicate accepts (integer coordinates, so the
float64 distances it compares are off by far less than 0.5), and nothing it returns is accepted without the predicate.

`regime` restates in plain Python which path of csrc/k3_epscomp.hip an input takes (kernel, cell side, clique or exhaustive
search, point or wave mode).  It is a restatement of the source, not a probe of the binary: when the kernel's dispatch
changes, it has to be changed by hand.

Time of `reference_labels` on the x86-64 host this was written on (one thread, seconds, best of two; the KD-tree route is
taken above BRUTE_MAX rows):
    g_exh_int           n = 10 528  eps  5.0   0.03      l_wave_exh_frac  n = 2 433  eps 12.8   brute force 0.28, KD-tree 0.01
    g_exh_frac          n = 10 528  eps 12.8   0.06      limit palette    n = 10 241 eps 27.0   0.16
    g_clq_int           n = 10 632  eps 27.0   0.04      l_lattice5       n = 9 372  eps  5.0   0.01
    g_clq_frac          n = 10 800  eps 27.5   0.21
    g_exh_below_side16  n = 10 800  eps 25.9   0.24
    the densest input of tests/test_gpu_kernels.py that the oracle cannot afford (8 423 rows in a 40-cube, eps 12.8, some
    4 million candidate pairs): 1.15
The oracle's propagation loop, for comparison: 4.4 at n = 2 433 (eps 3), 18 to 38 at n = 3 509 ... 3 596, 44 at n = 6 505,
78 at n = 9 372.  It agreed with `reference_labels` on every LDS case of the matrix when the matrix was written; the CPU
tests repeat that for the cases up to 2 500 rows only.
Every case's palette and reference are computed once per process and shared (do not modify what `case` and `reference` return)."""
import functools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

from oracle import rhccq_oracle as O

LDS_MAX = 10240                       # RHCCQ_EPS_LDS_MAX (include/rhccq.h): above it the global-memory kernel runs
LDS_SIDE_MIN = 9                      # the LDS kernel's grid is at most 30^3 cells: 255 / 30 + 1
GLOBAL_SIDE_MIN = 16                  # the global-memory kernel's grid is at most 16^3 cells
BRUTE_MAX = 3000                      # reference_labels takes the brute-force route up to this many rows


# ---- the exact predicate ----------------------------------------------------------------------------------------------------------
def _d2(P, i, j):
    d = P[i] - P[j]
    return (d * d).sum(axis=1)


def boundary_accepts(P, i, j, eps):
    """oracle.boundary_pair_is_neighbor for the rows P[i], P[j] (index arrays): d = 0; d = d + t * t channel by channel in float64,
    t = a / 255 - b / 255, against (eps / 255)^2"""
    f = np.asarray(P, np.float64) / np.float64(255.0)
    r = np.float64(eps) / np.float64(255.0)
    d = np.zeros(len(i), np.float64)
    for k in range(3):
        t = f[i, k] - f[j, k]
        d = d + t * t
    return d <= r * r


def is_neighbor(P, i, j, eps, on_radius="float64"):
    """the exact predicate on the pairs (P[i], P[j]) of int64 rows.  on_radius = "all" / "none" are the two wrong predicates a
    kernel without the float64 test would compute (d2 <= eps^2 and d2 < eps^2 in integers): the CPU tests use them to show that
    a case's labels depend on the float64 test."""
    thr, boundary = O.eps_threshold(eps)
    d2 = _d2(P, i, j)
    ok = d2 <= thr
    if boundary >= 0 and on_radius != "none":
        b = np.nonzero(d2 == boundary)[0]
        ok[b] = True if on_radius == "all" else boundary_accepts(P, i[b], j[b], eps)
    return ok


def _reach2(eps):
    thr, boundary = O.eps_threshold(eps)
    return boundary if boundary >= 0 else thr


# ---- candidate pairs --------------------------------------------------------------------------------------------------------------
def candidates_brute(P, eps, chunk=512):
    """every i < j with integer d2 <= reach2, by int64 differences in row chunks"""
    P = np.asarray(P, np.int64).reshape(-1, 3)
    reach2 = _reach2(eps)
    ii, jj = [], []
    for s in range(0, len(P), chunk):
        d = P[s:s + chunk, None, :] - P[None, :, :]
        a, b = np.nonzero((d * d).sum(-1) <= reach2)
        keep = a + s < b
        ii.append(a[keep] + s)
        jj.append(b[keep])
    if not ii:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64)


def candidates_kdtree(P, eps):
    """a superset of the pairs i < j within reach: cKDTree.query_pairs with radius sqrt(reach2) + 0.5"""
    P = np.asarray(P, np.int64).reshape(-1, 3)
    if len(P) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pr = cKDTree(P.astype(np.float64)).query_pairs(float(np.sqrt(_reach2(eps))) + 0.5, output_type="ndarray")
    return pr[:, 0].astype(np.int64), pr[:, 1].astype(np.int64)


def _components(n, i, j):
    """labels of the graph on n nodes with edges (i, j), numbered by the smallest member index"""
    g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    _, first = np.unique(lab, return_index=True)         # first[c] = smallest member index of scipy's component c
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[lab].astype(np.int32)


def reference_labels(P, eps, route=None, on_radius="float64"):
    """int32 labels of DBSCAN(eps / 255, min_samples = 1) on P / 255.  route: "brute", "kdtree" or None (by size); on_radius:
    see is_neighbor (anything but the default is a deliberately wrong answer)"""
    P = np.asarray(P, np.int64).reshape(-1, 3)
    n = len(P)
    if n == 0:
        return np.zeros(0, np.int32)
    if route is None:
        route = "brute" if n <= BRUTE_MAX else "kdtree"
    i, j = {"brute": candidates_brute, "kdtree": candidates_kdtree}[route](P, eps)
    ok = is_neighbor(P, i, j, eps, on_radius)
    return _components(n, i[ok], j[ok])


def boundary_pairs(P, eps):
    """(accepted, rejected): the pairs i < j with d2 == boundary by what the float64 test says; (0, 0) for non-integral eps^2"""
    P = np.asarray(P, np.int64).reshape(-1, 3)
    _, boundary = O.eps_threshold(eps)
    if boundary < 0:
        return 0, 0
    i, j = candidates_kdtree(P, eps) if len(P) > BRUTE_MAX else candidates_brute(P, eps)
    b = _d2(P, i, j) == boundary
    acc = boundary_accepts(P, i[b], j[b], eps)
    return int(acc.sum()), int((~acc).sum())


def label_stats(lab):
    """(components, share of the largest component, share of singletons)"""
    size = np.bincount(lab)
    return len(size), float(size.max()) / len(lab), float((size == 1).sum()) / len(lab)


# ---- the kernel's decisions, restated ---------------------------------------------------------------------------------------------
def regime(P, eps):
    """-> dict(kernel "lds" | "global", s, clique, G, heads, point_mode, integral).  s: the clique cell side (largest s with
    3 (s - 1)^2 <= thr) when the grid then fits the kernel's cap, else the cap's smallest side; heads: occupied cells; point_mode
    (one thread per point) exists in the LDS kernel only."""
    P = np.asarray(P, np.int64).reshape(-1, 3)
    n = len(P)
    thr, boundary = O.eps_threshold(eps)
    s = 1
    while 3 * s * s <= thr:
        s += 1
    kernel = "lds" if n <= LDS_MAX else "global"
    s_min = LDS_SIDE_MIN if kernel == "lds" else GLOBAL_SIDE_MIN
    clique = s >= s_min
    if not clique:
        s = s_min
    G = 255 // s + 1
    c = P // s
    heads = len(np.unique((c[:, 0] * G + c[:, 1]) * G + c[:, 2]))
    return dict(kernel=kernel, s=s, clique=clique, G=G, heads=heads, point_mode=kernel == "lds" and n < 3 * heads,
                integral=boundary >= 0)


def regime_key(P, eps):
    """(kernel, "clique" | "exhaustive", "point" | "wave", "integral" | "fractional")"""
    r = regime(P, eps)
    return (r["kernel"], "clique" if r["clique"] else "exhaustive", "point" if r["point_mode"] else "wave",
            "integral" if r["integral"] else "fractional")


# ---- generators: unique uint8 rows in shuffled order ------------------------------------------------------------------------------
def _finish(rng, pts):
    P = np.unique(np.clip(np.rint(pts), 0, 255).astype(np.uint8).reshape(-1, 3), axis=0)
    return P[rng.permutation(len(P))]


def blobs(n, k, sigma, seed=0, lo=0, hi=256):
    """n draws from k Gaussian blobs of deviation sigma with centres uniform in [lo, hi)^3, clipped to the cube"""
    rng = np.random.default_rng([seed, n, k])
    centres = rng.uniform(lo, hi, (k, 3))
    return _finish(rng, centres[rng.integers(0, k, n)] + rng.normal(0.0, sigma, (n, 3)))


def chains(lines, length, step, seed=0):
    """`length` points at distance `step` along each of `lines` random lines: long union-find paths"""
    rng = np.random.default_rng([seed, lines, length])
    start = rng.uniform(0, 256, (lines, 1, 3))
    d = rng.normal(size=(lines, 1, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return _finish(rng, start + d * (step * np.arange(length))[None, :, None])


def lattice(spacing, lo, hi, keep, seed=0):
    """the cubic lattice of the given spacing in [lo, hi]^3, each node kept with probability `keep`: on-axis and Pythagorean
    pairs sit exactly on eps = spacing"""
    rng = np.random.default_rng([seed, spacing, hi])
    a = np.arange(lo, hi + 1, spacing)
    pts = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    return _finish(rng, pts[rng.random(len(pts)) < keep])


def rods(spacing, pitch, motif, keep, axis=0, side=None, seed=0):
    """rods along one channel, `pitch` apart in the other two: every rod is a row of motif x motif bundles `spacing` apart,
    starting at an offset of its own, each point kept with probability `keep`; `side` limits the rods to side x side.  With
    pitch - (motif - 1) > spacing no pair joins two rods, and the only pairs within eps = spacing that join two bundles of a
    rod are the on-axis pairs at exactly eps: with a large eps (clique cells), too, the components hang on the float64 test"""
    rng = np.random.default_rng([seed, spacing, pitch, motif])
    across = np.arange(0, 256 - motif + 1, pitch)[:side]
    pts = []
    for y in across:
        for z in across:
            along = rng.integers(0, spacing) + np.arange(0, 256, spacing)
            g = np.stack(np.meshgrid(along[along < 256], y + np.arange(motif), z + np.arange(motif), indexing="ij"), -1)
            pts.append(g.reshape(-1, 3))
    pts = np.concatenate(pts)
    pts = pts[rng.random(len(pts)) < keep]
    return _finish(rng, np.roll(pts, axis, axis=1))


def dense(hi, n, seed=0):
    """n draws uniform in [0, hi)^3"""
    rng = np.random.default_rng([seed, hi, n])
    return _finish(rng, rng.integers(0, hi, (n, 3)))


# ---- the case matrix --------------------------------------------------------------------------------------------------------------
# palette name -> (generator, arguments); case name -> (palette name, eps).  The case names say which regime the case is there
# for; tests/test_eps_cases_cpu.py asserts that `regime` agrees and that every case can tell a wrong kernel from a right one.
PALETTES = {
    "blobs2500": (blobs, (2500, 40, 3.0)),
    "chains": (chains, (60, 60, 2.8)),
    "lattice3": (lattice, (3, 0, 60, 0.7)),
    "lattice5": (lattice, (5, 0, 120, 0.6)),
    "dense48": (dense, (48, 3000)),
    "sparse": (blobs, (3600, 300, 8.0)),
    "sparse_small": (blobs, (2400, 200, 8.0)),
    "lattice3_small": (lattice, (3, 0, 36, 0.7)),
    "lattice5_small": (lattice, (5, 0, 60, 0.6)),
    "global_a": (blobs, (10900, 220, 2.6)),
    "global_b": (blobs, (11700, 70, 2.9)),
    "rods14": (rods, (14, 17, 3, 0.8, 2, 6)),
    "rods15": (rods, (15, 18, 3, 0.8, 0, 6)),
    "rods15_thin": (rods, (15, 17, 1, 0.7, 1)),
    "rods20": (rods, (20, 23, 3, 0.8, 1, 7)),
    "rods27": (rods, (27, 30, 3, 0.85)),
    "rods26_global": (rods, (26, 30, 4, 0.84, 2)),
    "rods27_global": (rods, (27, 31, 4, 0.86, 1)),
    "limit": (blobs, (12400, 75, 2.9, 1)),
}

CASES = {
    # LDS kernel, one wave per occupied cell
    "l_wave_exh_int": ("blobs2500", 3.0),
    "l_wave_exh_frac": ("blobs2500", 12.8),
    "l_wave_clq_int": ("rods15", 15.0),
    "l_wave_clq_int27": ("rods27", 27.0),
    "l_wave_clq_frac": ("blobs2500", 27.5),
    "l_wave_exh_below_side9": ("blobs2500", 13.8),
    "l_wave_clq_at_side9": ("rods14", 14.0),
    "l_wave_exh_dense": ("dense48", 3.0),
    "l_wave_exh_one": ("dense48", 1.0),
    "l_wave_clq_int20": ("rods20", 20.0),
    # LDS kernel, one thread per point
    "l_point_exh_int": ("chains", 3.0),
    "l_point_exh_frac": ("chains", 12.8),
    "l_point_clq_int": ("rods15_thin", 15.0),
    "l_point_clq_frac": ("sparse", 14.5),
    "l_point_exh_int7": ("sparse", 7.0),
    "l_point_clq_int_sparse": ("sparse", 15.0),
    "l_point_exh_frac_sparse": ("sparse", 12.8),
    # decided by boundary pairs alone
    "l_lattice3": ("lattice3", 3.0),
    "l_lattice5": ("lattice5", 5.0),
    # point mode and lattices small enough for the oracle's propagation loop (tests/test_eps_cases_cpu.py)
    "l_point_exh_int_small": ("sparse_small", 9.0),
    "l_point_clq_int_small": ("sparse_small", 15.0),
    "l_lattice3_small": ("lattice3_small", 3.0),
    "l_lattice5_small": ("lattice5_small", 5.0),
    # global-memory kernel
    "g_exh_int": ("global_a", 5.0),
    "g_exh_frac": ("global_a", 12.8),
    "g_exh_int3": ("global_a", 3.0),
    "g_clq_int": ("rods27_global", 27.0),
    "g_clq_frac": ("global_b", 27.5),
    "g_exh_below_side16": ("global_b", 25.9),
    "g_clq_at_side16": ("rods26_global", 26.0),
}

LDS_REGIMES = [("lds", c, m, i) for c in ("clique", "exhaustive") for m in ("point", "wave") for i in ("integral", "fractional")]
GLOBAL_REGIMES = [("global", c, "wave", i) for c in ("clique", "exhaustive") for i in ("integral", "fractional")]


@functools.lru_cache(maxsize=None)
def palette(name):
    gen, args = PALETTES[name]
    P = gen(*args)
    P.setflags(write=False)
    return P


def names():
    return list(CASES)


def case(name):
    """-> (palette uint8[n, 3], eps)"""
    pal, eps = CASES[name]
    return palette(pal), eps


@functools.lru_cache(maxsize=None)
def reference(name):
    P, eps = case(name)
    lab = reference_labels(P, eps)
    lab.setflags(write=False)
    return lab


# ---- the edge of RHCCQ_EPS_LDS_MAX ------------------------------------------------------------------------------------------------
LIMIT_EPS = (5.0, 27.0)               # exhaustive and clique in both kernels


@functools.lru_cache(maxsize=None)
def limit_palette(n):
    """the first n rows (LDS_MAX or LDS_MAX + 1) of one blobs palette"""
    P = palette("limit")
    assert len(P) > LDS_MAX and n in (LDS_MAX, LDS_MAX + 1)
    return P[:n]


@functools.lru_cache(maxsize=None)
def limit_reference(n, eps):
    lab = reference_labels(limit_palette(n), eps)
    lab.setflags(write=False)
    return lab


# ---- min_samples > 1 --------------------------------------------------------------------------------------------------------------
# eps_count_kernel and eps_border_kernel stage 1024 keys at a time and run 256 threads per block
MS_SIZES = (255, 256, 257, 1023, 1024, 1025, 2049)
MS_MIN_SAMPLES = (2, 5)
MS_EPS = (3.0, 12.8)


@functools.lru_cache(maxsize=None)
def ms_palette(n):
    """exactly n rows: tight blobs (core points) with halos at two scales (border points at either eps of MS_EPS) over a thin
    uniform background (noise)"""
    rng = np.random.default_rng([77, n])
    k = max(3, n // 60)
    centres = rng.uniform(20, 236, (k, 3))
    m = 2 * n
    which = rng.integers(0, k, m)
    sigma = rng.choice([1.6, 5.0, 15.0], m, p=[0.4, 0.35, 0.25])
    pts = np.concatenate([centres[which] + rng.normal(0.0, sigma[:, None], (m, 3)), rng.uniform(0, 256, (n // 8, 3))])
    P = _finish(rng, pts)
    assert len(P) >= n
    P = P[:n]
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def ms_reference(n, min_samples, eps):
    lab = O.dbscan_labels(ms_palette(n), eps, min_samples)
    lab.setflags(write=False)
    return lab


# ---- small inputs -----------------------------------------------------------------------------------------------------------------
def _in_cell(n, seed):
    """n distinct colours inside the one grid cell [9, 17]^3 of side 9"""
    rng = np.random.default_rng([5, n, seed])
    pick = rng.permutation(729)[:n]
    return (np.stack([pick // 81, (pick // 9) % 9, pick % 9], 1) + 9).astype(np.uint8)


def _one_witness():
    """eps 14.5 (clique cells of side 9): 13 colours in the cell x <= 8 and 5 in the cell 18 <= x <= 26, two cells apart, so
    13 x 5 = 65 candidate pairs, one step of 64 and one more; (8, 4, 4) - (18, 4, 4) is the only pair within eps.  A third group
    far away keeps a second component."""
    a = [(x, y, 4) for x in (0, 1, 2) for y in (2, 3, 4, 5)] + [(8, 4, 4)]
    c = [(x, 4, 4) for x in (23, 24, 25, 26)] + [(18, 4, 4)]
    far = [(200, 200, 200), (203, 200, 200)]
    P = np.array(a + c + far, np.uint8)
    return P[np.random.default_rng(9).permutation(len(P))]


def _build_small():
    rng = np.random.default_rng(31)
    dup = rng.integers(0, 6, (400, 3)).astype(np.uint8)     # 216 colours at most: duplicated rows, d2 = 0 <= thr = 0
    out = {
        "one_point": (np.array([[7, 8, 9]], np.uint8), 12.8),
        "two_within": (np.array([[10, 10, 10], [13, 14, 10]], np.uint8), 5.5),
        "two_on_radius": (np.array([[10, 10, 10], [13, 14, 10]], np.uint8), 5.0),
        "two_beyond": (np.array([[10, 10, 10], [13, 14, 11]], np.uint8), 5.0),
        "cell64_exhaustive": (_in_cell(64, 0), 2.0),
        "cell65_exhaustive": (_in_cell(65, 1), 2.0),
        "cell64_clique": (_in_cell(64, 2), 14.5),
        "cell65_clique": (_in_cell(65, 3), 14.5),
        "one_witness": (_one_witness(), 14.5),
        "duplicates_eps1": (dup, 1.0),
    }
    for P, _ in out.values():
        P.setflags(write=False)
    return out


SMALL = _build_small()


@functools.lru_cache(maxsize=None)
def small_reference(name):
    P, eps = SMALL[name]
    lab = reference_labels(P, eps)
    lab.setflags(write=False)
    return lab
