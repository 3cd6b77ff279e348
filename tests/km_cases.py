"""Shared cases of the KMeans split regime tests (tests/test_km_cases_cpu.py, tests/test_gpu_kmeans_regimes.py): a plain helper
module, not a conftest.  numpy only.

kmeans_kernel (csrc/k7_kmeans.hip, with csrc/kpp_flat.h) is one 1024-thread workgroup per problem with separate code paths by
input size; every case here is (name, regime tags, points uint8[n, 3], k) and the tags say which paths it is there for:

    pts_lds / pts_global      points and labels in LDS (n <= LDS_MAX) or in the context's global scratch
    cent_lds / cent_global    centres and member sums in LDS (k <= CENT_LDS) or in the caller's work buffer
    kpp_flat4                 k-means++ by kpp_flat<16, 4>, four working waves (n <= FLAT4_MAX)
    kpp_flat16                k-means++ by kpp_flat<kKmFlatS, 16> (FLAT4_MAX < n <= FLAT16_MAX)
    kpp_scan                  k-means++ by the block-scan loop (n > FLAT16_MAX)
    T2 ... T9                 trials per pick, 2 + int(ln k)
    stop_tol / stop_strict    Lloyd ends on the centre-shift tolerance (the final re-assignment pass runs) or on unchanged labels
    empty                     an E-step leaves clusters empty: the mark, the farthest-point search, its dist.max() == 0 exit and the
                              copy of the heaviest centre run; clusters are still empty at the end and nothing was relocated
    tie                       the two largest member counts are equal when the heaviest centre is copied: the first arg-max decides
    pot_max                   the k-means++ potential reaches n / 2 x 195 075, what the 32-bit sums of kpp_flat are sized for
    degenerate                n = 1, n = k = 2, k = 1
    n4096 n4097 n10240 n10241 k1024 k1025        the two sides of every limit

tests/test_km_cases_cpu.py asserts, with the oracle, that every case is what its tags say, and reads the limits below back from
the sources, so that a moved threshold cannot silently empty a regime.

Not covered, on purpose: a relocation that actually moves a point (`relocated > 0`, which needs an empty cluster while
`dist.max() > 0`).  The oracle was searched for such an input and none was found: 200 000 random inputs of 6 to 59 points
(uniform, nearly one-dimensional, with duplicates) and 1 200 clustered inputs of up to 700 points at k = 0.2 n, 0.5 n and 0.8 n.
With exact means in three dimensions, greedy k-means++ and the fixed seed, the only empty clusters met were those whose centre
duplicates an earlier one (k above the number of distinct colours), and then every point sits on its own centre.  Nobody needs to
repeat that search; a case that turns up by accident is welcome.

Every case and its oracle result are computed once per process and shared (do not modify what `case` and `reference` return).
Oracle time on the x86-64 host this was written on: 3.9 s for glob_glob, about 2 s for each of k1024 / k1025, 0.6 s and less
for every other case, some 12 s for all of them."""
import functools
import math

import numpy as np

# ---- the limits, and where they come from ------------------------------------------------------------------------------------------
LDS_MAX = 10240                       # RHCCQ_KM_LDS_MAX (include/rhccq.h): `if (n <= RHCCQ_KM_LDS_MAX) { P = s_keys; ...`
CENT_LDS = 1024                       # kKmCentLds (k7_kmeans.hip): `if (k <= kKmCentLds) { C = s_cent; S = s_sum; }`
FLAT4_MAX = 16 * 64 * 4               # k7_kmeans.hip: `if (n <= 16 * 64 * 4)` -> kpp_flat<16, 4>
FLAT_S = 10                           # kKmFlatS (k7_kmeans.hip)
THREADS = 1024                        # kKmThreads (k7_kmeans.hip)
FLAT16_MAX = FLAT_S * THREADS         # k7_kmeans.hip: `else if (n <= kKmFlatS * kKmThreads)` -> kpp_flat<kKmFlatS, kKmWaves>
D2_MAX = 3 * 255 * 255                # 195 075: the largest squared distance of two colours


def trials(k):
    """n_local_trials of sklearn's greedy k-means++"""
    return 2 + int(math.log(k))


def regime_tags(n, k):
    """the storage, k-means++ and trial-count tags that follow from n and k alone: a restatement of the kernel's dispatch"""
    return {"pts_lds" if n <= LDS_MAX else "pts_global", "cent_lds" if k <= CENT_LDS else "cent_global",
            "kpp_flat4" if n <= FLAT4_MAX else "kpp_flat16" if n <= FLAT16_MAX else "kpp_scan", f"T{trials(k)}"}


# ---- generators --------------------------------------------------------------------------------------------------------------------
def cube(side, n, seed):
    """n different colours of [0, side)^3 in drawn (not sorted) order"""
    rng = np.random.default_rng(seed)
    pick = rng.choice(side ** 3, n, replace=False)
    return np.stack([pick // (side * side), (pick // side) % side, pick % side], 1).astype(np.uint8)


def repeats(n, distinct, seed):
    """`distinct` different colours of the full cube followed by n - distinct random repeats of them, permuted"""
    rng = np.random.default_rng(seed)
    base = cube(256, distinct, [seed, 1])
    P = np.concatenate([base, base[rng.integers(0, distinct, n - distinct)]])
    return P[rng.permutation(n)]


def two_valued(n):
    """black and white in turn"""
    P = np.zeros((n, 3), np.uint8)
    P[1::2] = 255
    return P


def first_index(n):
    """the first centre of KMeans(random_state=42) on n points: RandomState(42).choice(n, p=ones / n)"""
    cdf = np.cumsum(np.full(n, 1.0) / np.float64(n))
    cdf /= cdf[-1]
    return min(int(np.searchsorted(cdf, np.random.RandomState(42).random_sample(), side="right")), n - 1)


def pairs(distinct, seed):
    """every one of `distinct` colours twice, permuted, with point 0 of the colour of the first centre.  Every filled cluster then
    has two members; with k > distinct the further centres duplicate point 0, that is cluster 0, the first arg-max of the counts:
    copying the heaviest centre moves nothing and the first iteration ends on the tolerance.  Any other of the tied clusters
    moves the empty centres and costs a second iteration."""
    rng = np.random.default_rng(seed)
    base = cube(256, distinct, [seed, 1])
    P = np.concatenate([base, base])[rng.permutation(2 * distinct)]
    f = first_index(len(P))
    twin = [i for i in np.nonzero((P == P[f]).all(1))[0] if i != f][0]
    if f != 0:
        P[[0, twin]] = P[[twin, 0]]
    return P


@functools.lru_cache(maxsize=None)
def _boundary_set():
    return cube(64, LDS_MAX + 1, 0)


@functools.lru_cache(maxsize=None)
def _sweep_set():
    return cube(256, 4500, 0)


@functools.lru_cache(maxsize=None)
def _centre_set():
    return cube(256, 7000, 0)


SWEEP_K = (7, 8, 20, 21, 54, 55, 148, 149, 403, 404)     # every pair straddles a step of 2 + int(ln k): T = 3|4, 4|5, 5|6, 6|7, 7|8
SWEEP_STOP = {7: "stop_tol", 8: "stop_tol", 20: "stop_tol", 21: "stop_tol", 54: "stop_tol", 55: "stop_strict", 148: "stop_strict",
              149: "stop_strict", 403: "stop_strict", 404: "stop_strict"}


def _build():
    out = []

    def add(name, tags, P, k):
        P = np.ascontiguousarray(P, np.uint8)
        P.setflags(write=False)
        out.append((name, frozenset(set(tags) | regime_tags(len(P), k)), P, k))

    # point-count limits: prefixes of one set of 64-cube colours, k = 9; all four stop on the tolerance rule.  n = 10241 gives
    # per = 11 in the block-scan path, with trailing threads that own no sample
    for n in (FLAT4_MAX, FLAT4_MAX + 1, LDS_MAX, LDS_MAX + 1):
        add(f"n{n}", {f"n{n}", "stop_tol"}, _boundary_set()[:n], 9)
    # centre-count limit (and kpp_flat<10, 16> with T = 8)
    for k in (CENT_LDS, CENT_LDS + 1):
        add(f"k{k}", {f"k{k}", "stop_strict"}, _centre_set(), k)
    # global points with global centres
    add("glob_glob", {"stop_strict"}, cube(48, 10300, 0), 1100)
    # trial counts 3 ... 8 on one set of 4500 colours
    for k in SWEEP_K:
        add(f"sweep_k{k}", {SWEEP_STOP[k]}, _sweep_set(), k)
    # more centres than distinct colours, one case per storage regime
    add("empty_small", {"empty", "stop_strict"}, repeats(50, 10, 1), 20)
    add("empty_flat16", {"empty", "stop_strict"}, repeats(4097, 40, 2), 64)
    add("empty_cent_global", {"empty", "stop_strict"}, repeats(2600, 1100, 3), 1300)
    add("empty_pts_global", {"empty", "stop_strict"}, repeats(10300, 9, 4), 12)
    # the largest potential; with k = 3 one cluster stays empty beside two of equal count.  The third centre duplicates the colour of
    # point 0 (black).  At n = 10240 cluster 0 is white, so the copy of the heaviest centre (cluster 0, the first arg-max) moves the
    # empty centre across the cube, the shift is far above the tolerance and a second iteration ends strictly; at n = 4096 cluster 0
    # is black, the copy moves nothing and the first iteration ends on the tolerance.  With the other of the two tied clusters the
    # two would swap their iteration counts and stop rules.
    add("bw10240_k2", {"pot_max", "stop_tol"}, two_valued(10240), 2)
    add("bw10240_k3", {"pot_max", "empty", "tie", "stop_strict"}, two_valued(10240), 3)
    add("bw4096_k3", {"pot_max", "empty", "tie", "stop_tol"}, two_valued(4096), 3)
    # a tie among more than 1024 clusters, where a thread of the heaviest-cluster search holds two of them (j and j + 1024): all
    # 1100 filled clusters have two members, cluster 0 wins, and threads 0 ... 75 each hold a second filled cluster
    add("tie_cent_global", {"empty", "tie", "stop_tol"}, pairs(1100, 5), 1300)
    # degenerate
    add("one_point", {"degenerate", "stop_tol"}, np.array([[7, 8, 9]], np.uint8), 1)
    add("two_points_k2", {"degenerate", "stop_tol"}, np.array([[10, 20, 30], [200, 100, 0]], np.uint8), 2)
    add("sweep_k1", {"degenerate", "stop_strict"}, _sweep_set(), 1)
    return out


CASES = _build()
_BY_NAME = {c[0]: c for c in CASES}
assert len(_BY_NAME) == len(CASES)

ALL_TAGS = ("pts_lds", "pts_global", "cent_lds", "cent_global", "kpp_flat4", "kpp_flat16", "kpp_scan", "T2", "T3", "T4", "T5", "T6", "T7", "T8",
            "T9", "stop_tol", "stop_strict", "empty", "tie", "pot_max", "degenerate", "n4096", "n4097", "n10240", "n10241", "k1024", "k1025")

# cases whose oracle labels equal scikit-learn's KMeans(k, random_state=42, n_init=1).fit_predict label for label.  The cases with
# more than 1024 centres are left out: scikit-learn's BLAS arithmetic is not KM64.  With that many picks two candidates of a pick
# sooner or later have the same exact potential (pick 856 of glob_glob: 64 513 twice among its nine); KM64 takes the first of them,
# scikit-learn whichever its float64 distances round lower, and every later pick and label differs from there.
SKLEARN_CASES = tuple(c[0] for c in CASES if c[0] not in ("glob_glob", "empty_cent_global", "tie_cent_global"))

# problems that are also run alone in a launch of their own (tests/test_gpu_kmeans_regimes.py)
LONE_CASES = ("n10240", "n10241", "k1025", "empty_cent_global")


def names():
    return [c[0] for c in CASES]


def names_with(tag):
    return [c[0] for c in CASES if tag in c[1]]


def case(name):
    """-> (tags frozenset, points uint8[n, 3], k)"""
    return _BY_NAME[name][1:]


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (labels int32[n], info dict) of oracle.rhccq_oracle.kmeans_labels"""
    from oracle import rhccq_oracle as O
    _, P, k = case(name)
    lab, info = O.kmeans_labels(P, k, return_info=True)
    lab.setflags(write=False)
    return lab, info
