"""The exact reference of tests/eps_cases.py against the oracle and the sklearn goldens, and the conditions that keep a case of
the eps-components matrix from hiding a wrong kernel: which regime of csrc/k3_epscomp.hip it takes, and that its answer is
neither one component nor all singletons.  No GPU."""
import os

import numpy as np
import pytest

import eps_cases as E
from oracle import rhccq_oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")
ORACLE_MAX = 2500                     # the oracle's propagation loop takes a second or less up to here


def _g3():
    return np.load(os.path.join(G, "g3_dbscan.npz"), allow_pickle=False)


G3_NAMES = ["rand50", "rand500", "rand3000", "lattice", "gapped", "lenna64", "dark", "lenna_final", "adidas_final"]


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in E.names() if len(E.case(n)[0]) <= ORACLE_MAX])
def test_reference_equals_oracle(name):
    P, eps = E.case(name)
    assert np.array_equal(E.reference(name), O.eps_components(P, eps))


@pytest.mark.parametrize("name", list(E.SMALL))
def test_reference_equals_oracle_small(name):
    P, eps = E.SMALL[name]
    lab = E.small_reference(name)
    assert np.array_equal(lab, O.eps_components(P, eps))
    assert np.array_equal(lab, E.reference_labels(P, eps, route="kdtree"))


def test_small_cases_are_what_their_names_say():
    assert E.small_reference("one_point").tolist() == [0]
    assert E.small_reference("two_within").tolist() == [0, 0]
    assert E.small_reference("two_beyond").tolist() == [0, 1]
    P, eps = E.SMALL["two_on_radius"]
    assert E.boundary_pairs(P, eps) in ((1, 0), (0, 1))
    assert E.small_reference("two_on_radius").tolist() == ([0, 0] if O.boundary_pair_is_neighbor(P[0], P[1], eps) else [0, 1])
    for name in ("cell64_exhaustive", "cell65_exhaustive", "cell64_clique", "cell65_clique"):
        P, eps = E.SMALL[name]
        r = E.regime(P, eps)
        assert r["heads"] == 1 and not r["point_mode"] and r["clique"] == name.endswith("clique"), name
    assert max(E.small_reference("cell64_exhaustive")) > 0 and max(E.small_reference("cell65_exhaustive")) > 0
    # one witness pair among 13 x 5
    P, eps = E.SMALL["one_witness"]
    P64 = P.astype(np.int64)
    a, c = np.nonzero(P64[:, 0] <= 8)[0], np.nonzero((P64[:, 0] >= 18) & (P64[:, 0] <= 26))[0]
    assert (len(a), len(c)) == (13, 5) and E.regime(P, eps)["clique"] and E.regime(P, eps)["s"] == 9
    ii, jj = np.repeat(a, 5), np.tile(c, 13)
    assert int(E.is_neighbor(P64, ii, jj, eps).sum()) == 1
    lab = E.small_reference("one_witness")
    assert lab.max() == 1 and len(set(lab[a]) | set(lab[c])) == 1
    P, eps = E.SMALL["duplicates_eps1"]
    assert O.eps_threshold(eps) == (0, 1) and len(np.unique(P, axis=0)) < len(P)


@pytest.mark.parametrize("name", G3_NAMES)
def test_reference_equals_sklearn_golden(name):
    g = _g3()
    assert [str(n) for n in g["names"]] == G3_NAMES
    P = g[f"pal_{name}"]
    for ei, e in enumerate(g["eps"]):
        want = g[f"lab_{name}_{ei}"]
        for route in ("brute", "kdtree") if len(P) <= 1000 else (None,):
            assert np.array_equal(E.reference_labels(P, float(e), route=route), want), (name, float(e), route)


@pytest.mark.parametrize("name", [n for n in E.names() if len(E.case(n)[0]) <= 4000])
def test_candidate_routes_agree(name):
    """the KD-tree proposes a superset of the brute-force candidates, and the accepted pairs are the same"""
    P, eps = E.case(name)
    P64 = P.astype(np.int64)
    bi, bj = E.candidates_brute(P, eps)
    ki, kj = E.candidates_kdtree(P, eps)
    lo, hi = np.minimum(ki, kj), np.maximum(ki, kj)
    n = len(P)
    brute, kd = bi * n + bj, lo * n + hi
    assert len(np.unique(kd)) == len(kd) and np.isin(brute, kd).all()
    ok_b, ok_k = E.is_neighbor(P64, bi, bj, eps), E.is_neighbor(P64, lo, hi, eps)
    assert np.array_equal(np.sort(brute[ok_b]), np.sort(kd[ok_k]))
    assert np.array_equal(E.reference_labels(P, eps, route="brute"), E.reference_labels(P, eps, route="kdtree"))


# ---- the case matrix --------------------------------------------------------------------------------------------------------------
def test_generators_return_unique_shuffled_rows_and_repeat():
    for name, (gen, args) in E.PALETTES.items():
        P = E.palette(name)
        assert P.dtype == np.uint8 and P.ndim == 2 and P.shape[1] == 3
        assert len(np.unique(P, axis=0)) == len(P), name
        assert not np.array_equal(P, np.unique(P, axis=0)), name           # not in sorted order
        assert np.array_equal(P, gen(*args)), name                          # seeded


def test_matrix_reaches_every_regime():
    got = {E.regime_key(*E.case(n)) for n in E.names()}
    assert set(E.LDS_REGIMES) <= got, sorted(set(E.LDS_REGIMES) - got)
    assert set(E.GLOBAL_REGIMES) <= got, sorted(set(E.GLOBAL_REGIMES) - got)
    assert len(E.LDS_REGIMES) == 8 and len(E.GLOBAL_REGIMES) == 4


_NAME_WORDS = {"l": ("lds",), "g": ("global",), "wave": ("wave",), "point": ("point",), "exh": ("exhaustive",), "clq": ("clique",),
               "int": ("integral",), "frac": ("fractional",)}


@pytest.mark.parametrize("name", E.names())
def test_case_takes_the_regime_in_its_name(name):
    P, eps = E.case(name)
    key = E.regime_key(P, eps)
    for word in name.split("_"):
        word = word.rstrip("0123456789")
        if word in _NAME_WORDS:
            assert _NAME_WORDS[word][0] in key, (name, key)
    r = E.regime(P, eps)
    if r["kernel"] == "global":
        assert E.LDS_MAX < len(P) <= 11000
    if name.endswith("below_side9") or name.endswith("below_side16"):
        assert not r["clique"] and E.regime(P, eps + 0.2)["clique"]
    if name.endswith("at_side9") or name.endswith("at_side16"):
        assert r["clique"] and r["s"] == (9 if r["kernel"] == "lds" else 16) and not E.regime(P, eps - 0.2)["clique"]


@pytest.mark.parametrize("name", E.names())
def test_case_is_not_degenerate(name):
    P, eps = E.case(name)
    ncomp, largest, singletons = E.label_stats(E.reference(name))
    assert ncomp >= 2 and largest < 0.9 and singletons < 0.9, (ncomp, largest, singletons)
    if E.regime(P, eps)["integral"]:
        acc, rej = E.boundary_pairs(P, eps)
        assert acc + rej >= 20 and acc >= 5 and rej >= 5, (acc, rej)
        # and the answer hangs on them: d2 <= eps^2 and d2 < eps^2 in integers both give other labels
        for wrong in ("all", "none"):
            assert not np.array_equal(E.reference_labels(P, eps, on_radius=wrong), E.reference(name)), wrong


@pytest.mark.parametrize("name", ["l_lattice3", "l_lattice5", "l_lattice3_small", "l_lattice5_small"])
def test_lattice_cases_are_decided_by_boundary_pairs(name):
    """no pair of a lattice of spacing eps is nearer than eps: every edge of the graph is a boundary pair"""
    P, eps = E.case(name)
    P64 = P.astype(np.int64)
    i, j = E.candidates_kdtree(P, eps)
    thr, boundary = O.eps_threshold(eps)
    d2 = E._d2(P64, i, j)
    assert not (d2 <= thr).any() and (d2 == boundary).sum() >= 1000


@pytest.mark.parametrize("n", [E.LDS_MAX, E.LDS_MAX + 1])
def test_limit_cases(n):
    P = E.limit_palette(n)
    assert len(P) == n and np.array_equal(E.limit_palette(E.LDS_MAX), E.limit_palette(E.LDS_MAX + 1)[:E.LDS_MAX])
    kernel = "lds" if n == E.LDS_MAX else "global"
    want = {5.0: (kernel, "exhaustive", "wave", "integral"), 27.0: (kernel, "clique", "wave", "integral")}
    for eps in E.LIMIT_EPS:
        assert E.regime_key(P, eps) == want[eps]
        ncomp, largest, singletons = E.label_stats(E.limit_reference(n, eps))
        assert ncomp >= 2 and largest < 0.9 and singletons < 0.9


@pytest.mark.parametrize("n", E.MS_SIZES)
def test_min_samples_cases_have_core_border_and_noise(n):
    P = E.ms_palette(n)
    assert len(P) == n and len(np.unique(P, axis=0)) == n
    P64 = P.astype(np.int64)
    for eps in E.MS_EPS:
        i, j = E.candidates_brute(P, eps)
        ok = E.is_neighbor(P64, i, j, eps)
        deg = 1 + np.bincount(np.concatenate([i[ok], j[ok]]), minlength=n)          # itself included
        for ms in E.MS_MIN_SAMPLES:
            lab = E.ms_reference(n, ms, eps)
            core = deg >= ms
            noise = lab < 0
            border = ~core & ~noise
            assert core.sum() >= 5 and noise.sum() >= 5, (n, ms, eps, core.sum(), noise.sum())
            if ms == 2:
                assert border.sum() == 0          # a point with a neighbour counts 2 and is a core point itself
            else:
                assert border.sum() >= 5, (n, ms, eps, border.sum())
            assert not (core & noise).any() and lab.max() >= 1
