"""rhccq_eps_components (csrc/k3_epscomp.hip) in every regime of its two kernels, through Rhccq.eps_components, bit for bit
against the exact reference of tests/eps_cases.py; rhccq_eps_counts / rhccq_eps_border at their tile edges against the oracle.
tests/test_eps_cases_cpu.py proves, without a GPU, which regime each case takes and that no case has a trivial answer.  GPU only."""
import numpy as np
import pytest

import eps_cases as E
from oracle import rhccq_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rh():
    import torch
    from roibasedimagecompression_amd.ops import Rhccq
    assert torch.cuda.is_available()
    return Rhccq(0)


def _check(lab, ncomp, want, what):
    assert lab.dtype == np.int32 and lab.shape == want.shape, what
    assert ncomp == (int(want.max()) + 1 if len(want) else 0), (what, ncomp)
    assert ncomp == (int(lab.max()) + 1 if len(lab) else 0), (what, ncomp)
    bad = np.nonzero(lab != want)[0]
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), lab[bad[:8]].tolist(), want[bad[:8]].tolist())


# ---- the case matrix: a few batched calls of many problems each, as the frame encoder calls the kernel ------------------------------
_BATCHES = {
    "lds": [n for n in E.names() if n.startswith("l_")],
    "global": [n for n in E.names() if n.startswith("g_")],
    "all": E.names()[::-1],                                # both kernels in one launch pair, in the opposite order
}


@pytest.fixture(scope="module")
def matrix(rh):
    out = {}
    for batch, members in _BATCHES.items():
        labs, nc = rh.eps_components([O.pack_rgb(E.case(n)[0]) for n in members], [E.case(n)[1] for n in members])
        for n, l, c in zip(members, labs, nc):
            out[batch, n] = (l.copy(), c)
    return out


@pytest.mark.parametrize("name", E.names())
def test_case_matrix(matrix, name):
    P, eps = E.case(name)
    what = (name,) + E.regime_key(P, eps)
    lab, nc = matrix["lds" if name.startswith("l_") else "global", name]
    _check(lab, nc, E.reference(name), what)
    lab, nc = matrix["all", name]
    _check(lab, nc, E.reference(name), ("all",) + what)


# ---- n = RHCCQ_EPS_LDS_MAX and one more ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", E.LIMIT_EPS)
def test_lds_limit(rh, eps):
    sizes = (E.LDS_MAX, E.LDS_MAX + 1)
    labs, nc = rh.eps_components([O.pack_rgb(E.limit_palette(n)) for n in sizes], [eps] * 2)
    for n, l, c in zip(sizes, labs, nc):
        _check(l, c, E.limit_reference(n, eps), (n, eps) + E.regime_key(E.limit_palette(n), eps))
    # the LDS kernel alone: a call whose largest problem is 10 240 launches nothing else
    labs, nc = rh.eps_components([O.pack_rgb(E.limit_palette(E.LDS_MAX))], [eps])
    _check(labs[0], nc[0], E.limit_reference(E.LDS_MAX, eps), ("alone", eps))


# ---- LDS and global problems and an empty one in a single call ---------------------------------------------------------------------
def test_mixed_batch(rh, matrix):
    members = ["l_wave_exh_int", "g_exh_frac", None, "g_clq_int", "l_point_clq_int"]
    keys = [np.zeros(0, np.uint32) if n is None else O.pack_rgb(E.case(n)[0]) for n in members]
    eps = [12.8 if n is None else E.case(n)[1] for n in members]
    assert len(keys[1]) != len(keys[3]) and min(len(keys[1]), len(keys[3])) > E.LDS_MAX >= max(len(keys[0]), len(keys[4]))
    labs, nc = rh.eps_components(keys, eps)
    assert nc[2] == 0 and len(labs[2]) == 0
    for i, n in enumerate(members):
        if n is None:
            continue
        _check(labs[i], nc[i], E.reference(n), ("mixed", i, n))
        single, c = rh.eps_components([keys[i]], [eps[i]])
        _check(single[0], c[0], E.reference(n), ("single", i, n))
        assert np.array_equal(labs[i], single[0]) and nc[i] == c[0]
    # an empty problem in front, and one at the end
    labs, nc = rh.eps_components([keys[2], keys[3], keys[0], keys[2]], [1.0, eps[3], eps[0], 27.0])
    assert nc[0] == 0 and nc[3] == 0 and len(labs[0]) == 0 and len(labs[3]) == 0
    _check(labs[1], nc[1], E.reference(members[3]), "after an empty problem")
    _check(labs[2], nc[2], E.reference(members[0]), "before an empty problem")


def test_global_scratch_grows_and_is_reused():
    """a context of its own (no earlier call has sized its scratch): a global call, a larger one, the first again"""
    from roibasedimagecompression_amd.ops import Rhccq
    ctx = Rhccq(0)
    small, large = "g_exh_int", "g_clq_frac"
    assert E.LDS_MAX < len(E.case(small)[0]) < len(E.case(large)[0])
    k_small, k_large = O.pack_rgb(E.case(small)[0]), O.pack_rgb(E.case(large)[0])
    first, c1 = ctx.eps_components([k_small], [E.case(small)[1]])
    _check(first[0], c1[0], E.reference(small), "first")
    grown, c2 = ctx.eps_components([k_large, k_small, k_large], [E.case(large)[1], E.case(small)[1], E.case(large)[1]])
    for i, n in enumerate((large, small, large)):
        _check(grown[i], c2[i], E.reference(n), ("grown", i))
    again, c3 = ctx.eps_components([k_small], [E.case(small)[1]])
    _check(again[0], c3[0], E.reference(small), "again")


# ---- small inputs -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(rh):
    names = list(E.SMALL)
    labs, nc = rh.eps_components([O.pack_rgb(E.SMALL[n][0]) for n in names], [E.SMALL[n][1] for n in names])
    return {n: (l.copy(), c) for n, l, c in zip(names, labs, nc)}


@pytest.mark.parametrize("name", list(E.SMALL))
def test_small_inputs(rh, small, name):
    _check(*small[name], E.small_reference(name), name)
    P, eps = E.SMALL[name]
    labs, nc = rh.eps_components([O.pack_rgb(P)], [eps])
    _check(labs[0], nc[0], E.small_reference(name), (name, "alone"))


# ---- min_samples > 1: eps_count_kernel and eps_border_kernel at their tile edges ---------------------------------------------------
@pytest.mark.parametrize("n", E.MS_SIZES)
def test_dbscan_min_samples_at_tile_edges(rh, n):
    keys = O.pack_rgb(E.ms_palette(n))
    for eps in E.MS_EPS:
        for ms in E.MS_MIN_SAMPLES:
            want = E.ms_reference(n, ms, eps)
            got = rh.dbscan_labels(keys, eps, ms)
            bad = np.nonzero(got != want)[0]
            assert got.dtype == np.int32 and len(bad) == 0, (n, eps, ms, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(),
                                                           want[bad[:8]].tolist())
