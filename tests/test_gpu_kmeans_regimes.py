"""kmeans_kernel (csrc/k7_kmeans.hip, csrc/kpp_flat.h) in every regime of its storage, k-means++ and Lloyd paths, through
Rhccq.kmeans_split, label for label and iteration for iteration against the oracle on the cases of tests/km_cases.py.
tests/test_km_cases_cpu.py proves, without a GPU, which regime each case takes and pins the oracle to scikit-learn on them.
Every comparison is exact equality of integers.  The oracle runs once per case and process (km_cases.reference).  GPU only."""
import numpy as np
import pytest

import km_cases as K
from oracle import rhccq_oracle as O

pytestmark = pytest.mark.gpu


def _new_context():
    import torch
    from roibasedimagecompression_amd.ops import Rhccq
    assert torch.cuda.is_available()
    return Rhccq(0)


@pytest.fixture(scope="module")
def rh():
    return _new_context()


def _run(ctx, members):
    """one launch over the named cases -> {name: (labels, (n_iter, strict, relocated))}"""
    labs, info = ctx.kmeans_split([O.pack_rgb(K.case(n)[1]) for n in members], [K.case(n)[2] for n in members], return_info=True)
    assert len(labs) == len(members) and info.shape == (len(members), 4)
    return {n: (l.copy(), (int(i[0]), bool(i[1]), int(i[2]))) for n, l, i in zip(members, labs, info)}


def _failure(name, got, where):
    """None, or what differs from the oracle: case, tags, share of equal labels, info (got, wanted)"""
    lab, info = got
    want, oi = K.reference(name)
    winfo = (oi["n_iter"], bool(oi["strict"]), oi["relocated"])
    if lab.dtype == np.int32 and lab.shape == want.shape and np.array_equal(lab, want) and info == winfo:
        return None
    share = float((lab == want).mean()) if lab.shape == want.shape else None
    return dict(where=where, case=name, tags=sorted(K.case(name)[0]), n=len(want), k=K.case(name)[2], equal_labels=share, info=info,
                oracle_info=winfo)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


# ---- all cases in one launch, as the frame encoder batches its splits: LDS and global-scratch problems side by side, label
# offsets that are no multiples of 64 -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(rh):
    offs = np.cumsum([0] + [len(K.case(n)[1]) for n in K.names()])[:-1]
    assert (offs % 64 != 0).any() and max(len(K.case(n)[1]) for n in K.names()) > K.LDS_MAX
    return _run(rh, K.names())


@pytest.fixture(scope="module")
def reversed_batch(rh, batch):
    return _run(rh, K.names()[::-1])


def test_whole_batch_equals_oracle(batch):
    bad = [f for f in (_failure(n, batch[n], "batch") for n in K.names()) if f]
    assert not bad, bad


@pytest.mark.parametrize("tag", K.ALL_TAGS)
def test_regime_equals_oracle(batch, reversed_batch, tag):
    members = K.names_with(tag)
    assert members, tag
    bad = [f for n in members for f in (_failure(n, batch[n], "batch"), _failure(n, reversed_batch[n], "reversed batch")) if f]
    assert not bad, (tag, bad)


def test_reversed_order_gives_the_same_labels(batch, reversed_batch):
    differ = [n for n in K.names() if not _same(batch[n], reversed_batch[n])]
    assert not differ, differ


# ---- lone problems, and the scratch of rhccq_kmeans ---------------------------------------------------------------------------------
def test_lone_problems_and_scratch_growth(batch):
    """a context of its own, so that no earlier call has sized its scratch: first only problems of up to RHCCQ_KM_LDS_MAX points
    (no scratch is handed to the kernel), then a call that needs scratch, then one that needs more, then the smaller one again"""
    ctx = _new_context()
    small = [n for n in K.names() if len(K.case(n)[1]) <= K.LDS_MAX]
    assert "n10240" in small and "n10241" not in small and len(small) >= len(K.names()) - 4
    bad = []

    def check(members, where):
        got = _run(ctx, members)
        for n in members:
            f = _failure(n, got[n], where)
            if f:
                bad.append(f)
            elif not _same(got[n], batch[n]):
                bad.append(dict(where=where, case=n, tags=sorted(K.case(n)[0]), differs_from="batch"))

    check(small, "small problems only")
    for n in K.LONE_CASES:
        if len(K.case(n)[1]) <= K.LDS_MAX:
            check([n], "alone")
    large = [n for n in K.LONE_CASES if len(K.case(n)[1]) > K.LDS_MAX]
    assert large == ["n10241"]
    check(large, "alone: the first call with scratch")
    more = ["empty_pts_global", "n10241", "glob_glob", "n10240"]
    assert max(len(K.case(n)[1]) for n in more) > len(K.case("n10241")[1])                 # more problems, and a longer stride
    check(more, "a larger scratch")
    check(large, "alone: a smaller call on the grown scratch")
    assert not bad, bad
