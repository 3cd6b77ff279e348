"""Every entry point of csrc/k1_unique.hip, and K2 (rhccq_cluster_sums / rhccq_cluster_means), against the exact per-job reference of
tests/job_cases.py: through ops.Rhccq as FrameEncoder.prepare drives them, every intermediate compared with np.array_equal.
tests/test_job_cases_cpu.py proves, without a GPU, that the reference equals the oracle and that the matrix reaches the paths named
here (statistics table overflow, W < 4, H*W mod 4 != 0, unaligned class planes, grid-stride loops, ...).  GPU only."""
from types import SimpleNamespace

import numpy as np
import pytest

import job_cases as J

pytestmark = pytest.mark.gpu

E_ARG = -1
BITMAP = J.names("bitmap")
OUT_TYPES = (("uint8", 255), ("int16", 32767), ("int32", J.INT_MAX))


@pytest.fixture(scope="module")
def rh():
    import torch
    from roibasedimagecompression_amd.ops import Rhccq
    assert torch.cuda.is_available()
    return Rhccq(0)


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got.reshape(-1)[bad[:8]].tolist(), want.reshape(-1)[bad[:8]].tolist())


_DEV = {}
_STATE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_state():
    """the cases and their bitmap / (word, prefix) tables stay on the device while this module runs, not after it"""
    yield
    _DEV.clear()
    _STATE.clear()
    import torch
    torch.cuda.empty_cache()


def _dev(rh, name):
    """the case on the device (uploaded once)"""
    if name not in _DEV:
        cs = J.case(name)
        _DEV[name] = SimpleNamespace(rgb=rh.dev(cs.img.copy()), labels=[None if l is None else rh.dev(l.copy()) for l in cs.labels],
                                     job_base=cs.job_base)      # (copies: the case's arrays are read-only)
    return _DEV[name]


def _host(t):
    return t.cpu().numpy()


def _sparse(bitmaps):
    """(job, word, value) of every non-zero bitmap word, in (job, word) order"""
    import torch
    nz = torch.nonzero(bitmaps)
    return _host(nz[:, 0]), _host(nz[:, 1]), _host(bitmaps[nz[:, 0], nz[:, 1]]).view(np.uint32)


def _check_bitmaps(bitmaps, sets, what):
    """word for word on the words the reference sets, zero elsewhere"""
    jobs, words, vals = [], [], []
    for j, keys in enumerate(sets):
        w, v = J.bitmap_words(keys)
        jobs.append(np.full(len(w), j, np.int64))
        words.append(w)
        vals.append(v)
    gj, gw, gv = _sparse(bitmaps)
    _eq(gj, np.concatenate(jobs), (what, "job of set words"))
    _eq(gw, np.concatenate(words), (what, "set words"))
    _eq(gv, np.concatenate(vals), (what, "word values"))


# ---- scans -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BITMAP)
def test_scans(rh, monkeypatch, name):
    cs, ref, d = J.case(name), J.reference(name), _dev(rh, name)
    for black in (0, 1):
        # byte flags + pack; for black = 0 the black bits of rhccq_job_set_black are there first and must survive the pack's OR
        bitmaps, stats = rh.new_job_state(cs.n_jobs)
        pre = ref.black_jobs if black == 0 else []
        rh.job_set_black(bitmaps, pre)
        rh.job_scan(d.rgb, d.labels, d.job_base, bitmaps, stats, black_is_colour=black)
        _eq(_host(stats), ref.stats, (name, black, "bytes: stats"))
        _check_bitmaps(bitmaps, J.with_black(ref.sets[black], pre), (name, black, "bytes"))
        # bit atomics
        with monkeypatch.context() as mp:
            mp.setattr(rh, "BYTEMAP_MAX_JOBS", 0)
            bitmaps, stats = rh.new_job_state(cs.n_jobs)
            rh.job_scan(d.rgb, d.labels, d.job_base, bitmaps, stats, black_is_colour=black)
        _eq(_host(stats), ref.stats, (name, black, "atomics: stats"))
        _check_bitmaps(bitmaps, ref.sets[black], (name, black, "atomics"))
    _eq(_host(rh.job_stats(d.rgb, d.labels, d.job_base, cs.n_jobs)), ref.stats, (name, "job_stats"))


@pytest.mark.parametrize("name", J.names("stats"))
def test_statistics_table_full_and_overflowing(rh, monkeypatch, name):
    """80 jobs inside each block's pixels: 16 of them miss the 64 LDS slots and go to global atomics; 64: every slot used"""
    cs, ref, d = J.case(name), J.reference(name), _dev(rh, name)
    assert cs.n_jobs >= 64
    _eq(_host(rh.job_stats(d.rgb, d.labels, d.job_base, cs.n_jobs)), ref.stats, (name, "job_stats"))
    monkeypatch.setattr(rh, "BYTEMAP_MAX_JOBS", 0)
    for black in (0, 1):
        bitmaps, stats = rh.new_job_state(cs.n_jobs)
        rh.job_scan(d.rgb, d.labels, d.job_base, bitmaps, stats, black_is_colour=black)
        _eq(_host(stats), ref.stats, (name, black, "atomics: stats"))
        _check_bitmaps(bitmaps, ref.sets[black], (name, black, "atomics"))


# ---- the state FrameEncoder.prepare builds, once per case ----------------------------------------------------------------------------
def _state(rh, name, kind):
    """kind "fix": scan without black, black set where the crop shows background or the job is all black, fix_key; "plain": black is a
    colour, no fix"""
    if (name, kind) not in _STATE:
        cs, ref, d = J.case(name), J.reference(name), _dev(rh, name)
        bitmaps, stats = rh.new_job_state(cs.n_jobs)
        rh.job_scan(d.rgb, d.labels, d.job_base, bitmaps, stats, black_is_colour=(kind == "plain"))
        if kind == "fix":
            rh.job_set_black(bitmaps, ref.black_jobs)
        chunk, counts = rh.bitmap_count(bitmaps)
        pals = ref.pal_fix if kind == "fix" else ref.pal_plain
        off = J.pal_offsets(pals)
        d_off = rh.dev(off[:-1].copy())
        prefix, keys = rh.bitmap_emit(bitmaps, chunk, d_off, int(off[-1]))
        _STATE[name, kind] = SimpleNamespace(bitmaps=bitmaps, chunk=chunk, counts=counts, off=off, d_off=d_off, prefix=prefix, keys=keys, pals=pals,
                                             total=int(off[-1]), rank=ref.rank_fix if kind == "fix" else ref.rank_plain,
                                             fix_key=rh.dev(ref.fix_key.view(np.int32)) if kind == "fix" else None,
                                             fk=ref.fix_key if kind == "fix" else None)
    return _STATE[name, kind]


@pytest.mark.parametrize("kind", ("fix", "plain"))
@pytest.mark.parametrize("name", BITMAP)
def test_bitmap_passes(rh, name, kind):
    cs, S = J.case(name), _state(rh, name, kind)
    _eq(_host(S.counts), [len(p) for p in S.pals], (name, kind, "counts"))
    _eq(_host(S.chunk).view(np.uint32), np.stack([J.chunk_sums(p) for p in S.pals]), (name, kind, "chunk sums"))
    _eq(_host(S.keys[:S.total]).view(np.uint32), np.concatenate(S.pals), (name, kind, "keys_out"))
    for j, keys in enumerate(S.pals):
        for ch in np.unique(keys >> 15):          # (chunks without a colour are never written)
            got = _host(S.prefix[j, int(ch) * J.CHUNK_WORDS:(int(ch) + 1) * J.CHUNK_WORDS]).view(np.uint32)
            _eq(got, J.chunk_pairs(keys, int(ch)), (name, kind, j, int(ch), "(word, prefix) pairs"))


@pytest.mark.parametrize("name", BITMAP)
def test_blackfix(rh, name):
    import torch
    cs, ref, d = J.case(name), J.reference(name), _dev(rh, name)
    best = torch.full((cs.n_jobs,), -1, dtype=torch.int64, device=rh.device)
    rh.job_blackfix(d.rgb, d.labels, d.job_base, rh.dev(ref.d.needs_fix.astype(np.uint8)), best)
    _eq(_host(best).view(np.uint64), ref.best, (name, "best"))
    # no job flagged: nothing is written
    best = torch.full((cs.n_jobs,), -1, dtype=torch.int64, device=rh.device)
    rh.job_blackfix(d.rgb, d.labels, d.job_base, rh.zeros((cs.n_jobs,), torch.uint8), best)
    assert np.all(_host(best) == -1), name


def _first_pos(rh, n):
    import torch
    return torch.full((max(n, 1),), J.INT_MAX, dtype=torch.int32, device=rh.device)


@pytest.mark.parametrize("kind", ("fix", "plain"))
@pytest.mark.parametrize("name", BITMAP)
def test_job_index(rh, name, kind):
    cs, d, S = J.case(name), _dev(rh, name), _state(rh, name, kind)
    fpl = J.fp_lut(name, S.total)
    # idx_out alone
    idx = rh.job_index(d.rgb, d.labels, d.job_base, S.bitmaps, S.prefix, S.d_off, fix_key=S.fix_key)
    _eq(_host(idx), S.rank, (name, kind, "idx_out"))
    # first_pos alone, without and with fp_lut
    for lut in (None, fpl):
        ent, want_fp = J.entries(cs, S.rank, S.off, lut)
        fp = _first_pos(rh, len(want_fp))
        assert rh.job_index(d.rgb, d.labels, d.job_base, S.bitmaps, S.prefix, S.d_off, fix_key=S.fix_key, want_idx=False, first_pos=fp,
                            fp_lut=None if lut is None else rh.dev(lut)) is None
        _eq(_host(fp), want_fp, (name, kind, lut is not None, "first_pos"))
    # both
    fp = _first_pos(rh, len(want_fp))
    idx = rh.job_index(d.rgb, d.labels, d.job_base, S.bitmaps, S.prefix, S.d_off, fix_key=S.fix_key, first_pos=fp, fp_lut=rh.dev(fpl))
    _eq(_host(idx), S.rank, (name, kind, "idx_out beside first_pos"))
    _eq(_host(fp), want_fp, (name, kind, "first_pos beside idx_out"))


@pytest.mark.parametrize("name", BITMAP)
def test_job_index_entries(rh, name):
    import torch
    cs, d, S = J.case(name), _dev(rh, name), _state(rh, name, "fix")
    n_class, n_px = len(cs.labels), cs.H * cs.W
    for lut in (J.fp_lut(name, S.total), None):
        want_ent, want_fp = J.entries(cs, S.rank, S.off, lut)
        d_lut = None if lut is None else rh.dev(lut)
        # one call per class into its slice of one buffer (class c starts at c * H * W elements), as the pipelined encoder does
        buf = torch.full((n_class, n_px), -7, dtype=torch.int32, device=rh.device)
        fp = _first_pos(rh, len(want_fp))
        for c in range(n_class):
            rh.job_index_entries(d.rgb, [d.labels[c]], [d.job_base[c]], S.bitmaps, S.prefix, S.d_off, S.fix_key, fp, d_lut, buf[c])
        _eq(_host(buf), want_ent, (name, lut is not None, "entries, class by class"))
        _eq(_host(fp), want_fp, (name, lut is not None, "first_pos, class by class"))
        # all classes in one call
        buf = torch.full((n_class, n_px), -7, dtype=torch.int32, device=rh.device)
        fp = _first_pos(rh, len(want_fp))
        rh.job_index_entries(d.rgb, d.labels, d.job_base, S.bitmaps, S.prefix, S.d_off, S.fix_key, fp, d_lut, buf)
        _eq(_host(buf), want_ent, (name, lut is not None, "entries, one call"))
        _eq(_host(fp), want_fp, (name, lut is not None, "first_pos, one call"))


def _remap_variants(name):
    """(dtype, top, with_lut2, default_index): all twelve, three of them on the large case"""
    out = []
    for dt, top in OUT_TYPES:
        for with_lut2 in (False, True):
            for default in (0, top - 1):
                out.append((dt, top, with_lut2, default))
    return out if name != J.BIG else [out[1], out[6], out[8]]


def _as_int(t):
    a = _host(t)
    return a.astype(np.int64).reshape(-1)


@pytest.mark.parametrize("name", BITMAP)
def test_frame_remap(rh, name):
    import torch
    cs, d, S = J.case(name), _dev(rh, name), _state(rh, name, "fix")
    for dt, top, with_lut2, default in _remap_variants(name):
        lut, lut2 = J.luts(name, S.total, top, with_lut2)
        want = J.index_map(cs, S.rank, S.off, lut, lut2, default)
        got = rh.frame_remap(d.rgb, d.labels, d.job_base, S.bitmaps, S.prefix, S.d_off, S.fix_key, rh.dev(lut), default, getattr(torch, dt),
                             lut2=None if lut2 is None else rh.dev(lut2))
        assert got.shape == (cs.H, cs.W)
        _eq(_as_int(got), want, (name, dt, with_lut2, default, "index map"))


@pytest.mark.parametrize("name", BITMAP)
def test_frame_remap_entries(rh, name):
    import torch
    cs, d, S = J.case(name), _dev(rh, name), _state(rh, name, "fix")
    fpl = J.fp_lut(name, S.total)
    ent, fp = J.entries(cs, S.rank, S.off, fpl)
    assert len(fp) <= 255
    d_ent = rh.dev(ent)
    for dt, top, with_lut2, default in _remap_variants(name):
        lut2 = J.luts(name, len(fp), top, False)[0] if with_lut2 else None
        want = J.index_map_entries(cs, ent, lut2, default)
        got = rh.frame_remap_entries(cs.H, cs.W, d.labels, d.job_base, d_ent, default, getattr(torch, dt), lut2=None if lut2 is None else rh.dev(lut2))
        _eq(_as_int(got), want, (name, dt, with_lut2, default, "index map from entries"))


# ---- the sort path ---------------------------------------------------------------------------------------------------------------------
def _sort_unique(rh, d, cs, fix_key, black_jobs):
    """ops.Rhccq.job_sort_unique, keeping job_start and n_unique as the kernel wrote them"""
    import torch
    n, ptrs, bases = rh._class_args(d.labels, d.job_base)
    bj = rh.dev(np.asarray(black_jobs, dtype=np.int32)) if len(black_jobs) else None
    total = n * cs.H * cs.W + len(black_jobs)
    tb = int(rh.lib.rhccq_job_sort_unique_bytes(total))
    tmp = rh.empty((tb,), torch.uint8)
    rankmap = torch.full((n, cs.H * cs.W), -7, dtype=torch.int32, device=rh.device)
    keys = rh.empty((total,), torch.int32)
    start = torch.full((cs.n_jobs,), -7, dtype=torch.int32, device=rh.device)
    nu = torch.full((1,), -7, dtype=torch.int32, device=rh.device)
    rh._check(rh.lib.rhccq_job_sort_unique(rh.ctx, rh._p(d.rgb), cs.H, cs.W, n, ptrs, bases, cs.n_jobs, rh._p(fix_key), rh._p(bj), len(black_jobs),
                                           rh._p(tmp), tb, rh._p(rankmap), rh._p(keys), rh._p(start), rh._p(nu)), "job_sort_unique")
    return keys, start, nu, rankmap


@pytest.mark.parametrize("name", BITMAP)
def test_sort_path(rh, name):
    import torch
    cs, ref, d = J.case(name), J.reference(name), _dev(rh, name)
    variants = [(True, True), (False, False)] + ([(True, False), (False, True)] if name != J.BIG else [])
    for with_fix, with_black in variants:
        what = (name, with_fix, with_black)
        fk = ref.fix_key if with_fix else None
        black = ref.black_jobs if with_black else []
        pals = J.palettes(cs, fk, black)
        rank = J.ranks(cs, pals, fk)
        want_keys, want_start, want_n = J.sort_outputs(pals)
        d_fk = rh.dev(fk.view(np.int32)) if with_fix else None
        keys, start, nu, rankmap = _sort_unique(rh, d, cs, d_fk, black)
        assert int(_host(nu)[0]) == want_n, what
        _eq(_host(start), want_start, what + ("job_start",))
        _eq(_host(keys[:want_n]).view(np.uint32), want_keys, what + ("keys_out",))
        _eq(_host(rankmap), rank, what + ("rankmap",))
        # the wrapper's palette sizes
        P, k2, r2 = rh.job_sort_unique(d.rgb, d.labels, d.job_base, cs.n_jobs, d_fk, black)
        _eq(P, [len(p) for p in pals], what + ("P",))
        _eq(_host(r2), rank, what + ("rankmap (wrapper)",))
        if not (with_fix and with_black):
            continue
        # the ranked kernels against the reference and against the bitmap path
        S = _state(rh, name, "fix")
        assert np.array_equal(S.off, J.pal_offsets(pals))
        for lut in (None, J.fp_lut(name, S.total)):
            _, want_fp = J.entries(cs, rank, S.off, lut)
            d_lut = None if lut is None else rh.dev(lut)
            fp = _first_pos(rh, len(want_fp))
            rh.job_index_ranked(cs.H, cs.W, d.labels, d.job_base, rankmap, S.d_off, fp, d_lut)
            _eq(_host(fp), want_fp, what + (lut is not None, "first_pos (ranked)"))
            fp_b = _first_pos(rh, len(want_fp))
            rh.job_index(d.rgb, d.labels, d.job_base, S.bitmaps, S.prefix, S.d_off, fix_key=S.fix_key, want_idx=False, first_pos=fp_b, fp_lut=d_lut)
            assert torch.equal(fp, fp_b), what
        for dt, top, with_lut2, default in _remap_variants(name):
            lut, lut2 = J.luts(name, S.total, top, with_lut2)
            d_l, d_l2 = rh.dev(lut), None if lut2 is None else rh.dev(lut2)
            got = rh.frame_remap_ranked(cs.H, cs.W, d.labels, d.job_base, rankmap, S.d_off, d_l, default, getattr(torch, dt), lut2=d_l2)
            _eq(_as_int(got), J.index_map(cs, rank, S.off, lut, lut2, default), what + (dt, with_lut2, default, "index map (ranked)"))
            assert torch.equal(got, rh.frame_remap(d.rgb, d.labels, d.job_base, S.bitmaps, S.prefix, S.d_off, S.fix_key, d_l, default, getattr(torch, dt),
                                                   lut2=d_l2)), what


# ---- rhccq_remap / rhccq_decode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 255, 256, 1000, 262144 * 4 + 3))
def test_remap(rh, n):
    rng = np.random.default_rng(n)
    lut_n = 37
    lut = rng.integers(1, 1 << 30, lut_n).astype(np.int32)
    idx = rng.integers(0, lut_n, n).astype(np.int32)
    idx[-1] = lut_n - 1
    if n > 4:
        idx[:4] = [-1, lut_n, -(1 << 31), J.INT_MAX]           # outside the table: the documented 0
    want = np.where((idx >= 0) & (idx < lut_n), lut[np.clip(idx, 0, lut_n - 1)], 0)
    _eq(_host(rh.remap(rh.dev(idx), rh.dev(lut))), want, n)


@pytest.mark.parametrize("n", (1, 255, 256, 1000, 262144 * 4 + 3))
def test_decode(rh, n):
    import torch
    rng = np.random.default_rng(n + 1)
    for dt, pal_n in ((torch.uint8, 200), (torch.int16, 300), (torch.int32, 70000)):
        pal = rng.integers(1, 256, (pal_n, 3)).astype(np.uint8)
        idx = rng.integers(0, pal_n, n).astype(np.int64)
        idx[-1] = pal_n - 1
        if n > 4:
            idx[:3] = [pal_n, pal_n + 1, {torch.uint8: 255, torch.int16: 65535, torch.int32: (1 << 32) - 1}[dt]]      # >= pal_n: entry 0
        want = pal[np.where(idx < pal_n, idx, 0)]
        np_t = {torch.uint8: np.uint8, torch.int16: np.uint16, torch.int32: np.uint32}[dt]
        d_idx = torch.from_numpy(idx.astype(np_t).view({np.uint16: np.int16, np.uint32: np.int32}.get(np_t, np_t))).to(rh.device)
        _eq(_host(rh.decode(d_idx, rh.dev(pal))), want, (n, str(dt)))


# ---- K2 ----------------------------------------------------------------------------------------------------------------------------------
def _k2(rh, keys, labels, k):
    means, sums = rh.cluster_means(rh.dev(keys.view(np.int32)), rh.dev(labels), k)
    return _host(sums), _host(means).view(np.uint32)


@pytest.mark.parametrize("n", J.K2_SIZES)
def test_cluster_sums_and_means(rh, n):
    for kind in J.K2_KINDS:
        for k in (1, 3, 40):                       # 40 > n for the small sizes: empty clusters, mean key 0
            keys, lab = J.k2_case(n, kind, k)
            want_sums, want_means = J.k2_reference(keys, lab, k)
            sums, means = _k2(rh, keys, lab, k)
            _eq(sums, want_sums, (n, kind, k, "sums"))
            _eq(means, want_means, (n, kind, k, "means"))


def test_cluster_sums_k0(rh):
    """k = 0 takes the unpacked kernel; no label can be >= 0 then, and nothing may be written"""
    import torch
    keys, lab = J.k2_case(4099, "none", 0)
    guard = torch.full((8,), 0x5a5a5a5a, dtype=torch.int64, device=rh.device)
    d_keys, d_lab = rh.dev(keys.view(np.int32)), rh.dev(lab)
    rh._check(rh.lib.rhccq_cluster_sums(rh.ctx, rh._p(d_keys), rh._p(d_lab), len(keys), 0, rh._p(guard)), "cluster_sums")
    rh._check(rh.lib.rhccq_cluster_means(rh.ctx, rh._p(guard), 0, rh._p(guard)), "cluster_means")
    assert np.all(_host(guard) == 0x5a5a5a5a)
    means, sums = rh.cluster_means(d_keys, d_lab, 0)
    assert means.numel() == 0 and sums.numel() == 0


def _white_case(n, k):
    """keys all 0xFFFFFF (the largest sums), sorted runs of the labels 0 .. k-1 with a -1 every 1 000 points"""
    lab = (np.arange(n, dtype=np.int64) * k // n).astype(np.int32)
    lab[::1000] = -1
    cnt = np.bincount(lab[lab >= 0], minlength=k).astype(np.int64)
    return np.full(n, 0xFFFFFF, np.uint32), lab, np.stack([255 * cnt, 255 * cnt, 255 * cnt, cnt], 1)


def test_cluster_sums_packed_fields_at_their_limit(rh):
    """n = 2^24, the last size of the packed kernel, every point white and in ONE cluster: both 32-bit fields of a packed word at
    255 * 2^24, the largest value they are built for"""
    n = 1 << 24
    keys, lab = np.full(n, 0xFFFFFF, np.uint32), np.zeros(n, np.int32)
    sums, means = _k2(rh, keys, lab, 2)
    _eq(sums, [[255 * n, 255 * n, 255 * n, n], [0, 0, 0, 0]], "sums")
    _eq(means, [0xFFFFFF, 0], "means")


def test_cluster_sums_unpacked_kernel(rh):
    """n = 2^24 + 5: the first size of the unpacked kernel (four 64-bit atomics per point)"""
    n = (1 << 24) + 5
    keys, lab, want = _white_case(n, 3)
    sums, means = _k2(rh, keys, lab, 3)
    _eq(sums, want, "sums")
    _eq(means, [0xFFFFFF] * 3, "means")


# ---- argument errors: all of them return on the host before any launch ----------------------------------------------------------------
def test_argument_errors(rh):
    import torch
    name = "t6x11_c2_gap"
    cs, d, S = J.case(name), _dev(rh, name), _state(rh, name, "fix")
    H, W, p = cs.H, cs.W, rh._p
    raw = rh.dev(np.zeros(H * W * 3 + 4, np.uint8))
    odd = raw[1:1 + H * W * 3].view(H, W, 3)                   # rgb + 1
    assert odd.data_ptr() % 4 == 1
    bitmaps, stats = rh.new_job_state(cs.n_jobs)
    bytemaps = rh.zeros((cs.n_jobs, 1 << 24), torch.uint8)
    best = torch.full((cs.n_jobs,), -1, dtype=torch.int64, device=rh.device)
    flags = rh.zeros((cs.n_jobs,), torch.uint8)
    lut, _ = J.luts(name, S.total, 255, False)
    d_lut = rh.dev(lut)
    out = rh.empty((H, W), torch.int32)
    fp = _first_pos(rh, S.total)
    ent = rh.zeros((len(cs.labels), H * W), torch.int32)
    rankmap = rh.zeros((len(cs.labels), H * W), torch.int32)
    total = len(cs.labels) * H * W
    tb = int(rh.lib.rhccq_job_sort_unique_bytes(total))
    tmp = rh.empty((tb,), torch.uint8)
    keys, start, nu = rh.empty((total,), torch.int32), rh.empty((cs.n_jobs,), torch.int32), rh.empty((1,), torch.int32)
    pal = rh.dev(np.zeros((4, 3), np.uint8))
    idx8 = rh.zeros((16,), torch.uint8)
    rgb_out = rh.empty((16, 3), torch.uint8)
    lib = rh.lib

    def cls(labels=None, job_base=None):
        return rh._class_args(d.labels if labels is None else labels, d.job_base if job_base is None else job_base)

    def calls(rgb, H, W, n, ptrs, bases, out_bytes=4, idx_bytes=1, tmp_bytes=tb):
        return {
            "job_scan": lambda: lib.rhccq_job_scan(rh.ctx, p(rgb), H, W, n, ptrs, bases, 0, p(bitmaps), p(stats)),
            "job_scan_bytes": lambda: lib.rhccq_job_scan_bytes(rh.ctx, p(rgb), H, W, n, ptrs, bases, 0, p(bytemaps), p(stats)),
            "job_stats": lambda: lib.rhccq_job_stats(rh.ctx, p(rgb), H, W, n, ptrs, bases, p(stats)),
            "job_blackfix": lambda: lib.rhccq_job_blackfix(rh.ctx, p(rgb), H, W, n, ptrs, bases, p(flags), p(best)),
            "job_index": lambda: lib.rhccq_job_index(rh.ctx, p(rgb), H, W, n, ptrs, bases, p(S.bitmaps), p(S.prefix), p(S.d_off), p(S.fix_key), p(ent),
                                                     p(fp), None),
            "job_index_entries": lambda: lib.rhccq_job_index_entries(rh.ctx, p(rgb), H, W, n, ptrs, bases, p(S.bitmaps), p(S.prefix), p(S.d_off),
                                                                     p(S.fix_key), p(fp), None, p(ent)),
            "frame_remap": lambda: lib.rhccq_frame_remap(rh.ctx, p(rgb), H, W, n, ptrs, bases, p(S.bitmaps), p(S.prefix), p(S.d_off), p(S.fix_key),
                                                         p(d_lut), None, 0, p(out), out_bytes),
            "frame_remap_entries": lambda: lib.rhccq_frame_remap_entries(rh.ctx, H, W, n, ptrs, bases, p(ent), None, 0, p(out), out_bytes),
            "frame_remap_ranked": lambda: lib.rhccq_frame_remap_ranked(rh.ctx, H, W, n, ptrs, bases, p(rankmap), p(S.d_off), p(d_lut), None, 0, p(out),
                                                                       out_bytes),
            "job_index_ranked": lambda: lib.rhccq_job_index_ranked(rh.ctx, H, W, n, ptrs, bases, p(rankmap), p(S.d_off), p(fp), None),
            "job_sort_unique": lambda: lib.rhccq_job_sort_unique(rh.ctx, p(rgb), H, W, n, ptrs, bases, cs.n_jobs, None, None, 0, p(tmp), tmp_bytes,
                                                                 p(rankmap), p(keys), p(start), p(nu)),
            "decode": lambda: lib.rhccq_decode(rh.ctx, p(idx8), idx_bytes, 16, p(pal), 4, p(rgb_out)),
        }

    def refused(fn, what, names):
        """E_ARG, and a message of THIS refusal: the last error is first set to another entry point's, then has to name `names`"""
        rh.sync()
        assert lib.rhccq_remap(rh.ctx, None, -1, None, 0, None) == E_ARG
        assert rh._raw.rhccq_last_error(rh.ctx).decode().startswith("remap:")
        rc = fn()
        msg = (rh._raw.rhccq_last_error(rh.ctx) or b"").decode()
        assert rc == E_ARG and not msg.startswith("remap:") and names in msg, (what, rc, msg)

    per_class = [k for k in calls(d.rgb, H, W, *cls()) if k != "decode"]
    with_rgb = ("job_scan", "job_scan_bytes", "job_stats", "job_blackfix", "job_index", "job_index_entries", "frame_remap", "job_sort_unique")
    # n_class 0 and 5
    lab5 = [d.labels[0]] * 5
    for n_args in (cls([], []), cls(lab5, [0] * 5)):
        for k in per_class:
            refused(calls(d.rgb, H, W, *n_args)[k], (k, "n_class", n_args[0]), "n_class")
    # H or W <= 0
    for h, w in ((0, W), (H, 0), (-1, W), (H, -3)):
        for k in per_class:
            refused(calls(d.rgb, h, w, *cls())[k], (k, "H, W", h, w), k + ":")
    # element sizes
    for k in ("frame_remap", "frame_remap_entries", "frame_remap_ranked"):
        refused(calls(d.rgb, H, W, *cls(), out_bytes=3)[k], (k, "out_elem_bytes"), "out_elem_bytes")
    refused(calls(d.rgb, H, W, *cls(), idx_bytes=3)["decode"], "idx_elem_bytes", "idx_elem_bytes")
    # scratch one byte short
    refused(calls(d.rgb, H, W, *cls(), tmp_bytes=tb - 1)["job_sort_unique"], "tmp_bytes", "job_sort_unique: tmp")
    # rgb + 1: the kernels read four pixels as three dwords
    for k in ("job_scan", "job_scan_bytes", "job_stats", "job_blackfix", "job_index", "job_index_entries", "frame_remap"):
        refused(calls(odd, H, W, *cls())[k], (k, "rgb + 1"), k + ": rgb must be 4-byte aligned")
    assert set(with_rgb) <= set(per_class)
    # nothing was launched or written, and the context still works
    rh.sync()
    assert np.all(_host(best) == -1) and not bool(bitmaps.any()) and not bool(bytemaps.any())
    _eq(_host(stats), np.tile([J.INT_MAX, -1, J.INT_MAX, -1, 0, 0], (cs.n_jobs, 1)), "stats untouched")
    _eq(_host(rh.job_stats(d.rgb, d.labels, d.job_base, cs.n_jobs)), J.reference(name).stats, "a correct call afterwards")
