"""RHCCQ_OPT_CHAIN_RELEASE: every level-1 problem of a frame goes on the moment ITS k-means++ chain has ended inside the frame's one chain
launch (rhccq_mbk_init_released publishes a flag per problem; the problem's lane waits for it on the host), against the wait for the whole
launch.  Same frame bit for bit either way, with per-lane chains (RHCCQ_OPT_FRAME_CHAINS = 0) and through FrameEncoder.encode; a chain
kernel that publishes nothing falls back to the launch's event; and the hand-off itself, every word, under uneven load.  GPU only.

The frames are uniform-random RGB, W = 256, quality 50, in horizontal bands: nearly every pixel is a colour of its own, so a segment of P
pixels is a MiniBatchKMeans problem (>= 10 000 colours) of k ~ P / 20, and its chain's length goes with k."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = 256


@pytest.fixture(scope="module")
def rh():
    from roibasedimagecompression_amd.ops import Rhccq
    r = Rhccq(0)
    yield r
    r.set_option(Rhccq.OPT_CHAIN_RELEASE, 1)
    r.set_option(Rhccq.OPT_FRAME_CHAINS, 1)
    r.set_option(Rhccq.OPT_INIT_KERNEL, 0)


def _frame(rh, class_rows, seed):
    """class_rows[c] = the heights of class c's segments, bands from the top in class order; one region per class"""
    import torch
    from roibasedimagecompression_amd.frame import ClassSpec
    H = sum(sum(r) for r in class_rows)
    img = np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)
    specs, r = [], 0
    for rows in class_rows:
        lab = np.zeros((H, W), np.int32)
        top = r
        for s, h in enumerate(rows):
            lab[r:r + h] = s + 1
            r += h
        specs.append(ClassSpec(torch.from_numpy(lab).to(rh.device), np.zeros(len(rows), np.int64), [(top, 0, r, W)], 50))
    return torch.from_numpy(img).to(rh.device), specs


def _same(a, b):
    import torch
    assert np.array_equal(a["palette"], b["palette"])
    assert a["indices_dtype"] == b["indices_dtype"] and torch.equal(a["indices"], b["indices"])
    assert np.array_equal(a["n_unique"], b["n_unique"])
    assert tuple(a["shape"]) == tuple(b["shape"]) and tuple(a["top_left"]) == tuple(b["top_left"]) and a["quality3"] == b["quality3"]


def _fits(rh):
    info = np.zeros((8, 6), np.int64)
    n = rh._raw.rhccq_encode_frame_level2_info(rh.ctx, 8, info.ctypes.data)
    assert 0 <= n <= 8
    return info[:n].copy()


def _all_ways(rh, rgb, specs, init_kernel=0, python_too=True):
    """release 1, 0, 1 again, per-lane chains and FrameEncoder.encode: one frame; the level-2 report equal for the two release settings"""
    from roibasedimagecompression_amd.frame import FrameEncoder
    from roibasedimagecompression_amd.ops import Rhccq
    enc = FrameEncoder(rh)
    rh.set_option(Rhccq.OPT_INIT_KERNEL, init_kernel)
    rh.set_option(Rhccq.OPT_FRAME_CHAINS, 1)
    outs, fits = [], []
    try:
        for rel in (1, 0, 1):                            # release twice: warm lanes, reused arenas and the previous frame's flags must not matter
            rh.set_option(Rhccq.OPT_CHAIN_RELEASE, rel)
            outs.append(enc.encode_native(rgb, specs))
            fits.append(_fits(rh))
        rh.set_option(Rhccq.OPT_FRAME_CHAINS, 0)         # (the release option has no effect here)
        lanes = enc.encode_native(rgb, specs)
    finally:
        rh.set_option(Rhccq.OPT_FRAME_CHAINS, 1)
        rh.set_option(Rhccq.OPT_CHAIN_RELEASE, 1)
        rh.set_option(Rhccq.OPT_INIT_KERNEL, 0)
    _same(outs[0], outs[1])
    _same(outs[0], outs[2])
    _same(outs[0], lanes)
    assert np.array_equal(fits[0], fits[1]) and np.array_equal(fits[0], fits[2])
    if python_too:
        _same(enc.encode(rgb, specs), outs[0])
    return outs[0]


FRAME_B = ((50, 50), (150, 150))                         # the bench's shape in small: chains of k ~ 640 beside chains of k ~ 1 920
FRAME_C = ((44,) * 10, (200,))                           # ten problems on eight sublanes (two carry two) beside one long chain


def _expect_minibatch(out, class_rows):
    rows = [h for cr in class_rows for h in cr]
    assert len(out["n_unique"]) == len(rows)
    for n, h in zip(out["n_unique"], rows):
        assert 10000 + 1 <= n <= h * W + 1               # every band clears the MiniBatchKMeans threshold (+ 1: black where the crop shows a neighbour)


@pytest.fixture(scope="module")
def frame_b(rh):
    """frame B and what every way of encoding it gives with the default chain kernel (computed once, only read afterwards)"""
    rgb, specs = _frame(rh, FRAME_B, 11)
    return rgb, specs, _all_ways(rh, rgb, specs)


def test_frame_b_short_and_long_chains(rh, frame_b):
    out = frame_b[2]
    _expect_minibatch(out, FRAME_B)
    nu = out["n_unique"]
    assert min(nu[2:]) > 2.9 * max(nu[:2])               # the chains differ 3x


def test_frame_c_more_problems_than_sublanes(rh):
    rgb, specs = _frame(rh, FRAME_C, 12)
    out = _all_ways(rh, rgb, specs)
    _expect_minibatch(out, FRAME_C)


def test_fallback_chain_kernel_that_publishes_nothing(rh, frame_b):
    """RHCCQ_OPT_INIT_KERNEL = 2: the second-generation chain sets no flag; the lanes are let go by the launch's event, on the host"""
    rgb, specs, want = frame_b
    _same(_all_ways(rh, rgb, specs, init_kernel=2, python_too=False), want)


def test_option_validation(rh):
    from roibasedimagecompression_amd.ops import Rhccq, RhccqError
    for bad in (-1, 2, 7):
        with pytest.raises(RhccqError, match=r"\(-1\)"):
            rh.set_option(Rhccq.OPT_CHAIN_RELEASE, bad)
    rh.set_option(Rhccq.OPT_CHAIN_RELEASE, 0)
    rh.set_option(Rhccq.OPT_CHAIN_RELEASE, 1)


# ---- the hand-off -----------------------------------------------------------------------------------------------------------------
def _chain_inputs(rh, palettes, ks):
    """what rhccq_mbk_init takes for these problems (ops.minibatch_kmeans's set-up: rhccq_mbk_draws per problem, the uniforms from the
    device's word table)"""
    import torch
    from roibasedimagecompression_amd._lib import MbkDraw, MbkProblem
    n_prob = len(palettes)
    probs = (MbkProblem * n_prob)()
    keys = rh.dev(np.concatenate(palettes).astype(np.uint32).view(np.int32))
    init_list, draws = [], []
    off = koff = ioff = roff = 0
    for i, (pal, k) in enumerate(zip(palettes, ks)):
        n, d = len(pal), MbkDraw()
        assert rh._raw.rhccq_mbk_draws(n, k, C.byref(d), None, 0) == 0 and d.init_size < n
        init_idx = np.empty(d.init_size, np.int32)
        assert rh._raw.rhccq_mbk_draws(n, k, C.byref(d), init_idx.ctypes.data, d.init_size) == 0
        p = probs[i]
        p.off, p.n, p.k, p.koff = off, n, k, koff
        p.init_off, p.init_n, p.rand_off, p.first, p.T = ioff, d.init_size, roff, d.first, d.T
        init_list.append(init_idx)
        draws.append(d)
        off += n
        koff += k
        ioff += d.init_size
        roff += d.n_uniforms
    words, _ = rh._mt_words(max(d.pos + 2 * d.n_uniforms for d in draws))
    d_rand = rh.empty((roff,), torch.float64)
    for p, d in zip(probs, draws):
        rh._check(rh.lib.rhccq_mt_uniforms(rh.ctx, words, d.pos, d.n_uniforms, C.c_void_p(d_rand.data_ptr() + 8 * p.rand_off)), "mt_uniforms")
    d_init = rh.dev(np.concatenate(init_list))
    obytes = int(rh.lib.rhccq_mbk_order_bytes(ioff))
    otmp = rh.empty((obytes,), torch.uint8)
    d_perm = rh.empty((ioff,), torch.int32)
    rh._check(rh.lib.rhccq_mbk_order(rh.ctx, rh._p(keys), probs, n_prob, rh._p(d_init), rh._p(d_perm), rh._p(otmp), obytes), "mbk_order")
    torch.cuda.synchronize()
    return dict(keys=keys, probs=probs, n_prob=n_prob, d_init=d_init, d_perm=d_perm, d_rand=d_rand, K=koff, keep=otmp)


# the chain kernel's two publishing variants: init samples in global memory (a problem above 5 760 samples; the release record lies in the
# sample area) and in LDS (every problem at most 5 760 samples: k <= 1 900; flag and tag come from the kernel's argument segment)
HAND_OFFS = {"samples_in_global_memory": ((301, 1203, 3600), (10000, 20000, 40000)),
             "samples_in_lds": ((151, 603, 1900), (10000, 12000, 20000))}


@pytest.mark.parametrize("case", sorted(HAND_OFFS))
def test_hand_off_every_word_under_uneven_load(rh, case):
    """One released launch of three problems whose chains differ 12x (k = 301 / 1 203 / 3 600, or 151 / 603 / 1 900: the slices' borders
    fall INSIDE 128-byte lines), a second stream keeping the chip unevenly busy, a third stream that has read every slice once while the
    chains ran (a stale copy exists wherever one can) and copies a problem's slice, extended to whole lines, the moment its flag shows.
    The problem's own words must then be what they are after the launch and what a plain rhccq_mbk_init gives; every flag but the
    longest problem's must show before the launch's event completes."""
    import torch
    rng = np.random.RandomState(5)
    ks, sizes = HAND_OFFS[case]
    palettes = [np.unique(rng.randint(1, 1 << 24, n).astype(np.uint32)) for n in sizes]
    S = _chain_inputs(rh, palettes, ks)
    K, n_prob = S["K"], S["n_prob"]
    assert all(S["probs"][i].init_n <= 5760 for i in range(n_prob)) == (case == "samples_in_lds")     # which variant the launch takes
    koff = np.concatenate([[0], np.cumsum(ks)])

    def launch(released, centres, chosen, flags_dev=None, tag=0):
        args = (rh.ctx, rh._p(S["keys"]), S["probs"], n_prob, rh._p(S["d_init"]), rh._p(S["d_perm"]), rh._p(S["d_rand"]), rh._p(centres), rh._p(chosen))
        if not released:
            rh._check(rh.lib.rhccq_mbk_init(*args), "mbk_init")
            return 0
        pub = C.c_int32(-1)
        rh._check(rh.lib.rhccq_mbk_init_released(*args, flags_dev, tag, C.byref(pub)), "mbk_init_released")
        return pub.value

    # the plain launch: the reference, and the code object is loaded
    ref_c, ref_ch = rh.zeros((K + 4, 4), torch.float64), rh.zeros((K,), torch.int32)
    launch(False, ref_c, ref_ch)
    torch.cuda.synchronize()
    ref = ref_c.cpu().numpy()
    assert (ref[:K, :3].max(axis=1) > 0).all()           # every centre was written (no palette holds black)

    fh, fd = C.c_void_p(), C.c_void_p()
    assert rh._raw.rhccq_release_flags_alloc(n_prob, C.byref(fh), C.byref(fd)) == 0
    try:
        flags = np.ctypeslib.as_array((C.c_uint32 * (16 * n_prob)).from_address(fh.value))
        assert not flags.any()
        # bad arguments: no flags, tag 0
        assert rh._raw.rhccq_mbk_init_released(rh.ctx, rh._p(S["keys"]), S["probs"], n_prob, rh._p(S["d_init"]), rh._p(S["d_perm"]), rh._p(S["d_rand"]),
                                               rh._p(ref_c), rh._p(ref_ch), fd, 0, C.byref(C.c_int32())) == -1
        lines = [(int(koff[p]) // 4 * 4, (int(koff[p + 1]) + 3) // 4 * 4) for p in range(n_prob)]      # whole 128-byte lines = 4 centres
        chain_s, load_s, read_s = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        load = torch.ones(96 << 20, dtype=torch.float32, device=rh.device)                              # 384 MB
        # everything the timed part uses has run once on its stream (a kernel module loaded at its first use would stall the host for
        # longer than the chains take)
        with torch.cuda.stream(load_s):
            load.mul_(1.0)
            load[:1 << 20].mul_(1.0)
        with torch.cuda.stream(read_s):
            warm = [ref_c[lo:hi].clone() for lo, hi in lines]
        warm_ev = torch.cuda.Event()
        with torch.cuda.stream(chain_s):
            warm_ev.record()
        torch.cuda.synchronize()
        assert warm_ev.query() and len(warm) == n_prob
        for tag in (7, 8):                                # twice: the second launch finds the first one's tags in the flags
            centres, chosen = rh.zeros((K + 4, 4), torch.float64), rh.zeros((K,), torch.int32)
            torch.cuda.synchronize()
            done = torch.cuda.Event()
            with torch.cuda.stream(load_s):               # uneven: whole-buffer passes between short ones, for longer than the longest chain
                for i in range(160):
                    (load if i % 3 else load[:1 << 20]).mul_(1.0)
            with torch.cuda.stream(chain_s):
                t_launch = time.perf_counter()
                assert launch(True, centres, chosen, fd, tag) == 1
                done.record()
            with torch.cuda.stream(read_s):               # every slice once while the chains run
                early = [centres[lo:hi].clone() for lo, hi in lines]
            seen, at_flag, before_event = set(), {}, {}
            t_loop, t_seen, looks = time.perf_counter(), {}, 0
            while len(seen) < n_prob:
                ended = done.query()
                looks += 1
                for p in range(n_prob):
                    if p not in seen and flags[16 * p] == tag:
                        seen.add(p)
                        before_event[p] = not ended
                        t_seen[p] = time.perf_counter()
                        with torch.cuda.stream(read_s):
                            at_flag[p] = centres[lines[p][0]:lines[p][1]].clone()
                if ended and len(seen) < n_prob:
                    pytest.fail(f"the launch ended and the flags of problems {sorted(set(range(n_prob)) - seen)} never showed tag {tag}: {flags[::16]}")
            torch.cuda.synchronize()
            print(f"{case} tag {tag}: launch + early reads queued in {(t_loop - t_launch) * 1e3:.2f} ms, flags seen after "
                  f"{[round((t_seen[p] - t_launch) * 1e3, 2) for p in range(n_prob)]} ms, launch ended by {(time.perf_counter() - t_launch) * 1e3:.2f} ms, "
                  f"{looks} looks, released before the event: {before_event}")
            final = centres.cpu().numpy()
            assert all(int(v) == tag for v in flags[::16])
            for p in range(n_prob):
                lo, hi = lines[p]
                own = slice(int(koff[p]) - lo, int(koff[p + 1]) - lo)
                got = at_flag[p].cpu().numpy()
                assert np.array_equal(got[own], final[lo:hi][own]), f"problem {p}: its slice at the flag is not what it is after the launch"
                assert np.array_equal(got[own], ref[lo:hi][own]), f"problem {p}: its slice at the flag is not the plain launch's"
                assert early[p].shape == got.shape
            assert np.array_equal(final[:K], ref[:K]) and np.array_equal(chosen.cpu().numpy(), ref_ch.cpu().numpy())
            assert before_event[0] and before_event[1], before_event      # all but the longest chain: released while the launch still ran
    finally:
        torch.cuda.synchronize()
        rh._raw.rhccq_release_flags_free(fh)
