"""error_sums_kernel, error_tables_kernel, ssim7_kernel (csrc/metrics.hip) and dct_quant_kernel<8|16>, luma_kernel, qstep_kernel
(csrc/dct_ext.hip) on the cases of tests/metric_cases.py, through Rhccq.error_sums, error_tables, ssim7, dct_quant and luma_qstep:
every code path by input size, against references that share nothing with the device code or the oracle.  Integers are compared
for equality; the SSIM partials and means and the DCT coefficients against the rounding-error bounds derived in metric_cases.
tests/test_metric_cases_cpu.py proves, without a GPU, which path each case takes.  GPU only.

Measured on an MI355X (test_worst_differences_are_inside_the_bounds prints the figures): SSIM partials and means within 6.9e-16 of the
exact sums, where 3.3e-12 is allowed for a tile of one window; the worst DCT coefficient 7.629e-06 from the reference where 7.629e-06
(half a float32 ulp plus 1.3e-11) is allowed, a correctly rounded near-tie."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import metric_cases as MC

pytestmark = pytest.mark.gpu

E_ARG = -1                    # RHCCQ_E_ARG (include/rhccq.h)
WORST = {}                    # what the tests of this module measured: name -> (difference, allowed, case)


def _new_context():
    import torch
    from roibasedimagecompression_amd.ops import Rhccq
    assert torch.cuda.is_available()
    return Rhccq(0)


@pytest.fixture(scope="module")
def rh():
    return _new_context()


def _dev(rh, arr):
    import torch
    return torch.tensor(arr, device=rh.device)


def _offset_view(rh, arr, offset):
    """a contiguous device copy of arr whose first byte sits `offset` bytes behind an aligned allocation"""
    import torch
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = torch.zeros(len(raw) + 64, dtype=torch.uint8, device=rh.device)
    assert buf.data_ptr() % 64 == 0
    v = buf[offset:offset + len(raw)]
    v.copy_(torch.tensor(raw))
    assert v.is_contiguous() and v.data_ptr() % 64 == offset
    return v


def _note(key, diff, allowed, case):
    if key not in WORST or diff / allowed > WORST[key][0] / WORST[key][1]:
        WORST[key] = (diff, allowed, case)


# ---- error sums ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MC.SUMS))
def test_error_sums_equal_reference(rh, name):
    tags, a, b = MC.sums_case(name)
    got = rh.error_sums(_dev(rh, a), _dev(rh, b))
    want = MC.sums_reference(name)
    assert got.dtype == np.int64 and np.array_equal(got, want), dict(case=name, tags=sorted(tags), n_px=len(a), got=got.tolist(), wanted=want.tolist())
    swapped = rh.error_sums(_dev(rh, b), _dev(rh, a))                  # |a - b| is symmetric
    assert np.array_equal(swapped, want), dict(case=name, tags=sorted(tags), swapped=swapped.tolist(), wanted=want.tolist())


@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_error_sums_refuses_a_pointer_off_four_bytes(rh, which):
    """rhccq_error_sums returns its argument error, enqueues nothing (the sums keep what they held) and the context stays usable"""
    import torch
    tags, a, b = MC.sums_case("n1026")
    da = _offset_view(rh, a, 1 if which in ("a", "both") else 0)
    db = _offset_view(rh, b, 1 if which in ("b", "both") else 0)
    sums = torch.full((5,), -7, dtype=torch.int64, device=rh.device)
    rc = rh.lib.rhccq_error_sums(rh.ctx, rh._p(da), rh._p(db), len(a), rh._p(sums))
    torch.cuda.synchronize()
    assert rc == E_ARG and b"4-byte aligned" in rh._raw.rhccq_last_error(rh.ctx), (which, rc)
    assert sums.cpu().tolist() == [-7] * 5
    assert np.array_equal(rh.error_sums(_dev(rh, a), _dev(rh, b)), MC.sums_reference("n1026"))
    assert np.array_equal(rh.error_sums(_offset_view(rh, a, 4), _offset_view(rh, b, 8)), MC.sums_reference("n1026"))      # 4-byte offsets pass


# ---- error tables ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_maxerr", [False, True], ids=["no_maxerr", "maxerr"])
@pytest.mark.parametrize("name", list(MC.TABLES))
def test_error_tables_equal_reference(rh, name, want_maxerr):
    tags, a, b = MC.tables_case(name)
    n = len(a)
    tab, me = rh.error_tables(_dev(rh, a).view(1, n, 3), _dev(rh, b).view(1, n, 3), want_maxerr=want_maxerr)
    want, plane = MC.tables_reference(name)
    rows = np.nonzero((tab != want).any(axis=1))[0]
    assert tab.dtype == np.int64 and tab.shape == (256, 3) and len(rows) == 0, dict(
        case=name, tags=sorted(tags), n_px=n, rows=rows[:8].tolist(), got=tab[rows[:8]].tolist(), wanted=want[rows[:8]].tolist())
    if want_maxerr:
        got = me.cpu().numpy().reshape(-1)
        bad = np.nonzero(got != plane)[0]
        assert got.dtype == np.uint8 and len(bad) == 0, dict(case=name, tags=sorted(tags), pixels=bad[:8].tolist(), got=got[bad[:8]].tolist(),
                                                             wanted=plane[bad[:8]].tolist())
    else:
        assert me is None


@pytest.mark.parametrize("name", ["n257", "worst_channel", "hw_39x38"])
def test_error_tables_at_odd_byte_offsets(rh, name):
    """rhccq_error_tables has no alignment rule: both images and the error plane at odd addresses"""
    import torch
    tags, a, b = MC.tables_case(name)
    n = len(a)
    want, plane = MC.tables_reference(name)
    da, db = _offset_view(rh, a, 1), _offset_view(rh, b, 3)
    tab = torch.full((256, 3), -1, dtype=torch.int64, device=rh.device)
    me = torch.zeros(n + 16, dtype=torch.uint8, device=rh.device)
    rc = rh.lib.rhccq_error_tables(rh.ctx, rh._p(da), rh._p(db), n, rh._p(tab), C.c_void_p(me.data_ptr() + 5))
    assert rc == 0 and np.array_equal(tab.cpu().numpy(), want), (name, sorted(tags))
    got = me.cpu().numpy()
    assert np.array_equal(got[5:5 + n], plane) and not got[:5].any() and not got[5 + n:].any(), (name, sorted(tags))


# ---- ssim7 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MC.SSIM))
def test_ssim7_partials_and_mean_are_inside_the_bound(rh, name):
    tags, a, b = MC.ssim_case(name)
    H, W = a.shape[:2]
    ty, tx, _, _ = MC.ssim_grid(H, W)
    partial, count, total = MC.ssim_reference(name)
    n = (H - 6) * (W - 6)
    da, db = _dev(rh, a), _dev(rh, b)
    mean, part = rh.ssim7(da, db, return_partial=True)
    assert part.dtype == mean.dtype == np.float64 and part.shape == (ty, tx, 3) and mean.shape == (3,)
    assert np.array_equal(rh.ssim7(da, db), mean)                       # the default result is the mean alone
    bad = []
    for i in range(ty):
        for j in range(tx):
            allowed = MC.ssim_partial_bound(int(count[i, j]))
            for ch in range(3):
                d = MC.ssim_diff(part[i, j, ch], partial[i][j][ch])
                _note("ssim partial", d, allowed, name)
                if d > allowed:
                    bad.append(dict(tile=(i, j), channel=ch, windows=int(count[i, j]), got=float(part[i, j, ch]),
                                    wanted=float(Fraction(partial[i][j][ch], 1 << MC.SSIM_FRAC_BITS)), difference=d, allowed=allowed))
    assert not bad, dict(case=name, tags=sorted(tags), bad=bad[:6])
    for ch in range(3):
        d = MC.ssim_diff(mean[ch], total[ch], n)
        _note("ssim mean", d, MC.ssim_mean_bound(n), name)
        assert d <= MC.ssim_mean_bound(n), dict(case=name, tags=sorted(tags), channel=ch, got=float(mean[ch]),
                                               wanted=float(Fraction(total[ch], n << MC.SSIM_FRAC_BITS)), difference=d, allowed=MC.ssim_mean_bound(n))
    if tags & {"identical", "white_white"}:                            # every term is exactly 1.0
        assert np.array_equal(part, np.broadcast_to(count[..., None].astype(np.float64), part.shape)) and (mean == 1.0).all(), dict(
            case=name, tags=sorted(tags), got=part.tolist(), wanted=count.tolist(), mean=mean.tolist())
    if "apron_pixel" in tags:                                          # only the last tile holds a window that reaches the pixel
        exact = np.broadcast_to(count[..., None].astype(np.float64), part.shape)
        same = part == exact
        assert same.reshape(-1, 3)[:-1].all() and (part[-1, -1] < exact[-1, -1]).all(), dict(case=name, tags=sorted(tags), got=part.tolist(), counts=count.tolist())


def test_ssim7_refuses_small_images_and_a_wrong_block_count(rh):
    import torch
    _, a, b = MC.ssim_case("random_13x100")
    da, db = _dev(rh, a), _dev(rh, b)
    part = torch.full((8, 3), -3.0, dtype=torch.float64, device=rh.device)
    nb = int(rh.lib.rhccq_ssim7_blocks(13, 100))
    assert nb == 3 and rh.lib.rhccq_ssim7_blocks(6, 100) == 0 and rh.lib.rhccq_ssim7_blocks(100, 6) == 0 and rh.lib.rhccq_ssim7_blocks(7, 7) == 1
    for H, W, blocks in ((6, 100, 3), (13, 6, 1), (6, 6, 0), (13, 100, nb - 1), (13, 100, nb + 1), (13, 100, 0)):
        rc = rh.lib.rhccq_ssim7_sums(rh.ctx, rh._p(da), rh._p(db), H, W, rh._p(part), blocks)
        assert rc == E_ARG, (H, W, blocks, rc)
    torch.cuda.synchronize()
    assert (part.cpu().numpy() == -3.0).all()                           # nothing was launched
    for shape in ((6, 7, 3), (7, 6, 3), (3, 3, 3)):
        with pytest.raises(ValueError, match="win_size exceeds image extent"):
            rh.ssim7(_dev(rh, np.zeros(shape, np.uint8)), _dev(rh, np.zeros(shape, np.uint8)))
    assert rh.lib.rhccq_ssim7_sums(rh.ctx, rh._p(da), rh._p(db), 13, 100, rh._p(part), nb) == 0
    assert (part.cpu().numpy()[:nb] != -3.0).all() and (part.cpu().numpy()[nb:] == -3.0).all()


# ---- dct_quant ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MC.DCT))
def test_dct_quant_equals_reference(rh, name):
    tags, B, plane, qstep = MC.dct_case(name)
    coef, ratio, q = MC.dct_reference(name)
    dp, dq = _dev(rh, plane), _dev(rh, qstep)
    got_c, got_q = rh.dct_quant(dp, B, dq)
    none_c, lone_q = rh.dct_quant(dp, B, dq, want_coef=False)           # coef_out == NULL
    got_c, got_q, lone_q = got_c.cpu().numpy(), got_q.cpu().numpy(), lone_q.cpu().numpy()
    assert none_c is None and got_c.dtype == np.float32 and got_q.dtype == lone_q.dtype == np.int16 and got_c.shape == got_q.shape == plane.shape
    for what, g in (("q", got_q), ("q without coef_out", lone_q)):
        ys, xs = np.nonzero(g.astype(np.int64) != q)
        assert len(ys) == 0, dict(case=name, tags=sorted(tags), what=what, differing=len(ys), at=list(zip(ys[:6].tolist(), xs[:6].tolist())),
                                  got=g[ys[:6], xs[:6]].tolist(), wanted=q[ys[:6], xs[:6]].tolist(), ratio=[float(v) for v in ratio[ys[:6], xs[:6]]])
    diff, tol = np.abs(got_c.astype(np.longdouble) - coef), MC.dct_tol(coef, B)
    k = np.unravel_index(np.argmax(diff / tol), diff.shape)
    _note(f"dct B={B}", float(diff[k]), float(tol[k]), name)
    ys, xs = np.nonzero(diff > tol)
    assert len(ys) == 0, dict(case=name, tags=sorted(tags), differing=len(ys), at=list(zip(ys[:6].tolist(), xs[:6].tolist())),
                              got=got_c[ys[:6], xs[:6]].tolist(), wanted=[float(v) for v in coef[ys[:6], xs[:6]]],
                              difference=[float(v) for v in diff[ys[:6], xs[:6]]], allowed=[float(v) for v in tol[ys[:6], xs[:6]]])


def test_dct_quant_refuses_bad_arguments(rh):
    import torch
    _, B, plane, qstep = MC.dct_case("luma_b8_24x72")
    dp, dq = _dev(rh, plane), _dev(rh, qstep)
    q = torch.full((24, 72), -9, dtype=torch.int16, device=rh.device)
    coef = torch.full((24, 72), -9.0, dtype=torch.float32, device=rh.device)
    call = lambda p, H, W, blk: rh.lib.rhccq_dct_quant(rh.ctx, p, H, W, blk, rh._p(dq), rh._p(coef), rh._p(q))
    assert call(rh._p(dp), 24, 72, 4) == E_ARG                          # a block of 4
    assert call(rh._p(dp), 24, 72, 32) == E_ARG
    assert call(rh._p(dp), 24, 72, 16) == E_ARG                         # 16 does not divide 24
    assert call(rh._p(dp), 20, 72, 8) == E_ARG and call(rh._p(dp), 24, 68, 8) == E_ARG
    off = _offset_view(rh, plane, 4)                                    # float-aligned, not 16-byte aligned
    assert call(rh._p(off), 24, 72, 8) == E_ARG and b"16-byte aligned" in rh._raw.rhccq_last_error(rh.ctx)
    torch.cuda.synchronize()
    assert (q.cpu().numpy() == -9).all() and (coef.cpu().numpy() == -9.0).all()
    assert call(rh._p(_offset_view(rh, plane, 16)), 24, 72, 8) == 0 and np.array_equal(q.cpu().numpy().astype(np.int64), MC.dct_reference("luma_b8_24x72")[2])


# ---- luma_qstep --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["corner_pixels", "null_mask"])
@pytest.mark.parametrize("name", list(MC.LUMA_QSTEP))
def test_luma_qstep_equals_reference(rh, name, mask):
    B, rgb, roi = MC.luma_case(name)
    luma, qstep = rh.luma_qstep(_dev(rh, rgb), _dev(rh, roi) if mask == "corner_pixels" else None, B, 4.0, 16.0)
    luma, qstep = luma.cpu().numpy(), qstep.cpu().numpy()
    want = MC.luma_f32(rgb)
    ys, xs = np.nonzero(luma != want)
    assert luma.dtype == np.float32 and len(ys) == 0, dict(case=name, differing=len(ys), at=list(zip(ys[:6].tolist(), xs[:6].tolist())),
                                                           got=luma[ys[:6], xs[:6]].tolist(), wanted=want[ys[:6], xs[:6]].tolist())
    want_q = MC.qstep_reference(roi if mask == "corner_pixels" else np.zeros_like(roi), B, 4.0, 16.0)
    ys, xs = np.nonzero(qstep != want_q)
    assert qstep.dtype == np.float32 and qstep.shape == want_q.shape and len(ys) == 0, dict(
        case=name, mask=mask, differing=len(ys), blocks=list(zip(ys[:6].tolist(), xs[:6].tolist())), got=qstep[ys[:6], xs[:6]].tolist())


# ---- the mirror's host arithmetic over the same kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in MC.SUMS if "hw" in MC.SUMS[n][0]])
def test_calculate_quality_metrics_from_the_integer_reference(name):
    """mse, mae, max_error, mse_r/g/b of calculate_quality_metrics are the integer sums converted as api/comparison.py converts them:
    equal to the last bit, with the same scalar types"""
    from decoder.uncompression.comparison import calculate_quality_metrics
    tags, a, b = MC.sums_case(name)
    H, W = MC.hw_shape(name)
    s = [int(v) for v in MC.sums_reference(name)]
    got = calculate_quality_metrics(a.reshape(H, W, 3).copy(), b.reshape(H, W, 3).copy())
    mse64 = (s[0] + s[1] + s[2]) / (3.0 * H * W)
    want = {"mse": np.float32(mse64), "rmse": np.sqrt(np.float32(mse64)), "mae": np.float32(s[3] / (3.0 * H * W)), "max_error": np.float32(s[4]),
            "mse_r": np.float32(s[0] / float(H * W)), "mse_g": np.float32(s[1] / float(H * W)), "mse_b": np.float32(s[2] / float(H * W)),
            "psnr": np.float64(10.0) * np.log10(np.float64(255.0 ** 2) / np.float64(mse64))}
    for k, w in want.items():
        assert type(got[k]) is type(w) and got[k] == w, dict(case=name, tags=sorted(tags), key=k, got=got[k], wanted=w)


@pytest.mark.parametrize("name", [n for n in MC.TABLES if "hw" in MC.TABLES[n][0]])
def test_calculate_adaptive_quality_metrics_from_the_integer_reference(name):
    from decoder.uncompression.comparison import calculate_adaptive_quality_metrics
    tags, a, b = MC.tables_case(name)
    H, W = MC.hw_shape(name)
    tab, plane = MC.tables_reference(name)
    n = H * W
    got = calculate_adaptive_quality_metrics(a.reshape(H, W, 3).copy(), b.reshape(H, W, 3).copy())
    mse, mae = np.float32(int(tab[:, 1].sum()) / (3.0 * n)), np.float32(int(tab[:, 2].sum()) / (3.0 * n))
    want = {"psnr": 10 * np.log10(255 * 255 / mse), "mse": float(mse), "rmse": float(np.sqrt(mse)), "mae": float(mae), "max_error": float(plane.max()),
            "pixel_count": n}
    assert got["all_pixels"] == want, dict(case=name, tags=sorted(tags), got=got["all_pixels"], wanted=want)
    hist, edges = np.histogram(plane.astype(np.float32), bins=50)
    assert got["error_histogram"]["bins"] == hist.tolist() and got["error_histogram"]["bin_edges"] == edges.tolist(), dict(case=name, tags=sorted(tags))
    d = got["outlier_detection"]
    assert d["outlier_count"] + d["inlier_count"] == n and got["error_distribution"]["max"] == float(plane.max()) and got["error_distribution"]["min"] == float(plane.min())
    assert got["error_distribution"]["median"] == float(np.median(plane)) and got["error_distribution"]["q99"] == float(np.percentile(plane.astype(np.float32), 99))


# ---- what was measured -------------------------------------------------------------------------------------------------------------------
def test_worst_differences_are_inside_the_bounds():
    """the largest difference, as a share of what is allowed, that each floating-point comparison of this module met in this run
    (printed: run with -s); the figures of an MI355X are in the module's docstring"""
    for key, (diff, allowed, case) in sorted(WORST.items()):
        print(f"worst {key}: {diff:.3e} of {allowed:.3e} allowed ({diff / allowed:.3f}) at {case}")
        assert diff <= allowed, (key, diff, allowed, case)
