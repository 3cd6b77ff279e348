"""Shared cases of the quality-metric and block-DCT kernel tests (tests/test_metric_cases_cpu.py, tests/test_gpu_metric_regimes.py):
a plain helper module, not a conftest.  numpy and the standard library only; nothing here calls the device code or
oracle.rhccq_oracle.

csrc/metrics.hip (error_sums_kernel, error_tables_kernel, ssim7_kernel) and csrc/dct_ext.hip (dct_quant_kernel<8|16>, luma_kernel,
qstep_kernel) have separate code paths by input size; a case is (name, tags, inputs) and the tags say which path it is there for.

    error sums      tail0 .. tail3 (n_px & 3), no_quad (n_px < 4), one_group / groups (quads in one workgroup or several),
                    grid_stride (more quads than SUMS_GROUPS_MAX * GROUP lanes), past_2_32 (a channel sum above 2^32), max255,
                    first_only / last_only (one differing pixel), random, identical, hw (n_px = H * W of an SSIM shape)
    error tables    one_group / groups / grid_stride, rows_one / rows_all (table rows populated), row0, row255, worst_r / worst_g /
                    worst_b / ties (which channel holds the worst error), random, hw
    ssim7           tiles<T> (workgroups), last_rows<r> / last_cols<c> (window rows / columns of the last tile row / column),
                    windows<n>, and the contents random, identical, black_white, white_white, checker, flat, apron_pixel
    dct_quant       B8 / B16, tiles<T> (32 x 32 super-tiles), partial (H or W no multiple of SUPER_TILE), the planes const255,
                    impulse0 .. impulse3, checker, signed, luma, and q_int16 (q = 32 640), the steps per_block / eighth

References
    error sums / tables   int64 numpy.
    SSIM   the five window moments are exact integers (int64 integral images).  With C1, C2 and cov_norm the float64 constants of
           the kernel converted exactly (fractions.Fraction) a window's term is a ratio N / D of two integers; it is evaluated as
           floor(N * 2^200 / D), and the terms of a tile are added as integers.  Of the issue's two choices this is the first one
           (exact rational arithmetic), with each term cut to 200 fractional bits: a sum of 1024 Fractions of unrelated 110-bit
           denominators costs a second per tile, the cut costs 2^-200 per term, 44 decimal orders below the bound.  ssim_terms_exact
           keeps the uncut Fractions for the small cases, and the CPU test compares the two.
    DCT    basis[u][x] = s(u) cos(pi (2x+1) u / 2B) at np.longdouble (64-bit mantissa), the argument reduced exactly to the first
           octant in integers; coefficients basis @ block @ basis.T at np.longdouble; q = rint(coef / qstep).

Tolerances (u = 2^-53, gamma_k = k u / (1 - k u), M = 65 025 the largest moment)
    integers   exact equality.
    SSIM   the kernel computes, per window, from exact integer sums: ux = sx/49 (one rounding), ux*uy within gamma_3 M, uxy within
           gamma_1 M, their difference within gamma_5 M (the result is at most M/4), times cov_norm within EV = c gamma_6 M.
           A2 = 2 vxy + C2 and B2 = vx + vy + C2 are then each within E2 = gamma_13 c M + gamma_1 C2 (2 EV, and the roundings of sums
           of at most c M / 2 + C2).  B2 >= C2 and |A2 / B2| <= 1 exactly, so the computed ratio is within R2 = 2 E2 / (C2 - E2) --
           the smallest denominator enters here.  A1 = 2 ux uy + C1 and B1 = ux^2 + uy^2 + C1 are sums of positive terms: relative
           errors gamma_4 and gamma_5, 0 < A1 / B1 <= 1, ratio within gamma_9 relative.  Two products and a quotient add gamma_3:
               SSIM_TERM_BOUND = gamma_3 + (1 + gamma_3) (gamma_9 + (1 + gamma_9) R2)      = 3.3e-12
           A sum of n such terms (each at most 1 + SSIM_TERM_BOUND in size) in any order adds gamma_(n-1) n:
               ssim_partial_bound(n) = n SSIM_TERM_BOUND + gamma_(n-1) n (1 + SSIM_TERM_BOUND)     (3.5e-9 for n = 1024, on a sum of 1024)
               ssim_mean_bound(N) = SSIM_TERM_BOUND + gamma_(N+1) (1 + SSIM_TERM_BOUND)              (3.7e-12 for N = 4096)
           The bound of the mean, and of every partial per window of its tile, is below the 1e-9 that test_quality_metrics_vs_oracle
           grants (asserted below).  For identical images every term is exactly 1.0: 2 ux ux == ux ux + ux ux in floating point and
           vxy, vx, vy are the same expression, so partials equal their window counts and the mean is exactly 1.0.
    DCT coefficients   the basis entries are within gamma_6 relative (cospi 2 ulp = 4u, sqrt, one product; the argument is exact: 2B
           is a power of two).  A pass is a chain of B fma: Sum t_x b_x within gamma_(B+6) T L1, L1 = max_u Sum_x |basis[u][x]| =
           sqrt(B), T = 256 >= every |plane|.  The second pass carries the first's error through L1 again and adds its own:
               DCT_ACC_BOUND[B] = 2 gamma_(B+6) (1 + gamma_(B+6)) T B (1 + 2^-10)      (6.4e-12 at B = 8, 2.0e-11 at B = 16)
           (the last factor: the same formula for the reference, with u = 2^-64).  The kernel rounds the accumulator to float32 once:
               |got - ref| <= 0.5 ulp_float32(|ref|) + 2 DCT_ACC_BOUND[B]
           where the second DCT_ACC_BOUND pays for ulp(acc) > ulp(ref), which needs |ref| < 2^24 DCT_ACC_BOUND or a binade between them.
    quantised integers   exact equality.  acc / qstep is within DCT_ACC_BOUND / qstep + 2u |ref / qstep| of ref / qstep; no case may
           have a ratio that close to a half-integer (dct_guard_count, asserted to be zero by the CPU test).

Cases and references are computed once per process and shared: do not modify what the functions here return."""
import functools
import zlib
from fractions import Fraction

import numpy as np

# ---- the limits, and where they come from ------------------------------------------------------------------------------------------
SSIM_TILE = 32            # kSsimTile (metrics.hip): window centres per workgroup and axis
SSIM_WIN = 7              # kSsimWin (metrics.hip); kSsimPad = 3, kSsimIn = 38
QUAD = 4                  # error_sums_kernel: `const long long n4 = n_px >> 2;`, tail `threadIdx.x < (n_px & 3)`
GROUP = 256               # __launch_bounds__(256) of every kernel of both files
SUMS_GROUPS_MAX = 2048    # rhccq_error_sums: `blocks > 2048 ? 2048 : blocks`, blocks = (n_pixels / 4 + 255) / 256
TABLES_GROUPS_MAX = 2048  # rhccq_error_tables: `blocks = blocks > 2048 ? 2048 : blocks`, blocks = (n_pixels + 255) / 256
LUMA_GROUPS_MAX = 2048    # rhccq_luma_qstep: `if (b > 2048) b = 2048`
SUPER_TILE = 32           # kTile (dct_ext.hip): pixels per workgroup and axis
QSTEP_GROUP = 256         # qstep_kernel: one thread per block, 256 per workgroup

U = 2.0 ** -53
M = 255 * 255
C1 = (0.01 * 255.0) * (0.01 * 255.0)
C2 = (0.03 * 255.0) * (0.03 * 255.0)
COV_NORM = 49.0 / 48.0
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "the DCT reference needs a long double of 64 mantissa bits"


def _gamma(k):
    return Fraction(k, 2 ** 53) / (1 - Fraction(k, 2 ** 53))


def _ssim_term_bound():
    c, c2 = Fraction(COV_NORM), Fraction(C2)
    e2 = _gamma(13) * c * M + _gamma(1) * c2
    r2 = 2 * e2 / (c2 - e2)
    return _gamma(3) + (1 + _gamma(3)) * (_gamma(9) + (1 + _gamma(9)) * r2)


_TERM = _ssim_term_bound()
SSIM_TERM_BOUND = float(_TERM)


def ssim_partial_bound(n):
    """allowed |partial - exact| of a tile of n windows"""
    return float(n * _TERM + _gamma(max(n - 1, 0)) * n * (1 + _TERM))


def ssim_mean_bound(n):
    """allowed |mean - exact| over n windows"""
    return float(_TERM + _gamma(n + 1) * (1 + _TERM))


assert ssim_mean_bound(4096) <= 1e-9 and ssim_partial_bound(SSIM_TILE * SSIM_TILE) / (SSIM_TILE * SSIM_TILE) <= 1e-9

DCT_T = 256.0
DCT_ACC_BOUND = {B: float(2 * _gamma(B + 6) * (1 + _gamma(B + 6)) * 256 * B * (1 + Fraction(1, 1024))) for B in (8, 16)}


def ulp32(x):
    """the spacing of float32 at |x| (x: np.longdouble array)"""
    _, e = np.frexp(np.abs(x))
    e = np.where(x == 0, -200, e)
    return np.ldexp(np.longdouble(1), np.maximum(e - 24, -149))


def dct_tol(ref, B):
    return np.longdouble(0.5) * ulp32(ref) + np.longdouble(2 * DCT_ACC_BOUND[B])


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- error sums ------------------------------------------------------------------------------------------------------------------------
SSIM_SHAPES = ((7, 7), (7, 120), (120, 7), (8, 8), (37, 37), (38, 38), (39, 38), (38, 39), (70, 70), (71, 45), (13, 100))
HW_SHAPES = ((7, 7), (37, 37), (39, 38), (71, 45), (70, 70))            # n_px & 3 = 1, 1, 2, 3, 0
SUMS_GRID_N = 4 * 256 * 2048 + 4 * 300 + 3


def sums_tags(n):
    """the tags that follow from n_px alone: a restatement of rhccq_error_sums' launch"""
    quads = n // QUAD
    return {f"tail{n % QUAD}", "no_quad" if quads == 0 else "one_group" if quads <= GROUP else
            "grid_stride" if quads > GROUP * SUMS_GROUPS_MAX else "groups"}


def _random_pair(name, n):
    r = _rng(name)
    return r.integers(0, 256, (n, 3), dtype=np.uint8), r.integers(0, 256, (n, 3), dtype=np.uint8)


def _one_pixel(name, n, where):
    a = _rng(name).integers(0, 256, (n, 3), dtype=np.uint8)
    b = a.copy()
    b[where] = 255 - a[where]
    return a, b


def _sums_build():
    out = {}
    for n in (1, 2, 3, 4, 5, 6, 7, 1023, 1024, 1025, 1026, 1029):
        out[f"n{n}"] = (sums_tags(n) | {"random"}, functools.partial(_random_pair, f"sums{n}", n))
    out["black_white_grid_stride"] = (sums_tags(SUMS_GRID_N) | {"past_2_32", "max255"},
                                      lambda: (np.zeros((SUMS_GRID_N, 3), np.uint8), np.full((SUMS_GRID_N, 3), 255, np.uint8)))
    out["last_pixel_tail"] = (sums_tags(1027) | {"last_only"}, lambda: _one_pixel("last_t", 1027, -1))
    out["last_pixel_quad"] = (sums_tags(2048) | {"last_only"}, lambda: _one_pixel("last_q", 2048, -1))
    out["first_pixel"] = (sums_tags(1027) | {"first_only"}, lambda: _one_pixel("first", 1027, 0))

    def same():
        a = _rng("same").integers(0, 256, (1030, 3), dtype=np.uint8)
        return a, a.copy()
    out["identical"] = (sums_tags(1030) | {"identical"}, same)
    for h, w in HW_SHAPES:
        out[f"hw_{h}x{w}"] = (sums_tags(h * w) | {"random", "hw"}, functools.partial(_random_pair, f"sums{h}x{w}", h * w))
    return out


SUMS = _sums_build()
SUMS_TAGS = ("tail0", "tail1", "tail2", "tail3", "no_quad", "one_group", "groups", "grid_stride", "past_2_32", "max255", "last_only",
             "first_only", "random", "identical", "hw")


def hw_shape(name):
    """(H, W) of a `hw` case"""
    h, w = name.split("_")[-1].split("x")
    return int(h), int(w)


@functools.lru_cache(maxsize=None)
def sums_case(name):
    """-> (tags, a uint8[n, 3], b uint8[n, 3])"""
    tags, make = SUMS[name]
    return (frozenset(tags),) + tuple(_frozen(*make()))


def error_sums_reference(a, b):
    """int64[5]: the sum of squared differences of R, G, B, the sum of |d|, max |d|"""
    d = np.abs(a.reshape(-1, 3).astype(np.int64) - b.reshape(-1, 3).astype(np.int64))
    return np.array([*(d * d).sum(axis=0), d.sum(), d.max()], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def sums_reference(name):
    _, a, b = sums_case(name)
    return _frozen(error_sums_reference(a, b))


# ---- error tables ------------------------------------------------------------------------------------------------------------------------
TABLES_GRID_N = 256 * 2048 + 1


def tables_tags(n):
    return {"one_group" if n <= GROUP else "grid_stride" if n > GROUP * TABLES_GROUPS_MAX else "groups"}


def _every_error():
    """worst error i % 256 in channel i % 3, the other channels anything up to it"""
    n = 700
    r = _rng("every")
    a = np.zeros((n, 3), np.uint8)
    e = np.arange(n) % 256
    b = (r.integers(0, 256, (n, 3)) % (e[:, None] + 1)).astype(np.uint8)
    b[np.arange(n), np.arange(n) % 3] = e
    flip = r.random(n) < 0.5                               # the sign of the difference must not matter
    a[flip], b[flip] = b[flip], 0
    return a, b


def _worst_channel():
    """pixel i: worst error in channel i % 3; (i // 3) % 4 = 0: alone, 1: tied with the next channel, 2: with the previous, 3: all"""
    n = 600
    r = _rng("worst")
    e = r.integers(1, 256, n)
    d = (r.integers(0, 256, (n, 3)) % e[:, None])          # strictly below the worst error
    i = np.arange(n)
    d[i, i % 3] = e
    kind = (i // 3) % 4
    d[i, (i + 1) % 3] = np.where((kind == 1) | (kind == 3), e, d[i, (i + 1) % 3])
    d[i, (i + 2) % 3] = np.where((kind == 2) | (kind == 3), e, d[i, (i + 2) % 3])
    a, b = np.zeros((n, 3), np.uint8), d.astype(np.uint8)
    flip = r.random(n) < 0.5
    a[flip], b[flip] = b[flip], 0
    return a, b


def _tables_build():
    out = {}
    for n in (1, 255, 256, 257):
        out[f"n{n}"] = (tables_tags(n) | {"random"}, functools.partial(_random_pair, f"tab{n}", n))
    out["grid_stride"] = (tables_tags(TABLES_GRID_N) | {"random"}, functools.partial(_random_pair, "tabgrid", TABLES_GRID_N))
    out["every_error"] = (tables_tags(700) | {"rows_all"}, _every_error)
    out["row0"] = (tables_tags(3000) | {"rows_one", "row0"}, lambda: (np.full((3000, 3), 77, np.uint8), np.full((3000, 3), 77, np.uint8)))
    out["row255"] = (tables_tags(3000) | {"rows_one", "row255"}, lambda: (np.full((3000, 3), 255, np.uint8), np.zeros((3000, 3), np.uint8)))
    out["worst_channel"] = (tables_tags(600) | {"worst_r", "worst_g", "worst_b", "ties"}, _worst_channel)
    for h, w in HW_SHAPES:
        out[f"hw_{h}x{w}"] = (tables_tags(h * w) | {"random", "hw"}, functools.partial(_random_pair, f"tab{h}x{w}", h * w))
    return out


TABLES = _tables_build()
TABLES_TAGS = ("one_group", "groups", "grid_stride", "rows_one", "rows_all", "row0", "row255", "worst_r", "worst_g", "worst_b", "ties",
               "random", "hw")


@functools.lru_cache(maxsize=None)
def tables_case(name):
    """-> (tags, a uint8[n, 3], b uint8[n, 3])"""
    tags, make = TABLES[name]
    return (frozenset(tags),) + tuple(_frozen(*make()))


def error_tables_reference(a, b):
    """(int64[256][3]: pixels, sum of squared differences, sum of |differences| by worst-channel error; uint8[n] worst errors)"""
    d = np.abs(a.reshape(-1, 3).astype(np.int64) - b.reshape(-1, 3).astype(np.int64))
    e = d.max(axis=1)
    tab = np.zeros((256, 3), np.int64)
    np.add.at(tab[:, 0], e, 1)
    np.add.at(tab[:, 1], e, (d * d).sum(axis=1))
    np.add.at(tab[:, 2], e, d.sum(axis=1))
    return tab, e.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def tables_reference(name):
    _, a, b = tables_case(name)
    return _frozen(*error_tables_reference(a, b))


# ---- ssim7 -------------------------------------------------------------------------------------------------------------------------------
SSIM_CONTENTS = ("random", "identical", "black_white", "white_white", "checker", "flat", "apron_pixel")


def ssim_grid(h, w):
    """(tile rows, tile columns, window rows of the last tile row, window columns of the last tile column)"""
    ih, iw = h - (SSIM_WIN - 1), w - (SSIM_WIN - 1)
    ty, tx = -(-ih // SSIM_TILE), -(-iw // SSIM_TILE)
    return ty, tx, ih - (ty - 1) * SSIM_TILE, iw - (tx - 1) * SSIM_TILE


def ssim_tags(h, w):
    ty, tx, lr, lc = ssim_grid(h, w)
    return {f"tiles{ty * tx}", f"last_rows{lr}", f"last_cols{lc}", f"windows{(h - 6) * (w - 6)}"}


def _ssim_pair(content, h, w):
    r = _rng(f"ssim_{content}_{h}x{w}")
    a = r.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "random":
        b = r.integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif content == "identical":
        b = a.copy()
    elif content == "black_white":
        a, b = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    elif content == "white_white":
        a, b = np.full((h, w, 3), 255, np.uint8), np.full((h, w, 3), 255, np.uint8)
    elif content == "checker":
        a = np.broadcast_to((255 * ((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1)).astype(np.uint8)[..., None], (h, w, 3)).copy()
        b = 255 - a
    elif content == "flat":                                  # a patch flat in both, around it a flat in one and noise in the other
        b = np.clip(a.astype(np.int64) + r.integers(-40, 41, a.shape), 0, 255).astype(np.uint8)
        ph, pw = max(SSIM_WIN, h // 2), max(SSIM_WIN, w // 2)
        a[:ph, :pw] = (17, 200, 255)
        b[:ph, :pw // 2 + SSIM_WIN // 2 + 1] = (90, 200, 0)
    else:                                                    # apron_pixel: only the last window reaches the differing pixel
        b = a.copy()
        b[h - 1, w - 1] = 255 - a[h - 1, w - 1]
    return a, b


SSIM = {f"{c}_{h}x{w}": (ssim_tags(h, w) | {c}, (c, h, w)) for h, w in SSIM_SHAPES for c in SSIM_CONTENTS}
SSIM_SMALL = tuple(n for n, (_, (c, h, w)) in SSIM.items() if (h - 6) * (w - 6) <= 4)        # the uncut Fractions are compared here


@functools.lru_cache(maxsize=None)
def ssim_case(name):
    """-> (tags, a uint8[H, W, 3], b uint8[H, W, 3])"""
    tags, spec = SSIM[name]
    return (frozenset(tags),) + tuple(_frozen(*_ssim_pair(*spec)))


def _win7(x):
    """int64[H, W, 3] -> the sums over every full 7 x 7 window, int64[H - 6, W - 6, 3], by an integral image"""
    h, w = x.shape[:2]
    c = np.zeros((h + 1, w + 1, 3), np.int64)
    c[1:, 1:] = x.cumsum(axis=0).cumsum(axis=1)
    k = SSIM_WIN
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def ssim_moments(a, b):
    """the exact window sums (sx, sy, sxx, syy, sxy), each int64[H - 6, W - 6, 3]"""
    x, y = a.astype(np.int64), b.astype(np.int64)
    return _win7(x), _win7(y), _win7(x * x), _win7(y * y), _win7(x * y)


SSIM_FRAC_BITS = 200
_SH = max(Fraction(v).denominator for v in (C1, C2, COV_NORM)).bit_length() - 1
_K1, _K2, _CN = (int(f * 2 ** _SH) for f in (2401 * Fraction(C1), 2401 * Fraction(C2), Fraction(COV_NORM)))
assert Fraction(_K1, 2 ** _SH) == 2401 * Fraction(C1) and Fraction(_K2, 2 ** _SH) == 2401 * Fraction(C2) and Fraction(_CN, 2 ** _SH) == Fraction(COV_NORM)


def _term_ratio(sx, sy, sxx, syy, sxy):
    """a window's S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) as two integers (numerator, denominator): every
    factor is multiplied by 49^2 2^_SH, which cancels"""
    a1 = ((2 * sx * sy) << _SH) + _K1
    b1 = ((sx * sx + sy * sy) << _SH) + _K1
    a2 = 2 * _CN * (49 * sxy - sx * sy) + _K2
    b2 = _CN * (49 * sxx - sx * sx) + _CN * (49 * syy - sy * sy) + _K2
    return a1 * a2, b1 * b2


@functools.lru_cache(maxsize=None)
def ssim_reference(name):
    """-> (partial, count, total): partial[ty][tx][ch] the sum of S over the tile's windows as an integer scaled by 2^SSIM_FRAC_BITS
    (every term floor'ed there), count[ty][tx] its windows, total[ch] the sum of the partials"""
    _, a, b = ssim_case(name)
    mom = [m.tolist() for m in ssim_moments(a, b)]
    ih, iw = a.shape[0] - 6, a.shape[1] - 6
    ty, tx, _, _ = ssim_grid(*a.shape[:2])
    partial = [[[0, 0, 0] for _ in range(tx)] for _ in range(ty)]
    count = np.zeros((ty, tx), np.int64)
    for r in range(ih):
        for c in range(iw):
            p = partial[r // SSIM_TILE][c // SSIM_TILE]
            count[r // SSIM_TILE, c // SSIM_TILE] += 1
            for ch in range(3):
                num, den = _term_ratio(*(m[r][c][ch] for m in mom))
                p[ch] += (num << SSIM_FRAC_BITS) // den
    total = [sum(partial[i][j][ch] for i in range(ty) for j in range(tx)) for ch in range(3)]
    return partial, _frozen(count), total


def ssim_terms_exact(name):
    """the uncut terms: Fraction[H - 6][W - 6][3]"""
    _, a, b = ssim_case(name)
    mom = [m.tolist() for m in ssim_moments(a, b)]
    return [[[Fraction(*_term_ratio(*(m[r][c][ch] for m in mom))) for ch in range(3)] for c in range(a.shape[1] - 6)] for r in range(a.shape[0] - 6)]


def ssim_diff(got, fixed, scale=1):
    """|got - fixed / (2^SSIM_FRAC_BITS scale)| of a float64 and a reference integer, exactly, as a float"""
    return float(abs(Fraction(float(got)) - Fraction(fixed, scale << SSIM_FRAC_BITS)))


def ssim_float64(a, b):
    """the kernel's formula in plain numpy float64, the terms of a tile added one after the other in raster order (not the kernel's
    order) -> (partial float64[ty, tx, 3], mean float64[3], the terms float64[H - 6, W - 6, 3])"""
    sx, sy, sxx, syy, sxy = (m.astype(np.float64) for m in ssim_moments(a, b))
    ux, uy, uxx, uyy, uxy = sx / 49.0, sy / 49.0, sxx / 49.0, syy / 49.0, sxy / 49.0
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    s = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    ty, tx, _, _ = ssim_grid(*a.shape[:2])
    partial = np.zeros((ty, tx, 3))
    for i in range(ty):
        for j in range(tx):
            t = s[i * SSIM_TILE:(i + 1) * SSIM_TILE, j * SSIM_TILE:(j + 1) * SSIM_TILE].reshape(-1, 3)
            partial[i, j] = np.cumsum(t, axis=0)[-1]
    return partial, np.cumsum(partial.reshape(-1, 3), axis=0)[-1] / float(s.shape[0] * s.shape[1]), s


# ---- dct_quant ---------------------------------------------------------------------------------------------------------------------------
DCT_SHAPES = {8: ((8, 8), (8, 40), (40, 8), (24, 72), (32, 32), (48, 80)), 16: ((16, 16), (16, 48), (48, 16), (32, 32), (80, 112))}
DCT_PLANES = ("const255", "impulse0", "impulse1", "impulse2", "impulse3", "checker", "signed", "luma")


def luma_f32(rgb):
    """luma_kernel's float32 statement"""
    r, g, b = (rgb[..., i].astype(np.float32) for i in range(3))
    return (np.float32(0.299) * r + np.float32(0.587) * g) + np.float32(0.114) * b


def dct_tags(B, h, w):
    tiles = -(-h // SUPER_TILE) * -(-w // SUPER_TILE)
    return {f"B{B}", f"tiles{tiles}"} | ({"partial"} if h % SUPER_TILE or w % SUPER_TILE else set())


def _dct_plane(kind, B, h, w):
    r = _rng(f"dct_{kind}_{B}_{h}x{w}")
    if kind == "const255":
        return np.full((h, w), 255, np.float32)
    if kind.startswith("impulse"):                           # block i: 255 at corner (i + k) % 4 of the block, 0 elsewhere
        p = np.zeros((h, w), np.float32)
        for i, (by, bx) in enumerate((y, x) for y in range(h // B) for x in range(w // B)):
            cy, cx = divmod((i + int(kind[-1])) % 4, 2)
            p[by * B + cy * (B - 1), bx * B + cx * (B - 1)] = 255
        return p
    if kind == "checker":
        return (255 * ((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1)).astype(np.float32)
    luma = luma_f32(r.integers(0, 256, (h, w, 3), dtype=np.uint8))
    return luma - np.float32(128) if kind == "signed" else luma


def step_map(B, h, w):
    """a step that differs in every block: (13 + 6 i) / 16 at block i, exact in float32.  The numerator is odd, so the rational
    coefficients of the constant and impulse planes (255 B, 255 / B) never divide to a half-integer"""
    return (0.8125 + 0.375 * np.arange((h // B) * (w // B))).astype(np.float32).reshape(h // B, w // B)


def _dct_build():
    out = {}
    for B, shapes in DCT_SHAPES.items():
        for h, w in shapes:
            for kind in DCT_PLANES:
                out[f"{kind}_b{B}_{h}x{w}"] = (dct_tags(B, h, w) | {kind, "per_block"}, (kind, B, h, w, None))
    for h, w in ((16, 16), (80, 112)):
        out[f"const255_eighth_b16_{h}x{w}"] = (dct_tags(16, h, w) | {"const255", "eighth", "q_int16"}, ("const255", 16, h, w, 0.125))
    return out


DCT = _dct_build()
DCT_TAGS = ("B8", "B16", "partial", "per_block", "eighth", "q_int16") + DCT_PLANES


@functools.lru_cache(maxsize=None)
def dct_case(name):
    """-> (tags, B, plane float32[H, W], qstep float32[H / B, W / B])"""
    tags, (kind, B, h, w, step) = DCT[name]
    q = step_map(B, h, w) if step is None else np.full((h // B, w // B), step, np.float32)
    return (frozenset(tags), B) + tuple(_frozen(_dct_plane(kind, B, h, w), q))


@functools.lru_cache(maxsize=None)
def dct_basis(B):
    """basis[u][x] = s(u) cos(pi (2x+1) u / 2B), np.longdouble[B, B]; the argument pi k / N, N = 2B, k = (2x+1) u mod 2N, is folded
    into [0, pi/4] in integers before anything is rounded"""
    ld = np.longdouble
    pi = 4 * np.arctan(ld(1))
    N = 2 * B
    out = np.zeros((B, B), ld)
    for u in range(B):
        s = np.sqrt(ld(1) / B) if u == 0 else np.sqrt(ld(2) / B)
        for x in range(B):
            k = ((2 * x + 1) * u) % (2 * N)
            if k > N:
                k = 2 * N - k                                # cos(2 pi - t) = cos t
            sign = 1
            if 2 * k > N:
                sign, k = -1, N - k                          # cos(pi - t) = -cos t
            v = np.cos(pi * k / N) if 4 * k <= N else np.sin(pi * (N - 2 * k) / (2 * N))
            out[u, x] = sign * s * v
    return _frozen(out)


def _blocks(plane, B):
    h, w = plane.shape
    return plane.reshape(h // B, B, w // B, B).transpose(0, 2, 1, 3)


def _unblocks(blk):
    nby, nbx, B, _ = blk.shape
    return blk.transpose(0, 2, 1, 3).reshape(nby * B, nbx * B)


def dct_quant_reference(plane, B, qstep):
    """-> (coef np.longdouble[H, W], ratio = coef / qstep np.longdouble[H, W], q int64[H, W] = rint(ratio))"""
    bm = dct_basis(B)
    coef = _unblocks(np.matmul(np.matmul(bm, _blocks(plane.astype(np.longdouble), B)), bm.T))
    ratio = coef / np.repeat(np.repeat(qstep.astype(np.longdouble), B, axis=0), B, axis=1)
    return coef, ratio, np.rint(ratio).astype(np.int64)


@functools.lru_cache(maxsize=None)
def dct_reference(name):
    _, B, plane, qstep = dct_case(name)
    return _frozen(*dct_quant_reference(plane, B, qstep))


def dct_guard_count(name):
    """coefficients whose coef / qstep lies within the rounding error of the kernel's ratio of a half-integer"""
    _, B, plane, qstep = dct_case(name)
    _, ratio, _ = dct_reference(name)
    guard = DCT_ACC_BOUND[B] / np.repeat(np.repeat(qstep.astype(np.longdouble), B, axis=0), B, axis=1) + 2 * U * np.abs(ratio)
    return int((np.abs(np.abs(ratio - np.floor(ratio)) - 0.5) <= guard).sum())


def dct_float64(plane, B):
    """the separable transform in plain numpy float64 (basis rounded once from the long double one; numpy's dot order, no fma),
    rounded to float32 as the kernel rounds"""
    bm = dct_basis(B).astype(np.float64)
    return _unblocks(np.matmul(np.matmul(bm, _blocks(plane.astype(np.float64), B)), bm.T)).astype(np.float32)


# ---- luma_qstep --------------------------------------------------------------------------------------------------------------------------
LUMA_SHAPE = (528, 1000)      # 528 000 pixels > LUMA_GROUPS_MAX * GROUP: grid-stride; 66 x 125 blocks of 8 > QSTEP_GROUP


def corner_mask(B, h, w):
    """uint8[H, W]: one ROI pixel in a corner of some blocks -- block i of every 3rd block has it in corner (i // 3) % 4 -- and always in
    the outer corner of the four corner blocks"""
    m = np.zeros((h, w), np.uint8)
    nbx = w // B
    for i in range(0, (h // B) * nbx, 3):
        if i // nbx in (0, h // B - 1) and i % nbx in (0, nbx - 1):
            continue
        cy, cx = divmod((i // 3) % 4, 2)
        m[(i // nbx) * B + cy * (B - 1), (i % nbx) * B + cx * (B - 1)] = 1 + i % 255          # any non-zero value counts
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = 1
    return m


LUMA_QSTEP = {"grid_stride_b8": (8,) + LUMA_SHAPE, "b16_32x48": (16, 32, 48), "b8_16x40": (8, 16, 40)}


@functools.lru_cache(maxsize=None)
def luma_case(name):
    """-> (B, rgb uint8[H, W, 3], roi uint8[H, W])"""
    B, h, w = LUMA_QSTEP[name]
    return (B,) + tuple(_frozen(_rng(f"luma_{name}").integers(0, 256, (h, w, 3), dtype=np.uint8), corner_mask(B, h, w)))


def qstep_reference(roi, B, q_roi, q_bg):
    h, w = roi.shape
    return np.where(roi.reshape(h // B, B, w // B, B).max(axis=(1, 3)) > 0, np.float32(q_roi), np.float32(q_bg)).astype(np.float32)
