"""decoder/uncompression/comparison.py:30-80 on the device: `calculate_quality_metrics` with the reference's keys
and numpy scalar types.  The other names of that module (image loading through OpenCV, matplotlib reports) stay
with the reference.

Arithmetic: the error statistics come from exact integer sums (the reference averages float32 arrays with
numpy's pairwise float32 summation: its `mse`, `mae`, `mse_r/g/b` agree to float32 rounding, ~1e-7 relative);
`psnr` is scikit-image's float64 `10*log10(255^2 / mse)`; `ssim` is scikit-image's
structural_similarity(data_range=255, channel_axis=2, win_size=7) from exact integer window sums."""
import math

import numpy as np
import torch

from .. import ops

_RH = None


def _rh():
    global _RH
    if _RH is None:
        _RH = ops.Rhccq(0)
    return _RH


def calculate_quality_metrics(original, reconstructed):
    """Same keys as the reference: psnr, ssim, mse, rmse, mae, max_error, mse_r, mse_g, mse_b."""
    rh = _rh()
    original = np.ascontiguousarray(original)
    reconstructed = np.ascontiguousarray(reconstructed)
    if original.shape != reconstructed.shape or original.ndim != 3 or original.shape[2] != 3:
        raise ValueError("Input images must have the same dimensions.")      # skimage's check_shape_equality
    if original.dtype != np.uint8 or reconstructed.dtype != np.uint8:
        raise TypeError("calculate_quality_metrics: uint8 RGB images expected (what cv2.imread yields)")
    a, b = torch.from_numpy(original).to(rh.device), torch.from_numpy(reconstructed).to(rh.device)
    return metrics_from_device(rh, a, b)


def metrics_from_device(rh, a, b):
    """a, b: uint8[H,W,3] device tensors."""
    H, W = int(a.shape[0]), int(a.shape[1])
    s = rh.error_sums(a, b).astype(np.int64)
    n_ch = H * W
    sq = int(s[0]) + int(s[1]) + int(s[2])
    mse64 = sq / (3.0 * n_ch)
    m = {}
    with np.errstate(divide="ignore"):
        m["psnr"] = np.float64(10.0) * np.log10(np.float64(255.0 ** 2) / np.float64(mse64))
    try:
        m["ssim"] = np.float64(rh.ssim7(a, b).mean())
    except ValueError:
        m["ssim"] = np.float64(0.0)                      # the reference's fallback for images a 7x7 window does not fit
    m["mse"] = np.float32(mse64)
    m["rmse"] = np.sqrt(m["mse"])
    m["mae"] = np.float32(int(s[3]) / (3.0 * n_ch))
    m["max_error"] = np.float32(int(s[4]))
    for i, ch in enumerate("rgb"):
        m[f"mse_{ch}"] = np.float32(int(s[i]) / float(n_ch))
    return m


# ---- EXTENSION (no reference counterpart; not re-exported by the mirrored decoder/uncompression/comparison.py): the same metrics
# per class of a class map, e.g. inside and outside the ROI -------------------------------------------------------------------------
def _metrics_row(row, ssim_sum, ssim_count):
    """one entry of the per-class dict from an integer row {sum d^2 R, G, B, sum |d|, max |d|, pixels} and the sums of S per
    channel over `ssim_count` window centres: metrics_from_device's arithmetic and scalar types"""
    n_ch = int(row[5])
    if n_ch == 0:
        return None
    sq = int(row[0]) + int(row[1]) + int(row[2])
    mse64 = sq / (3.0 * n_ch)
    m = {}
    with np.errstate(divide="ignore"):
        m["psnr"] = np.float64(10.0) * np.log10(np.float64(255.0 ** 2) / np.float64(mse64))
    m["ssim"] = np.float64((np.asarray(ssim_sum, np.float64) / float(ssim_count)).mean()) if ssim_count else None
    m["mse"] = np.float32(mse64)
    m["rmse"] = np.sqrt(m["mse"])
    m["mae"] = np.float32(int(row[3]) / (3.0 * n_ch))
    m["max_error"] = np.float32(int(row[4]))
    for i, ch in enumerate("rgb"):
        m[f"mse_{ch}"] = np.float32(int(row[i]) / float(n_ch))
    m["pixel_count"] = n_ch
    return m


def region_metrics_from_sums(sums, ssim_sums, names):
    """Pure host arithmetic.  sums: integer [len(names), 6] rows of Rhccq.class_error_sums; ssim_sums: Rhccq.class_ssim7's (float64
    [len(names), 3], int [len(names)]) or None when no 7x7 window fits the image -> {name: metrics, ..., "all": metrics}.  An entry
    has calculate_quality_metrics' keys, scalar types and arithmetic plus `pixel_count`; a class without pixels is None, a class (or
    image) without a window centre has ssim None.  "all" comes from the column sums of the rows (max |d| folded with max)."""
    sums = np.asarray(sums).astype(np.int64).reshape(-1, 6)
    names = list(names)
    if len(names) != len(sums) or "all" in names or len(set(names)) != len(names):
        raise ValueError("region_metrics_from_sums: one distinct name per row of sums is expected, none of them 'all'")
    if ssim_sums is None:
        s_sum, s_cnt = np.zeros((len(names), 3)), np.zeros(len(names), np.int64)
    else:
        s_sum, s_cnt = np.asarray(ssim_sums[0], np.float64).reshape(-1, 3), np.asarray(ssim_sums[1]).astype(np.int64).reshape(-1)
        if len(s_sum) != len(names) or len(s_cnt) != len(names):
            raise ValueError("region_metrics_from_sums: ssim_sums must have one row per name")
    out = {name: _metrics_row(sums[k], s_sum[k], int(s_cnt[k])) for k, name in enumerate(names)}
    total = [int(v) for v in sums.sum(axis=0)]
    total[4] = int(sums[:, 4].max())
    out["all"] = _metrics_row(total, s_sum.sum(axis=0), int(s_cnt.sum()))
    return out


def region_metrics_from_device(rh, a, b, cls, names=("nonroi", "roi")):
    """a, b: uint8[H,W,3] device tensors, cls: uint8 / bool [H,W] device tensor with class k = names[k] (a value >= len(names)
    keeps the pixel out of every class).  Two device passes; only the len(names) x 6 sums and the SSIM partials come back."""
    n = len(names)
    return region_metrics_from_sums(rh.class_error_sums(a, b, cls, n), rh.class_ssim7(a, b, cls, n), names)


def _class_map_u8(class_map, shape):
    class_map = np.asarray(class_map)
    if class_map.dtype == np.bool_:
        class_map = class_map.view(np.uint8)
    if class_map.dtype != np.uint8:
        raise TypeError("class map: bool or uint8 expected")
    if class_map.ndim != 2 or tuple(class_map.shape) != tuple(shape):
        raise ValueError("class map: an H x W array of the image's height and width is expected")
    return np.ascontiguousarray(class_map)


def calculate_region_quality_metrics(original, reconstructed, class_map, names=("nonroi", "roi")):
    """calculate_quality_metrics per class: numpy uint8 RGB images and a bool / uint8 [H,W] class map in, the dict of
    region_metrics_from_sums out.  With the 0 / 1 region map of the ROI stage: quality outside and inside the ROI."""
    rh = _rh()
    original = np.ascontiguousarray(original)
    reconstructed = np.ascontiguousarray(reconstructed)
    if original.shape != reconstructed.shape or original.ndim != 3 or original.shape[2] != 3:
        raise ValueError("Input images must have the same dimensions.")
    if original.dtype != np.uint8 or reconstructed.dtype != np.uint8:
        raise TypeError("calculate_region_quality_metrics: uint8 RGB images expected")
    class_map = _class_map_u8(class_map, original.shape[:2])
    a, b = torch.from_numpy(original).to(rh.device), torch.from_numpy(reconstructed).to(rh.device)
    return region_metrics_from_device(rh, a, b, torch.from_numpy(class_map).to(rh.device), names)


def calculate_adaptive_quality_metrics(original, reconstructed):
    """comparison.py:345-536: quality metrics with adaptive outlier exclusion, same keys and nesting as the reference.

    Every statistic of the reference is a function of the per-pixel worst-channel error (an integer 0..255) and of sums over
    pixel subsets defined by thresholds on it, so one device pass builds a 256-row table (pixels, squared differences,
    absolute differences per error value) and the rest is the reference's own arithmetic on that table: the percentiles
    come from numpy on the (sorted) multiset of error values, the mean / std from the table in float64, rounded to float32
    -- they may differ from the reference's raster-order float32 pairwise sums in the last bits --, the subset MSE / MAE are exact integer sums
    (the reference averages float32 arrays: agreement to ~1e-7 relative), SSIM is the device kernel of
    calculate_quality_metrics (scikit-image's algorithm, parity unpinned), the masked SSIM greys the outliers on the device."""
    rh = _rh()
    original = np.ascontiguousarray(original)
    reconstructed = np.ascontiguousarray(reconstructed)
    if original.shape != reconstructed.shape or original.ndim != 3 or original.shape[2] != 3:
        raise ValueError("Input images must have the same dimensions.")
    if original.dtype != np.uint8 or reconstructed.dtype != np.uint8:
        raise TypeError("calculate_adaptive_quality_metrics: uint8 RGB images expected")
    a, b = torch.from_numpy(original).to(rh.device), torch.from_numpy(reconstructed).to(rh.device)
    tab, d_maxerr = rh.error_tables(a, b, want_maxerr=True)
    cnt, sq, ab = tab[:, 0], tab[:, 1], tab[:, 2]
    n = int(cnt.sum())
    err = np.repeat(np.arange(256, dtype=np.float32), cnt)             # max_error_per_pixel, sorted
    # mean / std from the exact table in float64, rounded to float32 once: numpy's float32 pairwise sums over the SORTED 4K multiset
    # drift 5e-6 relative from the exact std (1.9861755 for 1.9861647; the reference's raster-order float32 sum gives 1.9861636)
    values = np.arange(256, dtype=np.float64)
    mean64 = float(np.dot(values, cnt)) / n
    std64 = math.sqrt(float(np.dot((values - mean64) ** 2, cnt)) / n)
    stats = {"min": float(np.min(err)), "max": float(np.max(err)), "mean": float(np.float32(mean64)), "median": float(np.median(err)),
             "std": float(np.float32(std64)), "q75": float(np.percentile(err, 75)), "q90": float(np.percentile(err, 90)),
             "q95": float(np.percentile(err, 95)), "q99": float(np.percentile(err, 99))}
    q1, q3 = np.percentile(err, 25), np.percentile(err, 75)
    iqr_threshold = q3 + 2.5 * (q3 - q1)
    z_threshold = 3.0
    percentile_threshold = np.percentile(err, 99)
    if stats["mean"] > stats["median"] * 1.5:
        adaptive_threshold = stats["median"] + 3 * stats["std"]
    else:
        adaptive_threshold = stats["mean"] + 2.5 * stats["std"]
    values = np.arange(256, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (values - np.float32(stats["mean"])) / np.float32(stats["std"])
    masks = {"iqr": values > iqr_threshold, "zscore": np.abs(z) > z_threshold, "percentile": values > percentile_threshold,
             "adaptive": values > adaptive_threshold}                    # per error VALUE: which values are outliers
    best_method, best = None, None
    for name, mk in masks.items():
        pct = int(cnt[mk].sum()) / n * 100
        if 0.1 <= pct <= 10.0:
            best_method, best = name, mk
            break
    if best_method is None:
        best_method, best = "adaptive", masks["adaptive"]
    outlier_count = int(cnt[best].sum())
    outlier_pct = outlier_count / n * 100
    metrics = {"error_distribution": stats,
               "outlier_detection": {"method": best_method,
                                     "threshold": float({"iqr": iqr_threshold, "zscore": stats["mean"] + z_threshold * stats["std"],
                                                         "percentile": percentile_threshold, "adaptive": adaptive_threshold}[best_method]),
                                     "outlier_count": outlier_count, "outlier_percentage": float(outlier_pct),
                                     "inlier_count": int(n - outlier_count), "inlier_percentage": float(100 - outlier_pct)}}

    def subset(mk):
        c = int(cnt[mk].sum())
        mse = np.float32(int(sq[mk].sum()) / (3.0 * c))
        return c, mse, np.float32(int(ab[mk].sum()) / (3.0 * c))

    def psnr(mse):
        return 10 * np.log10(255 * 255 / mse) if mse > 0 else float("inf")
    c_all, mse_all, mae_all = subset(np.ones(256, bool))
    metrics["all_pixels"] = {"psnr": psnr(mse_all), "mse": float(mse_all), "rmse": float(np.sqrt(mse_all)), "mae": float(mae_all),
                             "max_error": stats["max"], "pixel_count": n}
    if 0 < outlier_count < n:
        c_in, mse_in, mae_in = subset(~best)
        metrics["without_outliers"] = {"psnr": psnr(mse_in), "mse": float(mse_in), "rmse": float(np.sqrt(mse_in)), "mae": float(mae_in),
                                       "max_error": float(np.max(values[~best & (cnt > 0)])), "pixel_count": c_in}
    for percentile in (99, 95, 90, 75):
        threshold = np.percentile(err, percentile)
        mk = values <= threshold
        c_p, mse_p, _ = subset(mk)
        if c_p > 0:
            metrics[f"percentile_{percentile}"] = {"psnr": psnr(mse_p), "mse": float(mse_p), "max_error_included": float(threshold),
                                                   "pixel_count": c_p, "percentage": float(percentile)}
    try:
        metrics["ssim"] = {"full": float(rh.ssim7(a, b).mean())}
        if 0 < outlier_count < n:
            out2d = torch.from_numpy(best).to(rh.device)[d_maxerr.long()]          # outlier mask per pixel
            grey = torch.full_like(a, 128)
            am, bm = torch.where(out2d[..., None], grey, a).contiguous(), torch.where(out2d[..., None], grey, b).contiguous()
            metrics["ssim"]["without_outliers"] = float(rh.ssim7(am, bm).mean())
    except ValueError:
        metrics["ssim"] = {"full": 0}
    present = cnt > 0
    hist, edges = np.histogram(values[present], bins=50, weights=cnt[present])    # same bin edges as over the per-pixel array
    metrics["error_histogram"] = {"bins": [int(v) for v in hist], "bin_edges": edges.tolist()}
    return metrics
