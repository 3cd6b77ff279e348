"""Per-class quality metrics and the caller's ROI mask on the 4K Kodak mosaic of tools/imagebench.py: the class kernels
(csrc/region_metrics.hip) against the unchanged whole-picture kernels of the same build (csrc/metrics.hip), and what the report and
the mask cost or save in ImageEncoder.encode.

    python tools/regionquality.py [--reps 5] [--out profiles/region_quality.json]
Kernel rows: device events around `inner` back-to-back calls, median of `reps` after a warm-up.  Encode rows: host clock around a
call that ends in a device synchronise, median of `reps`.  Bytes are the algorithmic ones."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")


def png(name):
    return np.asarray(Image.open(os.path.join(G, name + ".png")).convert("RGB"), dtype=np.uint8)


def kernel_ms(fn, reps, inner):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return statistics.median(out)


def wall_s(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from roibasedimagecompression_amd import synth
    from roibasedimagecompression_amd.image import ImageEncoder
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    n = H * W
    enc = ImageEncoder()
    rh = enc.rh
    res = enc.encode(img, 20, 10)
    region_map = enc.region_map.clone()                                   # the detector's own 0 / 1 map: the mask of the mask rows
    a = torch.from_numpy(img).to(rh.device)
    pal = rh.dev(np.asarray(res["palette"], np.uint8).reshape(-1, 3))
    idx = res["indices"].reshape(-1).contiguous()
    b = rh.decode(idx, pal).reshape(H, W, 3)
    cls16 = (torch.arange(n, device=rh.device, dtype=torch.int32) % 16).to(torch.uint8).reshape(H, W)
    L = rh.lib
    P = rh._p
    s5 = rh.empty((5,), torch.int64)
    s = rh.empty((16, 6), torch.int64)
    nb = int(L.rhccq_ssim7_blocks(H, W))
    part, cpart = rh.empty((nb, 3), torch.float64), rh.empty((nb, 16, 4), torch.float64)
    eb = idx.element_size()
    rows = {}

    def row(name, fn, bytes_px, parent=None):
        ms = kernel_ms(fn, args.reps, args.inner)
        rows[name] = {"ms": round(ms, 4), "bytes_per_px": bytes_px, "gb_s": round(bytes_px * n / ms / 1e6, 1)}
        if parent:
            rows[name]["vs_" + parent] = round(ms / rows[parent]["ms"], 3)
        print(name, json.dumps(rows[name]), flush=True)

    row("rhccq_error_sums", lambda: L.rhccq_error_sums(rh.ctx, P(a), P(b), n, P(s5)), 6)
    row("rhccq_class_error_sums_2", lambda: L.rhccq_class_error_sums(rh.ctx, P(a), P(b), P(region_map), n, 2, P(s)), 7, "rhccq_error_sums")
    row("rhccq_class_error_sums_indexed_2", lambda: L.rhccq_class_error_sums_indexed(rh.ctx, P(a), P(idx), eb, P(pal), pal.shape[0], P(region_map),
                                                                                      n, 2, P(s)), 4 + eb, "rhccq_error_sums")
    row("rhccq_class_error_sums_16", lambda: L.rhccq_class_error_sums(rh.ctx, P(a), P(b), P(cls16), n, 16, P(s)), 7, "rhccq_error_sums")
    row("rhccq_decode", lambda: rh.decode(idx, pal), eb + 3)
    row("rhccq_ssim7_sums", lambda: L.rhccq_ssim7_sums(rh.ctx, P(a), P(b), H, W, P(part), nb), 6)
    row("rhccq_class_ssim7_sums_2", lambda: L.rhccq_class_ssim7_sums(rh.ctx, P(a), P(b), P(region_map), H, W, 2, P(cpart), nb), 7, "rhccq_ssim7_sums")
    row("rhccq_class_ssim7_sums_16", lambda: L.rhccq_class_ssim7_sums(rh.ctx, P(a), P(b), P(cls16), H, W, 16, P(cpart), nb), 7, "rhccq_ssim7_sums")
    # the two forms give the same rows, and the rows add up to the whole-picture sums (a run that measures wrong results is void)
    plain, indexed = rh.class_error_sums(a, b, region_map, 2), rh.class_error_sums_indexed(a, idx, pal, region_map, 2)
    whole = rh.error_sums(a, b)
    assert np.array_equal(plain, indexed) and np.array_equal(plain[:, :4].sum(axis=0), whole[:4]) and plain[:, 4].max() == whole[4]
    mask = region_map.cpu().numpy()
    enc_rows = {}
    for name, fn in (("encode_detector", lambda: enc.encode(img, 20, 10)),
                     ("encode_detector_report", lambda: enc.encode(img, 20, 10, report=True)),
                     ("encode_mask", lambda: enc.encode(img, 20, 10, roi_mask=mask)),
                     ("encode_mask_report", lambda: enc.encode(img, 20, 10, roi_mask=mask, report=True)),
                     ("regions_detector", lambda: enc.regions(img)),
                     ("regions_mask", lambda: enc.regions(img, roi_mask=mask))):
        enc_rows[name] = round(wall_s(fn, args.reps), 4)
        print(name, enc_rows[name], flush=True)
    q = enc.encode(img, 20, 10, report=True)["stats"]
    quality = {k: (None if v is None else {m: (None if x is None else (x if isinstance(x, int) else float(x))) for m, x in v.items()}) for k, v in q["quality"].items()}
    out = {"tool": "tools/regionquality.py", "device": torch.cuda.get_device_name(0), "image": "kodak mosaic", "shape": [H, W], "reps": args.reps,
           "inner": args.inner, "index_bytes": eb, "palette": int(pal.shape[0]), "roi_fraction": float(mask.mean()), "kernels_ms": rows,
           "encode_s": enc_rows, "report_stage_s": q["seconds"].get("report"), "quality": quality}
    print(json.dumps(out["quality"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
