"""The candidate-grid search (csrc/palette_grid.hip) against the full search (csrc/palette_remap.hip) on the 4K Kodak mosaic of
tools/imagebench.py, in ONE process on a resident frame.  For K = 230 (ImageEncoder.quantize), 256, 1024 (quantize) and 4096, 16384,
65536 (rows drawn from the frame's unique colours, seeded): the grid's build time (Rhccq.palette_grid with the capacity known, HIP
events around the three launches), the remap through the grid and through the full search (HIP events, alternating, medians of --reps
after a warm-up of each), the pixel-weighted mean and the longest list, the entries used, flagged cells and overflow pixels, and from
those: the frames after which build + remaps through the grid beat the full search.

Exits non-zero when indices or sums differ at any K (the JSON is written all the same).

    python tools/gridbench.py [--reps 5] [--out profiles/palette_grid.json]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")


def png(name):
    return np.asarray(Image.open(os.path.join(G, name + ".png")).convert("RGB"), dtype=np.uint8)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from roibasedimagecompression_amd import synth
    from roibasedimagecompression_amd.image import ImageEncoder
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh = enc.rh
    rgb = rh.dev(img)
    packed = np.unique(img.reshape(-1, 3).astype(np.uint32) @ np.array([65536, 256, 1], np.uint32))
    unique = np.stack([packed >> 16, (packed >> 8) & 255, packed & 255], axis=1).astype(np.uint8)
    rng = np.random.default_rng(1)
    out = {"tool": "tools/gridbench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "image": "kodak_mosaic", "shape": [H, W],
           "unique_colours": len(unique), "rows": []}
    equal = True
    for K, source in ((230, "quantize"), (256, "quantize"), (1024, "quantize"), (4096, "unique"), (16384, "unique"), (65536, "unique")):
        if source == "quantize":
            pal = rh.dev(np.asarray(enc.quantize(img, colours=K)["palette"], np.uint8).reshape(-1, 3))
        else:
            pal = rh.dev(unique[rng.choice(len(unique), K, replace=False)])
        grid = rh.palette_grid(pal)                                         # sizes itself; also the warm-up of the build
        work = rh.zeros((grid.work.numel(),), torch.uint8)
        stats = rh.empty((4,), torch.int64)
        rh.palette_remap(rgb, pal)
        rh.palette_remap(rgb, pal, grid=grid)
        tb, tg, tf = [], [], []
        for _ in range(args.reps):                                          # alternating: all three see the same machine state
            tb.append(timed(lambda: rh._check(rh.lib.rhccq_palette_grid(rh.ctx, rh._p(pal), len(pal), grid.entries, rh._p(work), work.numel(),
                                                                        rh._p(stats)), "palette_grid"))[0])
            dt, (gi, gs) = timed(lambda: rh.palette_remap(rgb, pal, grid=grid))
            tg.append(dt)
            dt, (fi, fs) = timed(lambda: rh.palette_remap(rgb, pal))
            tf.append(dt)
        same = bool(torch.equal(gi, fi) and torch.equal(gs, fs) and torch.equal(work, grid.work))
        equal = equal and same
        cells = grid.work[:262144].view(torch.int32).reshape(-1, 2)[:, 1].to(torch.int64)
        px = rgb.reshape(-1, 3).to(torch.int64)
        per_px = cells[(px[:, 0] >> 3) << 10 | (px[:, 1] >> 3) << 5 | px[:, 2] >> 3]
        b, g, f = statistics.median(tb), statistics.median(tg), statistics.median(tf)
        out["rows"].append({"K": len(pal), "palette": source, "equal": same, "build": spread(tb), "remap_grid": spread(tg), "remap_full": spread(tf),
                            "remap_speedup": round(f / g, 2), "frames_to_amortise_build": math.ceil(b / (f - g)) if f > g else None,
                            "mean_list_per_pixel": round(float(per_px[per_px > 0].to(torch.float64).mean().item()), 2), **grid.stats,
                            "overflow_pixels": int(grid.overflow.item())})
        print(json.dumps(out["rows"][-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    if not equal:
        sys.exit("the grid search and the full search DIFFER")


if __name__ == "__main__":
    main()
