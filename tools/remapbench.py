"""The nearest-colour remap (csrc/palette_remap.hip) on the 4K Kodak mosaic of tools/imagebench.py, in ONE process:
  (a) ImageEncoder.encode(image, 20, 10), the full hierarchy                                  wall time, PSNR, .rhccq bytes
  (b) ImageEncoder.encode_with_palette(image, (a)'s palette)                                  wall time, PSNR, .rhccq bytes
  (c) rhccq_palette_remap alone on resident tensors, K = (a)'s palette size, 256, 4096, 65536   HIP events
Medians of --reps runs after a warm-up of every shape; (a) and (b) alternate.  The palettes of (c) other than (a)'s are colours
sampled from the image (seeded).  For each K of (c) the evaluations (pixels x K) and the arithmetic floor: 2.5 vector integer
operations per evaluation (two v_dot4_u32_u8, two v_lshl_add_u32, one v_min3_u32 per two entries) on CUs x 64 lanes at --ghz.

Exits non-zero when (b) is not faster than (a) (the JSON is written all the same).

    python tools/remapbench.py [--reps 5] [--out profiles/palette_remap.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
OPS_PER_EVAL = 2.5


def png(name):
    return np.asarray(Image.open(os.path.join(G, name + ".png")).convert("RGB"), dtype=np.uint8)


def wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ghz", type=float, default=2.4, help="clock of the arithmetic floor (the device's maximum)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from roibasedimagecompression_amd import container, synth
    from roibasedimagecompression_amd.image import ImageEncoder
    from roibasedimagecompression_amd.ops import psnr_from_sse
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh, dev = enc.rh, enc.rh.device
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    key = enc.encode(img, 20, 10)                                           # warm-up of (a)
    pal = np.asarray(key["palette"], np.uint8).reshape(-1, 3)
    enc.encode_with_palette(img, pal)                                       # warm-up of (b)
    ta, tb = [], []
    for _ in range(args.reps):                                              # alternating: both see the same machine state
        dt, key = wall(lambda: enc.encode(img, 20, 10), dev)
        ta.append(dt)
        dt, rem = wall(lambda: enc.encode_with_palette(img, pal), dev)
        tb.append(dt)
    (top, left), (h, w) = key["top_left"], key["shape"]
    rgb = rh.dev(img)
    crop = rgb[top:top + h, left:left + w].contiguous()
    row = rh.class_error_sums_indexed(crop, key["indices"].reshape(-1), rh.dev(pal), rh.zeros((h, w), torch.uint8), 1)[0]
    sse_a = int(row[0]) + int(row[1]) + int(row[2])
    with tempfile.TemporaryDirectory() as tmp:
        sizes = {}
        for name, res in (("encode", key), ("encode_with_palette", rem)):
            for exact in (False, True):
                path = os.path.join(tmp, "x.rhccq")
                container.write_frame(res, path, rh, exact=exact)
                sizes[name + ("_exact" if exact else "")] = os.path.getsize(path)
    out = {"tool": "tools/remapbench.py", "device": torch.cuda.get_device_name(0), "compute_units": cus, "reps": args.reps,
           "image": "kodak_mosaic", "shape": [H, W], "qualities": [20, 10], "palette_size": len(pal),
           "encode": {"median_s": round(statistics.median(ta), 5), "runs_s": [round(v, 5) for v in ta], "window": [top, left, h, w],
                      "sse": sse_a, "psnr": psnr_from_sse(sse_a, h * w)},
           "encode_with_palette": {"median_s": round(statistics.median(tb), 5), "runs_s": [round(v, 5) for v in tb],
                                   "sse": rem["stats"]["remap"]["all"]["sse"], "psnr": rem["stats"]["remap"]["all"]["psnr"],
                                   "stages_s": rem["stats"]["seconds"]},
           "rhccq_bytes": sizes, "kernel": []}
    out["speedup"] = round(out["encode"]["median_s"] / out["encode_with_palette"]["median_s"], 2)

    rng = np.random.default_rng(1)
    flat = img.reshape(-1, 3)
    for K in (len(pal), 256, 4096, 65536):
        p = rh.dev(pal if K == len(pal) else flat[rng.integers(0, len(flat), K)])
        rh.palette_remap(rgb, p)                                            # warm-up of this shape
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, sums = rh.palette_remap(rgb, p)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        evals = H * W * K
        floor_ms = evals * OPS_PER_EVAL / (cus * 64 * args.ghz * 1e9) * 1e3
        med = statistics.median(ms)
        out["kernel"].append({"K": K, "median_ms": round(med, 4), "runs_ms": [round(v, 4) for v in ms], "evaluations": evals,
                              "evaluations_per_s": round(evals / (med * 1e-3), 0), "arithmetic_floor_ms": round(floor_ms, 4),
                              "share_of_floor": round(floor_ms / med, 3), "sse": int(sums[-1, 1].item())})
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if not out["encode_with_palette"]["median_s"] < out["encode"]["median_s"]:
        sys.exit("encode_with_palette is NOT faster than encode: the remap has no purpose on this machine")


if __name__ == "__main__":
    main()
