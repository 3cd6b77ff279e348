"""Error diffusion onto a palette (csrc/palette_dither.hip) on the 4K Kodak mosaic of tools/imagebench.py, in ONE process, the frame
resident:
  (a) rhccq_palette_dither (remap + memsets + the wavefront launch, strength 256) against rhccq_palette_remap alone, at K = the encoder's
      palette, 256, 1024 and 4096, for every RHCCQ_OPT_DITHER_ROWS setting (image rows of a band).  HIP events around --inner calls, the
      two alternating; medians of --reps windows after a warm-up of every shape.
  (b) exact .rhccq bytes (container.frame_bytes(exact=True)), PSNR and the error of the 8 x 8 block means of encode_with_palette at
      dither = 0 / 128 / 256 on the encoder's palette, and of colours = 32 and 64 with and without dither = 256.

    python tools/ditherbench.py [--reps 5] [--inner 5] [--out profiles/palette_dither.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
ROWS = (4, 8, 16, 32)
KERNEL_STRENGTH = 256


def png(name):
    return np.asarray(Image.open(os.path.join(G, name + ".png")).convert("RGB"), dtype=np.uint8)


def window_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def block_mean_error(img, pal, idx):
    """the mean squared difference of the non-overlapping 8 x 8 block means of the picture and of its reconstruction"""
    h, w = img.shape[0] // 8 * 8, img.shape[1] // 8 * 8

    def means(a):
        return a[:h, :w].reshape(h // 8, 8, w // 8, 8, 3).astype(np.float64).mean(axis=(1, 3))
    return float(((means(img) - means(pal[idx])) ** 2).mean())


def ab(rh, rgb, pal, reps, inner):
    """remap alone and the whole dither call, alternating -> (remap row, dither row, moved pixels)"""
    rh.palette_remap(rgb, pal)
    _, sums = rh.palette_dither(rgb, pal, KERNEL_STRENGTH)                   # (checks the status word)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window_ms(lambda: rh.palette_remap(rgb, pal), inner))
        tb.append(window_ms(lambda: rh.palette_dither(rgb, pal, KERNEL_STRENGTH, with_status=True), inner))
    row = lambda t: {"median_ms": round(statistics.median(t), 4), "runs_ms": [round(v, 4) for v in t]}  # noqa: E731
    return row(ta), row(tb), int(sums[-1, 2].item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "palette_dither.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import container, ops, synth
    from roibasedimagecompression_amd.image import ImageEncoder
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh, dev = enc.rh, enc.rh.device
    key = enc.encode(img, 20, 10)
    pal = np.asarray(key["palette"], np.uint8).reshape(-1, 3)
    rgb = rh.dev(img)                                                        # the resident frame of every timed call below
    out = {"tool": "tools/ditherbench.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "reps": args.reps, "inner_calls": args.inner,
           "image": "kodak_mosaic", "shape": [H, W], "qualities": [20, 10], "palette_size": len(pal),
           "inputs": "resident device tensors (the frame is uploaded once before the timed loops); output buffers and the workspace are allocated inside the calls",
           "rows_default": ops.palette_dither_rows(), "kernel_strength": KERNEL_STRENGTH, "kernel": []}

    # ---- (a) the call against the remap alone, for every band height
    rng = np.random.default_rng(1)
    flat = img.reshape(-1, 3)
    try:
        for K in (len(pal), 256, 1024, 4096):
            p = rh.dev(pal if K == len(pal) else flat[rng.integers(0, len(flat), K)])
            for rows in ROWS:
                rh.set_option(rh.OPT_DITHER_ROWS, rows)
                remap, dither, moved = ab(rh, rgb, p, args.reps, args.inner)
                out["kernel"].append({"K": K, "rows": rows, "bands": -(-H // rows), "remap": remap, "palette_dither": dither,
                                      "wavefront_ms": round(dither["median_ms"] - remap["median_ms"], 4),
                                      "dither_over_remap": round(dither["median_ms"] / remap["median_ms"], 2), "moved": moved})
                print(json.dumps(out["kernel"][-1]), flush=True)
    finally:
        rh.set_option(rh.OPT_DITHER_ROWS, 0)
    for K in sorted({k["K"] for k in out["kernel"]}):
        rows = [k for k in out["kernel"] if k["K"] == K]
        out.setdefault("best_rows", {})[str(K)] = min(rows, key=lambda k: k["palette_dither"]["median_ms"])["rows"]

    # ---- (b) bytes, PSNR and block means: strength on the encoder's palette; the low rungs with and without dither
    p = rh.dev(pal)

    def point(colours, dither):
        res = enc.encode_with_palette(rgb, p, colours=colours, dither=dither)
        st = res["stats"]
        rpal = np.asarray(res["palette"], np.uint8).reshape(-1, 3)
        idx = res["indices"].cpu().numpy()
        idx = idx.view(np.uint16) if idx.dtype == np.int16 else idx
        return {"colours": len(rpal), "dither": dither, "rhccq_bytes_exact": len(container.frame_bytes(res, rh, exact=True)),
                "psnr": round(st["remap"]["all"]["psnr"], 4), "sse": st["remap"]["all"]["sse"],
                "block_mean_error": round(block_mean_error(img, rpal, idx.astype(np.int64)), 4),
                "moved": st["dither"]["moved"]["all"] if "dither" in st else None}
    out["strength"] = [point(None, s) for s in (None, 0, 128, 256)]
    out["low_rungs"] = [point(c, d) for c in (32, 64) for d in (None, 256)]
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
