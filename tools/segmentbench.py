"""The exact row segmentation (csrc/palette_segment.hip) on the 4K Kodak mosaic of tools/imagebench.py, in ONE process, the frame resident:
  (a) rhccq_palette_segment (remap + memset + the row launch; the workspace allocated by the call) beside rhccq_palette_remap and
      rhccq_palette_runs, K = the encoder's palette, 256, 1024.  HIP events around --inner calls, the three alternating; medians of --reps
      windows after a warm-up of every shape.
  (b) exact .rhccq bytes (container.frame_bytes(exact=True)) and PSNR of encode_with_palette for run_penalty in {32, 64, 128, 256, 512}
      x colours in {all, 128, 64}, beside run_slack of the same value.
  (c) the equal-bytes question: for every penalty on the full palette, the smallest greedy run_slack whose file has no more bytes
      (bisection on the integer slack), its PSNR, and the segmentation's advantage in dB.

    python tools/segmentbench.py [--reps 5] [--inner 20] [--out profiles/palette_segment.json]"""
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
PENALTIES = (32, 64, 128, 256, 512)
KERNEL_PENALTY = 128


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


def abc(rh, rgb, pal, reps, inner):
    """remap alone, the greedy run-carrying call and the segmentation, alternating -> (three rows, the segmentation's sums)"""
    fns = (lambda: rh.palette_remap(rgb, pal), lambda: rh.palette_runs(rgb, pal, KERNEL_PENALTY), lambda: rh.palette_segment(rgb, pal, KERNEL_PENALTY))
    for fn in fns:
        fn()
    _, sums = rh.palette_segment(rgb, pal, KERNEL_PENALTY)
    t = [[], [], []]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t[i].append(window_ms(fn, inner))
    row = lambda v: {"median_ms": round(statistics.median(v), 4), "runs_ms": [round(x, 4) for x in v]}  # noqa: E731
    return [row(v) for v in t], [int(x) for x in sums[-1].tolist()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "palette_segment.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import _lib, container, ops, synth
    from roibasedimagecompression_amd.image import ImageEncoder
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh, dev = enc.rh, enc.rh.device
    key = enc.encode(img, 20, 10)
    pal = np.asarray(key["palette"], np.uint8).reshape(-1, 3)
    rgb = rh.dev(img)                                                        # the resident frame of every timed call below
    out = {"tool": "tools/segmentbench.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "reps": args.reps, "inner_calls": args.inner,
           "image": "kodak_mosaic", "shape": [H, W], "qualities": [20, 10], "palette_size": len(pal),
           "inputs": "resident device tensors (the frame is uploaded once before the timed loops); output buffers and the segmentation's "
                     "workspace are allocated inside the calls (torch's caching allocator)",
           "tile_cols": ops.palette_segment_tile(), "max_rows": ops.palette_segment_max_rows(), "kernel_penalty": KERNEL_PENALTY, "kernel": []}

    # ---- (a) the call beside the remap and the greedy call
    rng = np.random.default_rng(1)
    flat = img.reshape(-1, 3)
    for K in (len(pal), 256, 1024):
        p = rh.dev(pal if K == len(pal) else flat[rng.integers(0, len(flat), K)])
        (remap, runs, seg), sums = abc(rh, rgb, p, args.reps, args.inner)
        out["kernel"].append({"K": K, "workspace_bytes": int(_lib.load().rhccq_palette_segment_bytes(H, W, K)), "remap": remap, "palette_runs": runs,
                              "palette_segment": seg, "segment_over_remap": round(seg["median_ms"] / remap["median_ms"], 3),
                              "segment_over_runs": round(seg["median_ms"] / runs["median_ms"], 3),
                              "sums": dict(zip(("pixels", "sse", "not_nearest", "breaks"), sums))})
    p = rh.dev(pal)

    # ---- (b) bytes and PSNR: penalty x colours, beside the slack of the same value
    def point(colours, **kw):
        res = enc.encode_with_palette(rgb, p, colours=colours, **kw)
        st = res["stats"]
        row = {"colours": len(res["palette"]), "rhccq_bytes_exact": len(container.frame_bytes(res, rh, exact=True)),
               "psnr": st["remap"]["all"]["psnr"], "sse": st["remap"]["all"]["sse"]}
        if "runs" in st:
            row["carried"] = st["runs"]["carried"]["all"]
            if "breaks" in st["runs"]:
                row["breaks"] = st["runs"]["breaks"]["all"]
        return row
    grid = []
    for colours in (None, 128, 64):
        grid.append(dict(point(colours), value=None))
        for v in PENALTIES:
            seg, greedy = point(colours, run_penalty=v), point(colours, run_slack=v)
            grid.append({"value": v, "colours": seg["colours"], "run_penalty": seg, "run_slack": greedy,
                         "bytes_ratio": round(seg["rhccq_bytes_exact"] / greedy["rhccq_bytes_exact"], 4),
                         "psnr_gain_db": round(seg["psnr"] - greedy["psnr"], 4)})
    out["grid"] = grid

    # ---- (c) equal bytes: the smallest greedy slack whose file is no larger than the segmentation's
    equal = []
    for g in grid:
        if g["value"] is None or g["colours"] != len(pal):
            continue
        target = g["run_penalty"]["rhccq_bytes_exact"]
        lo, hi, probes = g["value"], ops.RUN_SLACK_MAX, 0                   # (the greedy file at the same value is larger, or the answer is that slack)
        best = None
        if g["run_slack"]["rhccq_bytes_exact"] <= target:
            best, lo, hi = (g["value"], g["run_slack"]), 0, g["value"]
        while best is None or hi - lo > 1:
            if best is None:
                mid = min(hi, max(lo + 1, 2 * lo))                             # gallop up to the first slack that fits
            else:
                mid = (lo + hi) // 2
            row = point(None, run_slack=mid)
            probes += 1
            if row["rhccq_bytes_exact"] <= target:
                best, hi = (mid, row), mid
            else:
                lo = mid
                if best is None and mid == hi:
                    break
        e = {"run_penalty": g["value"], "rhccq_bytes_exact": target, "psnr": g["run_penalty"]["psnr"], "probes": probes}
        if best is not None:
            e.update(greedy_slack=best[0], greedy=best[1], advantage_db=round(g["run_penalty"]["psnr"] - best[1]["psnr"], 4))
        equal.append(e)
    out["equal_bytes"] = equal
    out["equal_bytes_advantage_reproduced"] = bool(equal) and all(e.get("advantage_db", 0) > 0 for e in equal)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
