"""The run-carrying remap (csrc/palette_runs.hip) on the 4K Kodak mosaic of tools/imagebench.py, in ONE process, the frame resident:
  (a) rhccq_palette_runs (remap + memset + row walk) against rhccq_palette_remap alone, K = the encoder's palette, 256, 1024, 4096, and
      at the encoder's palette for every RHCCQ_OPT_RUNS_ROWS setting (image rows a one-wave workgroup walks).  HIP events around
      --inner calls, the two alternating; medians of --reps windows after a warm-up of every shape.
  (b) exact .rhccq bytes (container.frame_bytes(exact=True)) and PSNR of encode_with_palette for run_slack in {off, 0, 32, 64, 128, 256}
      x colours in {all, 128, 64}, beside the colours-only rungs recorded in profiles/palette_reduce.json.
  (c) the equal-bytes question: for every slack on the full palette, the colours-only rung a byte-target search finds for the SAME
      number of bytes (encode_with_palette(target_bytes=those bytes)), and the PSNR difference.

    python tools/runsbench.py [--reps 5] [--inner 20] [--out profiles/palette_runs.json]"""
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
SLACKS = (0, 32, 64, 128, 256)
KERNEL_SLACK = 128


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


def ab(rh, rgb, pal, reps, inner):
    """remap alone and the whole run-carrying call, alternating -> (remap row, runs row, carried pixels)"""
    rh.palette_remap(rgb, pal)
    _, sums = rh.palette_runs(rgb, pal, KERNEL_SLACK)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window_ms(lambda: rh.palette_remap(rgb, pal), inner))
        tb.append(window_ms(lambda: rh.palette_runs(rgb, pal, KERNEL_SLACK), inner))
    row = lambda t: {"median_ms": round(statistics.median(t), 4), "runs_ms": [round(v, 4) for v in t]}  # noqa: E731
    return row(ta), row(tb), int(sums[-1, 2].item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "palette_runs.json"))
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
    rows_default, cols = ops.palette_runs_tile()
    out = {"tool": "tools/runsbench.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "reps": args.reps, "inner_calls": args.inner,
           "image": "kodak_mosaic", "shape": [H, W], "qualities": [20, 10], "palette_size": len(pal),
           "inputs": "resident device tensors (the frame is uploaded once before the timed loops); output buffers are allocated inside the calls",
           "tile": {"rows_default": rows_default, "cols": cols}, "kernel_slack": KERNEL_SLACK, "kernel": [], "rows_per_workgroup": []}

    # ---- (a) the call against the remap alone
    rng = np.random.default_rng(1)
    flat = img.reshape(-1, 3)
    for K in (len(pal), 256, 1024, 4096):
        p = rh.dev(pal if K == len(pal) else flat[rng.integers(0, len(flat), K)])
        remap, runs, carried = ab(rh, rgb, p, args.reps, args.inner)
        out["kernel"].append({"K": K, "remap": remap, "palette_runs": runs, "scan_ms": round(runs["median_ms"] - remap["median_ms"], 4),
                              "runs_over_remap": round(runs["median_ms"] / remap["median_ms"], 3), "carried": carried})
    p = rh.dev(pal)
    for rows in (2, 4, 8):
        rh.set_option(rh.OPT_RUNS_ROWS, rows)
        remap, runs, _ = ab(rh, rgb, p, args.reps, args.inner)
        out["rows_per_workgroup"].append({"rows": rows, "workgroups": -(-H // rows), "remap": remap, "palette_runs": runs,
                                          "scan_ms": round(runs["median_ms"] - remap["median_ms"], 4)})
    rh.set_option(rh.OPT_RUNS_ROWS, 0)

    # ---- (b) bytes and PSNR: slack x colours
    def point(colours, slack, **kw):
        res = enc.encode_with_palette(rgb, p, colours=colours, run_slack=slack, **kw)
        st = res["stats"]
        return res, {"colours": len(res["palette"]), "run_slack": slack, "rhccq_bytes_exact": len(container.frame_bytes(res, rh, exact=True)),
                     "psnr": st["remap"]["all"]["psnr"], "sse": st["remap"]["all"]["sse"],
                     "carried": st["runs"]["carried"]["all"] if "runs" in st else None}
    grid = []
    for colours in (None, 128, 64):
        for slack in (None,) + SLACKS:
            grid.append(point(colours, slack)[1])
    out["grid"] = grid
    try:
        with open(os.path.join(ROOT, "profiles", "palette_reduce.json")) as f:
            out["colours_only_rungs_recorded"] = [{"colours": r["colours"], "refine": r["refine"], "psnr": r["psnr"], "rhccq_bytes_exact": r["rhccq_bytes_exact"]}
                                                  for r in json.load(f)["ladder"]]
    except (OSError, KeyError):
        out["colours_only_rungs_recorded"] = None

    # ---- (c) equal bytes: the slack on the full palette against the colours-only rung of no more bytes
    equal = []
    for g in grid:
        if g["colours"] != len(pal) or g["run_slack"] in (None, 0):
            continue
        res = enc.encode_with_palette(rgb, p, target_bytes=g["rhccq_bytes_exact"], exact=True)
        tg = res["stats"]["target"]
        equal.append({"run_slack": g["run_slack"], "rhccq_bytes_exact": g["rhccq_bytes_exact"], "psnr": g["psnr"],
                      "colours_only": {"colours": tg["colours"], "met": tg["met"], "rhccq_bytes_exact": dict(map(tuple, tg["probes"]))[tg["colours"]],
                                       "psnr": res["stats"]["remap"]["all"]["psnr"]},
                      "advantage_db": round(g["psnr"] - res["stats"]["remap"]["all"]["psnr"], 4)})
    out["equal_bytes"] = equal
    out["equal_bytes_advantage_reproduced"] = bool(equal) and all(e["advantage_db"] > 0 for e in equal)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
