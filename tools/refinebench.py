"""The palette refinement (csrc/palette_refine.hip) on the 4K Kodak mosaic of tools/remapbench.py, in ONE process:
  (a) ImageEncoder.encode(image, 20, 10), the full hierarchy                                  wall time, PSNR, .rhccq bytes
  (b) ImageEncoder.encode_with_palette(image, (a)'s palette)                                  wall time, PSNR, .rhccq bytes
  (c) the same with refine = 1, 2, 4, 8, 16                                                   wall time, PSNR, .rhccq bytes, iterations run
  (d) ONE refinement iteration (the assign and update kernels) against rhccq_palette_remap alone on resident tensors (HIP events),
      K = (a)'s palette size, 256, lds_rows, lds_rows + 1, 4096, 65536; on the mosaic and on a one-colour frame of the same size
      (every add of a wave, and of the frame, goes to ONE row: the worst case for same-row adds); with the default options and with
      OPT_REFINE_LDS_ROWS = 0 (accumulators in global memory at every K).
Medians of --reps runs after a warm-up of every shape; compared variants alternate.  The frame is uploaded ONCE before the timed loop:
(b) and (c) take the resident device tensor, so their times hold no host-to-device copy ((a) takes the host image, as encode's
region stage wants it; tools/remapbench.py times (b) from the host image instead).  The palettes of (d) other than (a)'s are colours
sampled from the mosaic (seeded).  (d)'s "iteration" is Rhccq.palette_refine(max_iter=1): the two kernels AND the copy of the palette,
three memsets, three allocations and the binding, so its ratio to the remap is an upper bound for the kernels (the record says so).

Exits non-zero (the JSON is written all the same) when any (c) has a lower PSNR than (b) -- the refinement cannot raise the error,
so that is a bug -- or when any run of (c, refine = 8) is not faster than every run of (a): a refinement must be cheaper than the
re-encode it stands in for.  The ratios of (d) are reported, not gated.

    python tools/refinebench.py [--reps 5] [--out profiles/palette_refine.json]"""
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
REFINES = (1, 2, 4, 8, 16)


def png(name):
    return np.asarray(Image.open(os.path.join(G, name + ".png")).convert("RGB"), dtype=np.uint8)


def wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from roibasedimagecompression_amd import container, ops, synth
    from roibasedimagecompression_amd.image import ImageEncoder
    from roibasedimagecompression_amd.ops import psnr_from_sse
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh, dev = enc.rh, enc.rh.device
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    L = ops.palette_refine_lds_rows()

    rgb = rh.dev(img)                                                       # resident: (b), (c) and (d) read this tensor
    key = enc.encode(img, 20, 10)                                           # warm-up of every shape
    pal = np.asarray(key["palette"], np.uint8).reshape(-1, 3)
    enc.encode_with_palette(rgb, pal)
    for n in REFINES:
        enc.encode_with_palette(rgb, pal, refine=n)
    ta, tb, tc = [], [], {n: [] for n in REFINES}
    rc = {}
    for _ in range(args.reps):                                              # alternating: all see the same machine state
        dt, key = wall(lambda: enc.encode(img, 20, 10), dev)
        ta.append(dt)
        dt, rem = wall(lambda: enc.encode_with_palette(rgb, pal), dev)
        tb.append(dt)
        for n in REFINES:
            dt, rc[n] = wall(lambda: enc.encode_with_palette(rgb, pal, refine=n), dev)
            tc[n].append(dt)
    (top, left), (h, w) = key["top_left"], key["shape"]
    crop = rgb[top:top + h, left:left + w].contiguous()
    row = rh.class_error_sums_indexed(crop, key["indices"].reshape(-1), rh.dev(pal), rh.zeros((h, w), torch.uint8), 1)[0]
    sse_a = int(row[0]) + int(row[1]) + int(row[2])

    def size(res):
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "x.rhccq")
            container.write_frame(res, path, rh, exact=True)
            return os.path.getsize(path)

    def runs(ts):
        return {"median_s": round(statistics.median(ts), 5), "runs_s": [round(v, 5) for v in ts]}
    out = {"tool": "tools/refinebench.py", "device": torch.cuda.get_device_name(0), "compute_units": cus, "reps": args.reps,
           "image": "kodak_mosaic", "shape": [H, W], "qualities": [20, 10], "palette_size": len(pal), "lds_rows": L,
           "inputs": {"encode": "host image", "encode_with_palette": "resident device tensor (uploaded once before the timed loop)",
                      "refine": "resident device tensor", "iteration": "resident device tensors"},
           "iteration_includes": "Rhccq.palette_refine(max_iter=1): assign + update kernels, the palette copy, three memsets, three "
                                 "allocations and the Python binding; the ratios to the remap are upper bounds for the kernels",
           "encode": dict(runs(ta), window=[top, left, h, w], sse=sse_a, psnr=psnr_from_sse(sse_a, h * w), rhccq_bytes_exact=size(key)),
           "encode_with_palette": dict(runs(tb), sse=rem["stats"]["remap"]["all"]["sse"], psnr=rem["stats"]["remap"]["all"]["psnr"],
                                       rhccq_bytes_exact=size(rem)),
           "refine": [], "iteration": []}
    for n in REFINES:
        st = rc[n]["stats"]
        out["refine"].append(dict(runs(tc[n]), refine=n, iterations=st["refine"]["iterations"], converged=st["refine"]["converged"],
                                  sse=st["remap"]["all"]["sse"], psnr=st["remap"]["all"]["psnr"], weighted_sse=st["refine"]["sse"],
                                  changed=st["refine"]["changed"], rhccq_bytes_exact=size(rc[n])))

    # (d) one iteration against the remap alone
    rng = np.random.default_rng(1)
    flat = img.reshape(-1, 3)
    one_colour = rh.dev(np.broadcast_to(flat[len(flat) // 2], img.shape).copy())
    for K in (len(pal), 256, L, L + 1, 4096, 65536):
        p = rh.dev(pal if K == len(pal) else flat[rng.integers(0, len(flat), K)])
        for frame_name, frame in (("mosaic", rgb), ("one_colour", one_colour)):
            rec = {"K": K, "frame": frame_name}
            variants = (("remap", None), ("iteration", L), ("iteration_global", 0))
            ms = {v: [] for v, _ in variants}
            for rep in range(args.reps + 1):                                # (rep 0: the warm-up of this shape)
                for v, lds in variants:
                    if lds is None:
                        dt = events(lambda: rh.palette_remap(frame, p))
                    else:
                        rh.set_option(rh.OPT_REFINE_LDS_ROWS, lds)
                        try:
                            dt = events(lambda: rh.palette_refine(frame, p, max_iter=1))
                        finally:
                            rh.set_option(rh.OPT_REFINE_LDS_ROWS, L)
                    if rep:
                        ms[v].append(dt)
            for v, _ in variants:
                rec[v + "_ms"] = round(statistics.median(ms[v]), 4)
                rec[v + "_runs_ms"] = [round(x, 4) for x in ms[v]]
            rec["accumulators"] = "lds" if K <= L else "global"
            rec["iteration_over_remap"] = round(rec["iteration_ms"] / rec["remap_ms"], 3)
            rec["iteration_global_over_remap"] = round(rec["iteration_global_ms"] / rec["remap_ms"], 3)
            out["iteration"].append(rec)

    failures = []
    for r in out["refine"]:
        if r["psnr"] < out["encode_with_palette"]["psnr"]:
            failures.append(f"refine={r['refine']} has a lower PSNR ({r['psnr']}) than the plain remap ({out['encode_with_palette']['psnr']})")
    r8 = next(r for r in out["refine"] if r["refine"] == 8)
    if not max(r8["runs_s"]) < min(out["encode"]["runs_s"]):
        failures.append(f"refine=8 (slowest run {max(r8['runs_s'])} s) is not faster than every encode (fastest run {min(out['encode']['runs_s'])} s)")
    out["failures"] = failures
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if failures:
        sys.exit("; ".join(failures))


if __name__ == "__main__":
    main()
