"""The palette reduction (csrc/palette_reduce.hip) on the 4K Kodak mosaic of tools/remapbench.py, in ONE process:
  (a) ImageEncoder.encode(image, 20, 10), the full hierarchy                                  wall time, PSNR, .rhccq bytes
  (b) ImageEncoder.encode_with_palette(image, (a)'s palette, colours=N, refine=R)             wall time, PSNR, .rhccq bytes
      for N = 256 (if the palette has more rows), 128, 64, 32 and R = 0, 4: the quality ladder one full encode gives
  (c) rhccq_palette_reduce alone on resident tensors (HIP events around the three launches, buffers allocated before), K = 256, 1024
      and the device cap, down to K / 2, down to 16, and down to K (no merge: the row state, the table of nearest partners and an
      empty chain); microseconds per merge step = (time - time of no merge) / steps.  The palettes are colours sampled from the
      mosaic (seeded), the counts the histogram of the mosaic's remap onto them (+ 1, so that every row lives).
Medians of --reps runs after a warm-up of every shape; compared variants alternate.  The frame is uploaded ONCE before the timed loop:
(b) and (c) take resident device tensors, (a) takes the host image, as encode's region stage wants it.

Exits non-zero (the JSON is written all the same) when, at the same R, a rung with fewer colours has a higher PSNR or a file that is
not smaller than the rung above it: either would mean the ladder does not trade size for quality.  The times are reported, not gated.

    python tools/reducebench.py [--reps 5] [--out profiles/palette_reduce.json]"""
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
COLOURS = (256, 128, 64, 32)
REFINES = (0, 4)


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
    cap = ops.palette_reduce_max_rows()

    rgb = rh.dev(img)                                                       # resident: (b) and (c) read this tensor
    key = enc.encode(img, 20, 10)                                           # warm-up of every shape
    pal = np.asarray(key["palette"], np.uint8).reshape(-1, 3)
    rungs = [(n, r) for n in COLOURS if n < len(pal) for r in REFINES]
    for n, r in rungs:
        enc.encode_with_palette(rgb, pal, colours=n, refine=r)
    ta, tb, rb = [], {k: [] for k in rungs}, {}
    for _ in range(args.reps):                                              # alternating: all see the same machine state
        dt, key = wall(lambda: enc.encode(img, 20, 10), dev)
        ta.append(dt)
        for n, r in rungs:
            dt, rb[(n, r)] = wall(lambda: enc.encode_with_palette(rgb, pal, colours=n, refine=r), dev)
            tb[(n, r)].append(dt)
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
    plain = enc.encode_with_palette(rgb, pal)
    out = {"tool": "tools/reducebench.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "reps": args.reps, "image": "kodak_mosaic",
           "shape": [H, W], "qualities": [20, 10], "palette_size": len(pal), "max_rows": cap,
           "inputs": {"encode": "host image", "ladder": "resident device tensor (uploaded once before the timed loop)",
                      "kernel": "resident device tensors, buffers allocated before the timed calls"},
           "encode": dict(runs(ta), window=[top, left, h, w], sse=sse_a, psnr=psnr_from_sse(sse_a, h * w), rhccq_bytes_exact=size(key)),
           "encode_with_palette": {"sse": plain["stats"]["remap"]["all"]["sse"], "psnr": plain["stats"]["remap"]["all"]["psnr"],
                                   "rhccq_bytes_exact": size(plain), "indices_dtype": plain["indices_dtype"]},
           "ladder": [], "kernel": []}
    for n, r in rungs:
        st = rb[(n, r)]["stats"]
        out["ladder"].append(dict(runs(tb[(n, r)]), colours=n, refine=r, reduce=st["reduce"], sse=st["remap"]["all"]["sse"],
                                  psnr=st["remap"]["all"]["psnr"], indices_dtype=rb[(n, r)]["indices_dtype"],
                                  rhccq_bytes_exact=size(rb[(n, r)])))

    # (c) the three launches alone
    rng = np.random.default_rng(1)
    flat = img.reshape(-1, 3)
    for K in (256, 1024, cap):
        p = rh.dev(flat[rng.integers(0, len(flat), K)])
        counts = (container.index_histogram(rh.palette_remap(rgb, p)[0], K, rh) + 1).contiguous()
        wbytes = int(rh._raw.rhccq_palette_reduce_bytes(K))
        work = rh.empty((wbytes // 8,), torch.int64)
        pal_out, cnt_out = rh.empty((K, 3), torch.uint8), rh.empty((K,), torch.int64)
        map_, merges, k_out = rh.empty((K,), torch.int32), rh.empty((K - 1, 2), torch.int32), rh.empty((1,), torch.int32)
        targets = [("none", K), ("half", K // 2), ("to_16", 16)]
        ms = {name: [] for name, _ in targets}
        for rep in range(args.reps + 1):                                    # (rep 0: the warm-up of this shape)
            for name, target in targets:
                def call():
                    rh._check(rh.lib.rhccq_palette_reduce(rh.ctx, rh._p(p), rh._p(counts), K, target, rh._p(work), wbytes, rh._p(pal_out),
                                                          rh._p(cnt_out), rh._p(map_), rh._p(merges), rh._p(k_out)), "palette_reduce")
                dt = events(call)
                assert int(k_out.item()) == target
                if rep:
                    ms[name].append(dt)
        base = statistics.median(ms["none"])
        for name, target in targets:
            med, steps = statistics.median(ms[name]), K - target
            out["kernel"].append({"K": K, "to": target, "steps": steps, "ms": round(med, 4), "runs_ms": [round(x, 4) for x in ms[name]],
                                  "us_per_step": round((med - base) * 1000.0 / steps, 3) if steps else None})

    failures = []
    for r in REFINES:
        rung = [x for x in out["ladder"] if x["refine"] == r]
        for hi, lo in zip(rung, rung[1:]):
            if lo["psnr"] > hi["psnr"]:
                failures.append(f"refine={r}: {lo['colours']} colours have a higher PSNR ({lo['psnr']}) than {hi['colours']} ({hi['psnr']})")
            if not lo["rhccq_bytes_exact"] < hi["rhccq_bytes_exact"]:
                failures.append(f"refine={r}: the file of {lo['colours']} colours is not smaller than that of {hi['colours']}")
    out["failures"] = failures
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if failures:
        sys.exit("; ".join(failures))


if __name__ == "__main__":
    main()
