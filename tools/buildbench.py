"""The palette build (csrc/palette_build.hip) on the 4K Kodak mosaic of tools/remapbench.py, in ONE process:
  (a) ImageEncoder.encode(image, 20, 10), the full hierarchy, and the plain remap onto its palette      wall time, PSNR, .rhccq bytes
  (b) ImageEncoder.quantize(image, colours=N, refine=R) for N = the rows of (a)'s palette and 256, R = 0, 4   wall time, PSNR, .rhccq bytes
  (c) rhccq_palette_cells alone on the resident frame (HIP events around the memset and the launch, the table allocated before)
  (d) rhccq_palette_build alone on (c)'s table (HIP events around its four launches, buffers allocated before) at K_target = 1 (the
      three prefix launches and a chain that evaluates box 0 and splits nothing), 64, 256 and the device cap; microseconds per chain
      step = (time - time at K_target = 1) / (K_target - 1)
  (e) rhccq_palette_moments alone on the resident frame, no index output, with a class map of two classes (the centre half of the frame
      and the rest: three tables), at (a)'s palette (accumulators in LDS) and at 1 024 colours sampled from the mosaic (above
      rhccq_palette_moments_lds_rows(2): one global atomic per pixel and quantity, the naive form of (c))
Medians of --reps runs after a warm-up of every shape; compared variants alternate.  The frame is uploaded ONCE before the timed loop:
(b) to (e) take resident device tensors, (a) takes the host image, as encode's region stage wants it.

Exits non-zero (the JSON is written all the same) when the cells pass is not faster than the moments pass in its global-memory form, or
quantize(colours=256) is not faster than encode: the two conditions the build was accepted on.  Neither has a margin.

    python tools/buildbench.py [--reps 5] [--out profiles/palette_build.json]"""
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
    n_px = H * W
    enc = ImageEncoder()
    rh, dev = enc.rh, enc.rh.device
    cap = ops.palette_build_max_rows()

    rgb = rh.dev(img)                                                       # resident: (b) to (e) read this tensor
    key = enc.encode(img, 20, 10)                                           # warm-up of every shape
    pal = np.asarray(key["palette"], np.uint8).reshape(-1, 3)
    rows = [(n, r) for n in sorted({len(pal), 256}) for r in REFINES]
    for n, r in rows:
        enc.quantize(rgb, colours=n, refine=r)
    ta, tb, rb = [], {k: [] for k in rows}, {}
    for _ in range(args.reps):                                              # alternating: all see the same machine state
        dt, key = wall(lambda: enc.encode(img, 20, 10), dev)
        ta.append(dt)
        for n, r in rows:
            dt, rb[(n, r)] = wall(lambda: enc.quantize(rgb, colours=n, refine=r), dev)
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

    def runs_ms(ts):
        return {"ms": round(statistics.median(ts), 4), "runs_ms": [round(v, 4) for v in ts]}
    plain = enc.encode_with_palette(rgb, pal)
    out = {"tool": "tools/buildbench.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "reps": args.reps, "image": "kodak_mosaic",
           "shape": [H, W], "qualities": [20, 10], "palette_size": len(pal), "max_rows": cap, "cells_granules": list(ops.palette_cells_granules()),
           "inputs": {"encode": "host image", "quantize": "resident device tensor (uploaded once before the timed loop)",
                      "kernel": "resident device tensors, buffers allocated before the timed calls"},
           "encode": dict(runs(ta), window=[top, left, h, w], sse=sse_a, psnr=psnr_from_sse(sse_a, h * w), rhccq_bytes_exact=size(key)),
           "encode_with_palette": {"sse": plain["stats"]["remap"]["all"]["sse"], "psnr": plain["stats"]["remap"]["all"]["psnr"],
                                   "rhccq_bytes_exact": size(plain), "indices_dtype": plain["indices_dtype"]},
           "quantize": [], "kernel": {}}
    for n, r in rows:
        st = rb[(n, r)]["stats"]
        out["quantize"].append(dict(runs(tb[(n, r)]), colours=n, refine=r, build=st["build"], sse=st["remap"]["all"]["sse"],
                                    psnr=st["remap"]["all"]["psnr"], indices_dtype=rb[(n, r)]["indices_dtype"], rhccq_bytes_exact=size(rb[(n, r)]),
                                    seconds=st["seconds"]))

    # (c), (d), (e): the launches alone, alternating
    rng = np.random.default_rng(1)
    flat = img.reshape(-1, 3)
    cells = rh.empty(ops.PALETTE_CELLS_SHAPE, torch.int64)
    wbytes = int(rh._raw.rhccq_palette_build_bytes())
    work = rh.empty((wbytes // 8,), torch.int64)
    pal_out, cnt_out, boxes = rh.empty((cap, 3), torch.uint8), rh.empty((cap,), torch.int64), rh.empty((cap, 6), torch.uint8)
    splits, k_out = rh.empty((cap, 3), torch.int32), rh.empty((1,), torch.int32)
    targets = sorted({1, 64, 256, cap})
    pals = {"lds": rh.dev(pal), "global": rh.dev(flat[rng.integers(0, len(flat), 1024)])}
    assert len(pal) <= ops.palette_moments_lds_rows(2) < 1024
    cls = rh.zeros((H, W), torch.uint8)
    cls[H // 4:H - H // 4, W // 4:W - W // 4] = 1
    moments = {k: rh.empty((3, int(p.shape[0]), 5), torch.int64) for k, p in pals.items()}

    def cells_call():
        rh._check(rh.lib.rhccq_palette_cells(rh.ctx, rh._p(rgb), n_px, None, 0, None, 0, rh._p(cells)), "palette_cells")

    def build_call(target):
        rh._check(rh.lib.rhccq_palette_build(rh.ctx, rh._p(cells), target, rh._p(work), wbytes, rh._p(pal_out), rh._p(cnt_out), rh._p(boxes),
                                             rh._p(splits), rh._p(k_out)), "palette_build")

    def moments_call(which):
        p = pals[which]
        rh._check(rh.lib.rhccq_palette_moments(rh.ctx, rh._p(rgb), n_px, rh._p(p), int(p.shape[0]), rh._p(cls), 2, None, 0, rh._p(moments[which])),
                  "palette_moments")
    t_cells, t_build, t_mom = [], {t: [] for t in targets}, {k: [] for k in pals}
    for rep in range(args.reps + 1):                                        # (rep 0: the warm-up of every shape)
        dt = events(cells_call)
        if rep:
            t_cells.append(dt)
        for t in targets:
            dt = events(lambda: build_call(t))
            assert int(k_out.item()) == t
            if rep:
                t_build[t].append(dt)
        for k in pals:
            dt = events(lambda: moments_call(k))
            if rep:
                t_mom[k].append(dt)
    assert int(cells[0].sum()) == n_px
    base = statistics.median(t_build[1])
    out["kernel"]["cells"] = dict(runs_ms(t_cells), pixels=n_px, occupied_cells=int((cells[0] != 0).sum()))
    out["kernel"]["build"] = [dict(runs_ms(t_build[t]), K_target=t, steps=t - 1,
                                   us_per_step=round((statistics.median(t_build[t]) - base) * 1000.0 / (t - 1), 3) if t > 1 else None) for t in targets]
    out["kernel"]["moments"] = [dict(runs_ms(t_mom[k]), K=int(pals[k].shape[0]), n_classes=2, accumulators=k) for k in pals]
    cells_ms, naive_ms = out["kernel"]["cells"]["ms"], statistics.median(t_mom["global"])
    q256 = next(x for x in out["quantize"] if x["colours"] == 256 and x["refine"] == 0)
    out["ratios"] = {"moments_global_over_cells": round(naive_ms / cells_ms, 2),
                     "moments_lds_over_cells": round(statistics.median(t_mom["lds"]) / cells_ms, 2),
                     "encode_over_quantize_256": round(out["encode"]["median_s"] / q256["median_s"], 1)}
    # beside the reduction's merge step as tools/reducebench.py recorded it (256 rows down to 128), when that profile is there
    recorded = os.path.join(ROOT, "profiles", "palette_reduce.json")
    if os.path.exists(recorded):
        with open(recorded) as f:
            step = next((k["us_per_step"] for k in json.load(f)["kernel"] if (k["K"], k["to"]) == (256, 128)), None)
        if step:
            mine = next(b["us_per_step"] for b in out["kernel"]["build"] if b["K_target"] == 256)
            out["reduce_step"] = {"source": "profiles/palette_reduce.json", "K": 256, "to": 128, "us_per_step": step}
            out["ratios"]["build_step_over_reduce_step_256"] = round(mine / step, 2)

    failures = []
    if not cells_ms < naive_ms:
        failures.append(f"the cells pass ({cells_ms} ms) is not faster than the moments pass in global memory ({naive_ms} ms)")
    if not q256["median_s"] < out["encode"]["median_s"]:
        failures.append(f"quantize(colours=256) ({q256['median_s']} s) is not faster than encode ({out['encode']['median_s']} s)")
    out["failures"] = failures
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if failures:
        sys.exit("; ".join(failures))


if __name__ == "__main__":
    main()
