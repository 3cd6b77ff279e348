"""The batched palette build path (csrc/palette_batch.hip, ImageEncoder.quantize_batch) against the loop of ImageEncoder.quantize it
replaces, in ONE process, on B = 1, 8 and 64 frames of 1920 x 1080 cut from the 4K Kodak mosaic of tools/remapbench.py:
  (a) quantize_batch(frames, colours=256, refine=R) for R = 0 and 4                                   wall time
  (b) [quantize(frame, colours=256, refine=R) for frame in frames] over the same frames, same run     wall time (the yardstick: quantize
      is unchanged code)
  (c) the batched launches alone on the resident frames (HIP events around each call, buffers allocated before): cells, build at
      K_target = 1 (the prefix launches and chains that split nothing) and 256 (their difference is the chains), refine (4 iterations),
      remap
Medians of --reps runs after a warm-up of every shape, with the runs and their spread (max - min) beside them; (a) and (b) alternate.
The frames are uploaded ONCE, as one [B, 1080, 1920, 3] tensor: (a) takes it in place, (b) takes its slices.  (a) and (b) are checked to
agree on every frame's palette and indices before anything is timed.

    python tools/batchbench.py [--reps 5] [--batches 1,8,64] [--out profiles/palette_batch.json]"""
import argparse
import ctypes as C
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
REFINES = (0, 4)
COLOURS = 256
FH, FW = 1080, 1920


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


def runs(ts, unit="s", digits=5):
    return {f"median_{unit}": round(statistics.median(ts), digits), f"runs_{unit}": [round(v, digits) for v in ts],
            f"spread_{unit}": round(max(ts) - min(ts), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from roibasedimagecompression_amd import synth
    from roibasedimagecompression_amd.image import ImageEncoder
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh, dev = enc.rh, enc.rh.device
    batches = [int(v) for v in args.batches.split(",")]
    top = max(batches)
    # frames at distinct offsets of the mosaic, spread over it
    ys, xs = np.linspace(0, H - FH, 8).astype(int), np.linspace(0, W - FW, max((top + 7) // 8, 1)).astype(int)
    where = [(int(y), int(x)) for x in xs for y in ys][:top]
    frames = rh.dev(np.stack([img[y:y + FH, x:x + FW] for y, x in where]))          # resident: everything below reads this tensor
    out = {"tool": "tools/batchbench.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "reps": args.reps, "image": "kodak_mosaic",
           "mosaic_shape": [H, W], "frame_shape": [FH, FW], "colours": COLOURS, "slice": enc.QUANTIZE_BATCH_SLICE,
           "inputs": "one resident [B, 1080, 1920, 3] device tensor, uploaded once; quantize takes its slices", "wall": [], "kernel": []}

    for B in batches:
        part = frames[:B]
        n_px = B * FH * FW
        for r in REFINES:
            got = enc.quantize_batch(part, COLOURS, refine=r)                          # warm-up of every shape, and the check
            loop = [enc.quantize(part[i], COLOURS, refine=r) for i in range(B)]
            for a, b in zip(got, loop):
                assert np.array_equal(a["palette"], b["palette"]) and torch.equal(a["indices"], b["indices"]) and a["stats"]["build"] == b["stats"]["build"]
            tb, tl = [], []
            for _ in range(args.reps):                                                  # alternating: both see the same machine state
                tb.append(wall(lambda: enc.quantize_batch(part, COLOURS, refine=r), dev)[0])
                tl.append(wall(lambda: [enc.quantize(part[i], COLOURS, refine=r) for i in range(B)], dev)[0])
            mb, ml = statistics.median(tb), statistics.median(tl)
            out["wall"].append({"B": B, "refine": r, "batch": runs(tb), "loop": runs(tl), "loop_over_batch": round(ml / mb, 2),
                                "batch_ms_per_frame": round(mb * 1000.0 / B, 3), "loop_ms_per_frame": round(ml * 1000.0 / B, 3),
                                "batch_mpx_s": round(n_px / mb / 1e6, 1), "loop_mpx_s": round(n_px / ml / 1e6, 1),
                                "gain_exceeds_spread": bool(ml - mb > max(max(tb) - min(tb), max(tl) - min(tl)))})

        # (c): the launches alone
        rgb = part.reshape(-1, 3)
        off = (np.arange(B + 1, dtype=np.int64) * FH * FW)
        off_dev = rh.dev(off)
        p_off = C.c_void_p(off.ctypes.data)
        cells = rh.empty((B, 4, 32, 32, 32), torch.int64)
        wbytes = int(rh._raw.rhccq_palette_build_batch_bytes(B))
        work = rh.empty((wbytes // 8,), torch.int64)
        pal, cnt = rh.empty((B, COLOURS, 3), torch.uint8), rh.empty((B, COLOURS), torch.int64)
        k_out = rh.empty((B,), torch.int32)
        idx, sums = rh.empty((n_px,), torch.uint8), rh.empty((B, 1, 2), torch.int64)
        rbytes = int(rh._raw.rhccq_palette_refine_batch_bytes(B, COLOURS))
        rwork, hist, nit = rh.empty((rbytes // 8,), torch.int64), rh.empty((B, 4, 2), torch.int64), rh.empty((B,), torch.int32)
        refined = rh.empty((B, COLOURS, 3), torch.uint8)

        def cells_call():
            rh._check(rh.lib.rhccq_palette_cells_batch(rh.ctx, rh._p(rgb), p_off, rh._p(off_dev), B, None, 0, None, rh._p(cells)), "palette_cells_batch")

        def build_call(target):
            rh._check(rh.lib.rhccq_palette_build_batch(rh.ctx, rh._p(cells), B, target, rh._p(work), wbytes, rh._p(pal), rh._p(cnt), None, None,
                                                       rh._p(k_out)), "palette_build_batch")

        def refine_call():
            rh._check(rh.lib.rhccq_palette_refine_batch(rh.ctx, rh._p(rgb), p_off, rh._p(off_dev), B, rh._p(refined), COLOURS, rh._p(k_out), None, 0, None, 4,
                                                        rh._p(rwork), rbytes, rh._p(hist), rh._p(nit)), "palette_refine_batch")

        def remap_call():
            rh._check(rh.lib.rhccq_palette_remap_batch(rh.ctx, rh._p(rgb), p_off, rh._p(off_dev), B, rh._p(pal), COLOURS, rh._p(k_out), None, 0, rh._p(idx), 1,
                                                       rh._p(sums)), "palette_remap_batch")
        t = {"cells": [], "build_K1": [], "build_K256": [], "refine_4": [], "remap": []}
        for rep in range(args.reps + 1):                                                # (rep 0: the warm-up)
            row = {"cells": events(cells_call), "build_K1": events(lambda: build_call(1)), "build_K256": events(lambda: build_call(COLOURS))}
            refined.copy_(pal)                                                          # (every repetition refines the built palettes)
            row["refine_4"] = events(refine_call)
            row["remap"] = events(remap_call)
            if rep:
                for key, v in row.items():
                    t[key].append(v)
        assert int(k_out.min()) == COLOURS and int(sums[:, 0, 0].sum()) == n_px
        chain = statistics.median(t["build_K256"]) - statistics.median(t["build_K1"])
        out["kernel"].append(dict({key: runs(v, "ms", 4) for key, v in t.items()}, B=B, pixels=n_px, chains_ms=round(chain, 4),
                                  chain_us_per_step=round(chain * 1000.0 / (COLOURS - 1), 3), iterations=[int(v) for v in nit.tolist()][:8]))

    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
