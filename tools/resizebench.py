"""The resize (csrc/resize.hip, Rhccq.resize) under tools/gifbench.py's conditions: ONE process, the 4K Kodak mosaic and 64 1080p frames cut
from it, frames resident, HIP events around --inner calls, every shape warmed up, medians of --reps windows with [min, max].
  (a) Rhccq.resize of the 4K frame to 1/2, 1/4 and 1/8 and of its 480p reduction back to 4K, for each filter; beside each time the bytes
      the two passes must move (source read, intermediate written and read once, result written: computed here from the shapes) over the
      card's HBM rate: the floor;
  (b) the 64-frame clip through ImageEncoder.animate(size=(270, 480)) against the path without it, ALTERNATING in one run: Pillow's
      resize of every frame on the host (the frames are on the host, as a caller of today has them), upload, animate.

    python tools/resizebench.py [--reps 5] [--inner 5] [--frames 64] [--out profiles/resize.json]"""
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

from ditherbench import png, window_ms  # noqa: E402

HBM_BYTES_PER_S = 8.0e12              # MI355X: 8 TB/s peak
PILLOW = {"box": Image.BOX, "triangle": Image.BILINEAR, "cubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def row(t):
    return {"median_ms": round(statistics.median(t), 4), "min_max_ms": [round(min(t), 4), round(max(t), 4)]}


def floor_bytes(B, H, W, C, OH, OW):
    """what the two passes must move: the source once, the intermediate [H][OW C rounded up to 4] out and in, the result once"""
    pitch = (OW * C + 3) & ~3
    return B * (H * W * C + 2 * H * pitch + OH * OW * C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import ops, synth
    from roibasedimagecompression_amd.image import ImageEncoder
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh = enc.rh
    rgb = rh.dev(img)
    out = {"tool": "tools/resizebench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "inner_calls": args.inner, "image": "kodak_mosaic",
           "shape": [H, W], "hbm_bytes_per_s": HBM_BYTES_PER_S, "single": [], "clip": {}}
    small = rh.resize(rgb, (H * 480 // W, 480), "lanczos")
    shapes = [("1/2", rgb, (H // 2, W // 2)), ("1/4", rgb, (H // 4, W // 4)), ("1/8", rgb, (H // 8, W // 8)), ("480p to 4K", small, (H, W))]
    for name, src, to in shapes:
        calls = {f: (lambda f=f: rh.resize(src, to, f)) for f in ops.RESIZE_FILTERS}
        for fn in calls.values():
            fn()                                                               # warm-up of every shape and filter
        times = {f: [] for f in calls}
        for _ in range(args.reps):                                           # interleaved: a repetition times every filter once
            for f, fn in calls.items():
                times[f].append(window_ms(fn, args.inner))
        nbytes = floor_bytes(1, int(src.shape[0]), int(src.shape[1]), 3, *to)
        for f in calls:
            r = dict(row(times[f]), shape=name, filter=f, **{"from": list(src.shape[:2]), "to": list(to)}, floor_bytes=nbytes,
                     floor_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 4))
            r["times_floor"] = round(r["median_ms"] / r["floor_ms"], 2)
            out["single"].append(r)
            print(json.dumps(r), flush=True)
    # ---- the clip: animate(size=) on resident frames against Pillow on the host, upload, animate ----
    B, h, w, to = args.frames, 1080, 1920, (270, 480)
    clip = torch.stack([rgb[4 * f:4 * f + h, 8 * f:8 * f + w] for f in range(B)]).contiguous()
    host = clip.cpu().numpy()

    def device_path():
        return enc.animate(clip, 256, size=to, resample="lanczos")

    def host_path():
        frames = np.stack([np.asarray(Image.fromarray(f).resize((to[1], to[0]), PILLOW["lanczos"], reducing_gap=None)) for f in host])
        return enc.animate(rh.dev(frames), 256)
    a, b = device_path(), host_path()                                         # warm-up; and the two paths build the same file
    same = bool(np.array_equal(a["palette"], b["palette"]) and torch.equal(a["indices"], b["indices"]))
    times = {"device": [], "host": []}
    for _ in range(args.reps):
        for name, fn in (("device", device_path), ("host", host_path)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    resize_only = [window_ms(lambda: rh.resize(clip, to, "lanczos"), args.inner) for _ in range(args.reps)]
    out["clip"] = {"frames": [B, h, w], "to": list(to), "filter": "lanczos", "same_result": same, "animate_size": row(times["device"]),
                   "pillow_upload_animate": row(times["host"]), "resize_alone": dict(row(resize_only), floor_ms=round(floor_bytes(B, h, w, 3, *to) / HBM_BYTES_PER_S * 1e3, 4))}
    print(json.dumps(out["clip"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
