"""The optimising JPEG writer (csrc/jpeg_optimize.hip, container.jpeg_bytes(optimize=True)) in ONE process: the 4K Kodak mosaic, resident on
the device, written at quality 75 and 95 in 4:4:4 and 4:2:0 by jpeg_bytes with and without optimize (tables, every launch, the length's
read, the file's download) and by the download plus Pillow's save(optimize=True) on one host core, the contenders alternating inside every
repetition; medians of --reps with [min, max]; the file's bytes both ways; the histogram and the table launches alone beside them
(Rhccq.jpeg_histogram, Rhccq.jpeg_huffman on coefficients and counts already there).  Every file is compared with Pillow's first.
Writes profiles/jpeg_optimize.json."""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from ditherbench import png  # noqa: E402

SUB = {"444": 0, "420": 2}


def med(v):
    return {"median_ms": round(1e3 * statistics.median(v), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3)}


def pillow_save(a, quality, sub, optimize):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=SUB[sub], optimize=optimize)
    return b.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_optimize.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import container, ops, synth
    rh = ops.default_context()
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    dev = rh.dev(img)
    out = {"tool": "tools/jpegoptbench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "image": "kodak_mosaic", "shape": list(img.shape), "files": {}}

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for quality in (75, 95):
        for sub in ("444", "420"):
            plain, made = container.jpeg_bytes(dev, rh, quality, sub), container.jpeg_bytes(dev, rh, quality, sub, optimize=True)
            assert plain == pillow_save(img, quality, sub, False) and made == pillow_save(img, quality, sub, True)
            coef = rh.jpeg_blocks(dev, sub, quality)
            counts = rh.jpeg_histogram(coef, img.shape, sub)
            t = {"jpeg_bytes": [], "jpeg_bytes_optimize": [], "download_pillow_optimize": [], "device_launches": [], "device_launches_optimize": [],
                 "histogram_launch": [], "huffman_launch": []}
            for _ in range(args.reps + 1):
                t["jpeg_bytes"].append(timed(lambda: container.jpeg_bytes(dev, rh, quality, sub)))
                t["jpeg_bytes_optimize"].append(timed(lambda: container.jpeg_bytes(dev, rh, quality, sub, optimize=True)))
                t["download_pillow_optimize"].append(timed(lambda: pillow_save(rh.to_host(dev), quality, sub, True)))
                t["device_launches"].append(timed(lambda: rh.jpeg_encode(dev, sub, quality)))
                t["device_launches_optimize"].append(timed(lambda: rh.jpeg_encode(dev, sub, quality, optimize=True)))
                t["histogram_launch"].append(timed(lambda: rh.jpeg_histogram(coef, img.shape, sub)))
                t["huffman_launch"].append(timed(lambda: rh.jpeg_huffman(counts, img.shape, sub, quality)))
            name = f"q{quality}_{sub}"
            out["files"][name] = dict({k: med(v[1:]) for k, v in t.items()}, bytes=len(plain), bytes_optimize=len(made),
                                      saved_percent=round(100.0 * (len(plain) - len(made)) / len(plain), 2))
            print(name, json.dumps(out["files"][name]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
