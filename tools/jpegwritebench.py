"""The JPEG writer (csrc/jpeg_write.hip, container.jpeg_bytes) in ONE process: the 4K Kodak mosaic, resident on the device, written at quality
75 and 95 in 4:4:4 and 4:2:0, with and without restart_rows=1, by jpeg_bytes (tables, every launch, the length's read, the file's
download) and by the download plus Pillow's save on one host core, the contenders alternating inside every repetition; medians of --reps
with [min, max]; the device launches alone (Rhccq.jpeg_encode, nothing downloaded) and their blocks half (Rhccq.jpeg_blocks) beside
them.  Then the thumbnail path, 4K read_jpeg -> resize to 480 x 270 -> write_jpeg, against the same three steps in Pillow, and one
64 x 64 file.  Every file is compared with Pillow's first.  Writes profiles/jpeg_write.json."""
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
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from ditherbench import png  # noqa: E402

SUB = {"444": 0, "420": 2}


def med(v):
    return {"median_ms": round(1e3 * statistics.median(v), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3)}


def pillow_save(a, quality, sub, rows):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", quality=quality, subsampling=SUB[sub], optimize=False, **({"restart_marker_rows": rows} if rows else {}))
    return b.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_write.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import container, ops, synth
    from roibasedimagecompression_amd.image import ImageEncoder
    rh = ops.default_context()
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    dev = rh.dev(img)
    out = {"tool": "tools/jpegwritebench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "image": "kodak_mosaic", "shape": list(img.shape), "files": {}}

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def duel(frame, quality, sub, rows):
        assert container.jpeg_bytes(frame, rh, quality, sub, rows) == pillow_save(frame.cpu().numpy(), quality, sub, rows)
        t = {"jpeg_bytes": [], "download_pillow": [], "device_launches": [], "device_blocks": []}
        for _ in range(args.reps + 1):
            t["jpeg_bytes"].append(timed(lambda: container.jpeg_bytes(frame, rh, quality, sub, rows)))
            t["download_pillow"].append(timed(lambda: pillow_save(rh.to_host(frame), quality, sub, rows)))
            t["device_launches"].append(timed(lambda: rh.jpeg_encode(frame, sub, quality, rows)))
            t["device_blocks"].append(timed(lambda: rh.jpeg_blocks(frame, sub, quality)))
        return {k: med(v[1:]) for k, v in t.items()}

    for quality in (75, 95):
        for sub in ("444", "420"):
            for rows in (0, 1):
                name = f"q{quality}_{sub}" + ("_rst" if rows else "")
                out["files"][name] = dict(duel(dev, quality, sub, rows), bytes=len(container.jpeg_bytes(dev, rh, quality, sub, rows)))
                print(name, json.dumps(out["files"][name]), flush=True)
    small = dev[200:264, 300:364].contiguous()
    out["small_64x64_q75_420"] = duel(small, 75, "420", 0)
    print("64x64", json.dumps(out["small_64x64_q75_420"]), flush=True)

    src = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"jpegwritebench_{os.getpid()}.jpg")
    dst = src[:-4] + "_small.jpg"
    with open(src, "wb") as f:
        f.write(pillow_save(img, 90, "420", 0))
    enc = ImageEncoder(rh)

    def device_path():
        enc.resize(src, (270, 480), "lanczos", jpeg_path=dst, quality=75)

    def pillow_path():
        Image.open(src).convert("RGB").resize((480, 270), Image.LANCZOS, reducing_gap=None).save(dst + ".pil", "JPEG", quality=75, subsampling=2, optimize=False)
    t = {"read_resize_write_device": [], "read_resize_write_pillow": []}
    for _ in range(args.reps + 1):
        t["read_resize_write_device"].append(timed(device_path))
        t["read_resize_write_pillow"].append(timed(pillow_path))
    with open(dst, "rb") as a, open(dst + ".pil", "rb") as b:
        same = a.read() == b.read()
    out["thumbnail_4k_to_480x270"] = dict({k: med(v[1:]) for k, v in t.items()}, files_equal=same)
    print("thumbnail", json.dumps(out["thumbnail_4k_to_480x270"]), flush=True)
    for p in (src, dst, dst + ".pil"):
        os.remove(p)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
