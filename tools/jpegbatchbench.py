"""The batch JPEG reader (csrc/jpeg_batch.hip, container.read_jpeg_batch) in ONE process against the loop of container.read_jpeg it replaces
and against Pillow on one host core plus an upload: wall clock from the files' bytes in host memory to their pixels on the device, the three
contenders alternating inside every repetition; medians of --reps with [min, max].  Workloads (crops of the 4K Kodak mosaic, quality 90,
4:2:0): 64 files of 1080p, 256 of 256 x 256, 256 of 64 x 64, a mixed batch of all three sizes; and one 4K file through the batch form
against read_jpeg.  Every decode is checked against Pillow first.  Writes profiles/jpeg_batch.json."""
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


def med(v):
    return {"median_ms": round(1e3 * statistics.median(v), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3)}


def pillow(data):
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_batch.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import container, ops, synth
    rh = ops.default_context()
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])

    def saved(a, **kw):
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(a)).save(b, "JPEG", **{"quality": 90, "subsampling": 2, **kw})
        return b.getvalue()

    def crops(n, h, w):
        ys, xs = (img.shape[0] - h) // max(n - 1, 1), (img.shape[1] - w) // max(n - 1, 1)
        return [saved(img[ys * i:ys * i + h, xs * i:xs * i + w]) for i in range(n)]
    clip, mid, thumbs = crops(64, 1080, 1920), crops(256, 256, 256), crops(256, 64, 64)
    workloads = {"64x1080p": clip, "256x256x256": mid, "256x64x64": thumbs, "mixed_16x1080p_64x256_64x64": clip[::4] + mid[::4] + thumbs[::4],
                 "1x4k": [saved(img)]}
    out = {"tool": "tools/jpegbatchbench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "image": "kodak_mosaic crops, quality 90, 4:2:0",
           "clock": "bytes in host memory -> pixels on the device, synchronised", "workloads": {}}
    for name, files in workloads.items():
        res = container.read_jpeg_batch(files, rh)
        for d, got in zip(files, res["images"]):
            ref = pillow(d)
            assert np.array_equal(got.cpu().numpy(), ref) and np.array_equal(container.read_jpeg(d, rh)["image"].cpu().numpy(), ref), name
        t = {"read_jpeg_batch": [], "read_jpeg_loop": [], "pillow_upload": []}
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            container.read_jpeg_batch(files, rh)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for d in files:
                container.read_jpeg(d, rh)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            for d in files:
                torch.from_numpy(pillow(d)).to(rh.device)
            torch.cuda.synchronize()
            t["read_jpeg_batch"].append(t1 - t0), t["read_jpeg_loop"].append(t2 - t1), t["pillow_upload"].append(time.perf_counter() - t2)
        # where the batch call's time goes: the host parse of every file, filling and copying the one upload, the launches
        parts = {"host_parse": [], "device_decode_from_parsed": []}
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            parsed = [ops.jpeg_parse(d) for d in files]
            t1 = time.perf_counter()
            rh.jpeg_decode_batch(files, parsed)
            torch.cuda.synchronize()
            parts["host_parse"].append(t1 - t0), parts["device_decode_from_parsed"].append(time.perf_counter() - t1)
        files_stats = res["stats"]["files"]
        out["workloads"][name] = {"files": len(files), "bytes": sum(len(d) for d in files), "subsequences": sum(s["subsequences"] for s in files_stats),
                                  "most_sync_rounds": max(s["sync_rounds"] for s in files_stats), **{k: med(v[1:]) for k, v in t.items()},
                                  "batch_parts": {k: med(v[1:]) for k, v in parts.items()}}
        print(name, json.dumps(out["workloads"][name]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
