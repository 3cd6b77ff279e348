"""The JPEG reader (csrc/jpeg_read.hip, container.read_jpeg) in ONE process: the 4K Kodak mosaic saved by Pillow in six variants (quality 75
and 95, 4:2:0 and 4:4:4 at 95, with and without restart_marker_rows=1 at 75 4:2:0 and 95 4:4:4), each read by read_jpeg (the host parse,
the upload, every launch, the status read), by Pillow on one host core (Image.open + np.asarray + upload) and by the serial host form,
the contenders alternating inside every repetition; medians of --reps with [min, max].  Then a sweep of subsequence_bits over 256..4096
on the device decode alone (file and tables resident), with the sync rounds each took, and the two halves of the decode: the entropy
half alone (Rhccq.jpeg_coefficients: unstuff .. dc) and what the whole call takes beyond it (idct and colour).  Then small files (crops of
the mosaic from 64 x 64 to 1080p, quality 90 4:2:0) and a clip of 64 frames of 1080p as a loop of files, read_jpeg against Pillow plus
upload.  Writes profiles/jpeg_read.json."""
import argparse
import ctypes as C
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

VARIANTS = {"q75_420": dict(quality=75, subsampling=2), "q95_420": dict(quality=95, subsampling=2), "q95_444": dict(quality=95, subsampling=0),
            "q75_420_rst": dict(quality=75, subsampling=2, restart_marker_rows=1), "q95_444_rst": dict(quality=95, subsampling=0, restart_marker_rows=1),
            "q75_444": dict(quality=75, subsampling=0)}


def med(v):
    return {"median_ms": round(1e3 * statistics.median(v), 3), "min_ms": round(1e3 * min(v), 3), "max_ms": round(1e3 * max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_read.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import _lib, container, ops, synth
    rh = ops.default_context()
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    out = {"tool": "tools/jpegbench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "image": "kodak_mosaic", "shape": list(img.shape), "files": {}}
    lib = _lib.load()
    for name, kw in VARIANTS.items():
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", **kw)
        data = b.getvalue()
        a = np.frombuffer(data, np.uint8)
        ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        res = container.read_jpeg(data, rh)
        assert np.array_equal(res["image"].cpu().numpy(), ref), name
        t = {"read_jpeg": [], "pillow_upload": [], "host_form": []}
        host_rgb, st = np.zeros_like(ref), np.zeros(2, np.int32)
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            container.read_jpeg(data, rh)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))).to(rh.device)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            lib.rhccq_jpeg_decode_host(C.c_void_p(a.ctypes.data), a.size, C.c_void_p(host_rgb.ctypes.data), C.c_void_p(st.ctypes.data))
            t3 = time.perf_counter()
            t["read_jpeg"].append(t1 - t0), t["pillow_upload"].append(t2 - t1), t["host_form"].append(t3 - t2)
        parsed, dev = ops.jpeg_parse(data), rh.dev(a.copy())
        sweep = {}
        for S in (256, 512, 1024, 2048, 4096):
            v = []
            for _ in range(args.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o = rh.jpeg_decode(dev, parsed, subsequence_bits=S)
                torch.cuda.synchronize()
                v.append(time.perf_counter() - t0)
            head = rh.to_host(o["head"])
            sweep[str(S)] = dict(med(v[1:]), subsequences=int(head[1]), rounds=int(head[2]), boundary_rounds=int(head[3]), longest_walk=int(head[4]))
        halves = {"entropy": [], "whole": []}
        for _ in range(args.reps + 1):
            for key, call in (("entropy", rh.jpeg_coefficients), ("whole", rh.jpeg_decode)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(dev, parsed)
                torch.cuda.synchronize()
                halves[key].append(time.perf_counter() - t0)
        stages = {"entropy_unstuff_to_dc": med(halves["entropy"][1:]), "whole_decode": med(halves["whole"][1:]),
                  "idct_and_colour_by_difference_ms": round(1e3 * (statistics.median(halves["whole"][1:]) - statistics.median(halves["entropy"][1:])), 3)}
        out["files"][name] = {"bytes": len(data), "stats": res["stats"], **{k: med(v) for k, v in t.items()}, "device_decode_by_subsequence_bits": sweep,
                              "device_halves": stages}
        print(name, json.dumps(out["files"][name]), flush=True)

    def duel(files):
        """the files one after another by read_jpeg and by Pillow plus upload, alternating -> the two medians"""
        t = {"read_jpeg": [], "pillow_upload": []}
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for d in files:
                container.read_jpeg(d, rh)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for d in files:
                torch.from_numpy(np.array(Image.open(io.BytesIO(d)).convert("RGB"))).to(rh.device)
            torch.cuda.synchronize()
            t["read_jpeg"].append(t1 - t0), t["pillow_upload"].append(time.perf_counter() - t1)
        return {k: med(v[1:]) for k, v in t.items()}

    def saved(a):
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(a)).save(b, "JPEG", quality=90, subsampling=2)
        return b.getvalue()
    out["small_files"] = {}
    for h, w in ((64, 64), (256, 256), (512, 768), (1080, 1920)):
        data = saved(img[200:200 + h, 300:300 + w])
        assert np.array_equal(container.read_jpeg(data, rh)["image"].cpu().numpy(), np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
        out["small_files"][f"{h}x{w}"] = dict(duel([data]), bytes=len(data))
        print(h, w, json.dumps(out["small_files"][f"{h}x{w}"]), flush=True)
    clip = [saved(img[8 * i:8 * i + 1080, 24 * i:24 * i + 1920]) for i in range(64)]
    out["clip_64x1080p_loop_of_files"] = dict(duel(clip), bytes=sum(len(d) for d in clip))
    print("clip", json.dumps(out["clip_64x1080p_loop_of_files"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
