"""ImageEncoder.encode (roibasedimagecompression_amd/image.py) against flow.script_flow on Lenna, the 24 Kodak images and a 4K mosaic of
Kodak images (synth.kodak_mosaic): best-of-N wall time of each, their per-stage host clocks, and the device-to-host bytes each moves
(torch.Tensor.cpu, torch.Tensor.to to the host, Rhccq.to_host), ImageEncoder's split by stage.  No container in either.

    python tools/imagebench.py [--reps N] [--only NAME] [--out profiles/r08_image_flow.json]
Kernel times: a separate `rocprofv3 --kernel-trace --stats` run with `--only mosaic --reps 1`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")


class D2H:
    """counts device-to-host bytes while active, under the label in `stage`"""

    def __init__(self):
        self.bytes, self.stage = {}, "other"

    def _add(self, n):
        self.bytes[self.stage] = self.bytes.get(self.stage, 0) + n

    def __enter__(self):
        from roibasedimagecompression_amd.ops import Rhccq
        self._orig = (torch.Tensor.cpu, torch.Tensor.to, Rhccq.to_host)
        o_cpu, o_to, o_host = self._orig
        me = self

        def cpu(t, *a, **k):
            if t.is_cuda:
                me._add(t.numel() * t.element_size())
            return o_cpu(t, *a, **k)

        def to(t, *a, **k):
            out = o_to(t, *a, **k)
            if t.is_cuda and not out.is_cuda:
                me._add(t.numel() * t.element_size())
            return out

        def to_host(rh, *ts):
            me._add(sum(t.numel() * t.element_size() for t in ts))
            return o_host(rh, *ts)
        torch.Tensor.cpu, torch.Tensor.to, Rhccq.to_host = cpu, to, to_host
        return self

    def __exit__(self, *exc):
        from roibasedimagecompression_amd.ops import Rhccq
        torch.Tensor.cpu, torch.Tensor.to, Rhccq.to_host = self._orig


def png(name):
    return np.asarray(Image.open(os.path.join(G, name + ".png")).convert("RGB"), dtype=np.uint8)


def inputs(only):
    from roibasedimagecompression_amd import synth
    names = ["Lenna"] + [f"kodak_{i}" for i in range(1, 25)] + ["mosaic"]
    for name in names:
        if only and name != only:
            continue
        if name == "mosaic":
            yield name, synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
        else:
            yield name, png(name)


def measure(name, img, reps):
    from roibasedimagecompression_amd.flow import script_flow
    from roibasedimagecompression_amd.image import ImageEncoder
    enc = ImageEncoder()
    dev = enc.rh.device
    enc.encode(img, 20, 10)                                                # warm-up (and the library's first loads)
    best, stages = float("inf"), None
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = enc.encode(img, 20, 10)
        dt = time.perf_counter() - t0
        if dt < best:
            best, stages = dt, res["stats"]["seconds"]
    ref_best, ref_stages = float("inf"), None
    for _ in range(max(1, min(reps, 2))):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        _, _, info = script_flow(img, 20, 10, container=False)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if dt < ref_best:
            ref_best, ref_stages = dt, info["seconds"]
    with D2H() as d:
        d.stage = "regions"
        regions, maps, rgb, _ = enc.regions(img)
        d.stage = "split_score"
        n_seg = enc.split_segments(rgb, maps, regions)
        d.stage = "slic"
        small = enc.slic(img, rgb, maps, regions, n_seg)
        d.stage = "layers"
        enc.layers(maps, regions, small, (20, 10))
        d.stage = "encode_total"
        enc.encode(img, 20, 10)
        d.stage = "script_flow_total"
        script_flow(img, 20, 10, container=False)
    st = res["stats"]
    H, W = img.shape[:2]
    return {"image": name, "shape": [H, W], "image_encoder_s": round(best, 4), "image_encoder_mpx_s": round(H * W / best / 1e6, 2),
            "image_encoder_stages_s": stages, "script_flow_s": round(ref_best, 4), "script_flow_stages_s": ref_stages,
            "speedup": round(ref_best / best, 2), "d2h_bytes": d.bytes, "frame_bytes": int(img.size),
            "regions": [st["roi_regions"], st["nonroi_regions"]], "segments": [st["roi_segments"], st["nonroi_segments"]],
            "segments_dropped": st["segments_dropped"], "layers": [st["roi_layers"], st["nonroi_layers"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    for name, img in inputs(args.only):
        row = measure(name, img, args.reps)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/imagebench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
