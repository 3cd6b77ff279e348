"""Writing a result as a PNG file on the device (csrc/png_write.hip) on the 4K Kodak mosaic of tools/imagebench.py, under the other palette
tools' conditions: ONE process, the frame and the result resident, HIP events around --inner calls, medians of --reps windows after a
warm-up of every shape.  For ImageEncoder.quantize at 2, 4, 16, 230 and 256 colours and for a palette above 256 rows:
  (a) Rhccq.png_encode_async, fast and exact, and its parts in calls of their own: the scanlines (rhccq_png_scanlines), the deflate
      (rhccq_zlib_compress / rhccq_zlib9_compress over those scanlines), the CRC (rhccq_crc32 over the stream with its device-side
      length), and the copy of the finished file to the host (Rhccq.to_host, wall clock);
  (b) the file's bytes, fast and exact, beside the bytes of the exact .rhccq of the same result (container.frame_bytes(exact=True));
  (c) the host baseline: Pillow's Image.save(..., compress_level=9) of the same index map and palette (mode P up to 256 rows, RGB
      above), wall clock and bytes, the index map already on the host; and zlib.crc32 of the fast stream on the host beside the CRC launches.
The floor the three new kernels are compared with is the bytes they must move over the HBM figures of the MI355X guide (8.0 TB/s
specified, 6.3 TB/s achieved by a float4 copy), not a figure of this code.

    python tools/pngbench.py [--reps 5] [--inner 5] [--host-reps 5] [--out profiles/png_write.json]"""
import argparse
import io
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ditherbench import png, window_ms  # noqa: E402

COLOURS = (2, 4, 16, 230, 256, 1024)
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.3


def row(t):
    return {"median_ms": round(statistics.median(t), 4), "runs_ms": [round(v, 4) for v in t]}


def wall_ms(fn, reps):
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return row(t)


def floor_us(n_bytes):
    return {"bytes": int(n_bytes), "us_at_spec": round(n_bytes / HBM_SPEC_TBS * 1e-6, 3), "us_at_copy_rate": round(n_bytes / HBM_COPY_TBS * 1e-6, 3)}


def pillow_save(idx, pal):
    from PIL import Image
    if len(pal) <= 256:
        im = Image.fromarray(idx.astype(np.uint8), "P")
        im.putpalette(pal.reshape(-1).tolist())
    else:
        im = Image.fromarray(pal[idx], "RGB")
    buf = io.BytesIO()
    im.save(buf, format="PNG", compress_level=9)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_write.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import container, synth
    from roibasedimagecompression_amd.image import ImageEncoder
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh, dev = enc.rh, enc.rh.device
    rgb = rh.dev(img)                                                        # the resident frame
    out = {"tool": "tools/pngbench.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "reps": args.reps, "inner_calls": args.inner,
           "host_reps": args.host_reps, "image": "kodak_mosaic", "shape": [H, W],
           "inputs": "resident device tensors (frame, index map and palette); output buffers and workspaces are allocated inside the calls",
           "hbm_tb_per_s": {"spec": HBM_SPEC_TBS, "float4_copy": HBM_COPY_TBS}, "rows": []}
    for colours in COLOURS:
        res = enc.quantize(rgb, colours=colours)
        pal = np.asarray(res["palette"], np.uint8).reshape(-1, 3)
        K = len(pal)
        idx, d_pal = res["indices"].reshape(-1).contiguous(), rh.dev(pal)
        host_idx = idx.cpu().numpy()
        host_idx = (host_idx.view(np.uint16) if host_idx.dtype == np.int16 else host_idx).reshape(H, W)
        r = {"asked": colours, "K": K, "colour_type": 3 if K <= 256 else 2, "index_bytes": idx.element_size()}

        def timed(fn):
            fn()                                                             # warm-up of this shape
            return row([window_ms(fn, args.inner) for _ in range(args.reps)])
        scan, rows = rh.png_scanlines(idx, H, W, d_pal)
        r["filter_rows"] = [int(v) for v in rows.cpu()]
        r["scan_bytes"] = scan.numel()
        r["scanlines"] = timed(lambda: rh.png_scanlines(idx, H, W, d_pal))
        # colour type 2 reads the row and the row above in both passes; the floor counts every byte once
        r["scanlines_floor"] = floor_us(idx.numel() * idx.element_size() + scan.numel())
        for name, exact in (("fast", False), ("exact", True)):
            stream, length = rh.zlib_compress_async(scan, exact=exact)
            n = int(length.item())
            e = {"deflate": timed(lambda: rh.zlib_compress_async(scan, exact=exact)), "stream_bytes": n,
                 "crc": timed(lambda: rh.crc32_async(stream, length)), "crc_floor": floor_us(n),
                 "png_encode_async": timed(lambda: rh.png_encode_async(idx, H, W, d_pal, exact=exact))}
            o, ln = rh.png_encode_async(idx, H, W, d_pal, exact=exact)
            size = int(ln.item())
            e["png_bytes"] = size
            e["copy_to_host_wall"] = wall_ms(lambda: rh.to_host(o[:size]), args.reps)
            e["png_encode_wall"] = wall_ms(lambda: rh.png_encode(idx, H, W, d_pal, exact=exact), args.reps)
            if not exact:
                host_stream = rh.to_host(stream[:n]).tobytes()
                t = []
                for _ in range(args.host_reps):
                    t0 = time.perf_counter()
                    zlib.crc32(host_stream)
                    t.append((time.perf_counter() - t0) * 1e3)
                e["host_zlib_crc32_of_stream"] = row(t)
            r[name] = e
        r["rhccq_bytes_exact"] = len(container.frame_bytes(res, rh, exact=True))
        t, data = [], b""
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            data = pillow_save(host_idx, pal)
            t.append((time.perf_counter() - t0) * 1e3)
        r["pillow_level9"] = dict(row(t), bytes=len(data))
        if K > 256:
            plain = rh.png_encode(idx, H, W, d_pal, exact=True, filter=False)
            r["exact_png_bytes_without_filters"] = len(plain)
        out["rows"].append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
