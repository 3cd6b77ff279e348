"""Reading a PNG file on the device (csrc/png_read.hip) on the 4K Kodak mosaic of tools/imagebench.py, under the other palette tools'
conditions: ONE process, the file resident, HIP events around --inner calls, medians of --reps windows after a warm-up of every shape.
Three forms of the mosaic:
  pillow_rgb     truecolour written by Pillow at its default level (adaptive filters, many IDATs);
  palette_256    the project's own 256-colour palette PNG (container.png_bytes of ImageEncoder.quantize);
  truecolour_1024   its 1 024-row truecolour PNG.
Per form: the stages in calls of their own -- segment CRCs, IDAT join, inflate, unfilter, expand --, Rhccq.png_decode (all of them on one
stream, the file and its table resident), and by the wall clock container.read_png of the file beside Image.open + np.asarray + upload
of the same file.  The unfilter kernel is set against its floor: the scanline bytes in and the raw bytes out over the HBM figures of the
MI355X guide (8.0 TB/s specified, 6.3 TB/s achieved by a float4 copy), not a figure of this code.

    python tools/pngreadbench.py [--reps 5] [--inner 3] [--host-reps 5] [--out profiles/png_read.json]"""
import argparse
import io
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ditherbench import png, window_ms  # noqa: E402
from pngbench import floor_us, row, wall_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_read.json"))
    args = ap.parse_args()
    from PIL import Image
    from roibasedimagecompression_amd import container, ops, synth
    from roibasedimagecompression_amd.image import ImageEncoder
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh, dev = enc.rh, enc.rh.device
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="PNG")
    files = {"pillow_rgb": buf.getvalue()}
    rgb = rh.dev(img)
    files["palette_256"] = container.png_bytes(enc.quantize(rgb, colours=256), rh)
    files["truecolour_1024"] = container.png_bytes(enc.quantize(rgb, colours=1024), rh)
    out = {"tool": "tools/pngreadbench.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "reps": args.reps, "inner_calls": args.inner,
           "host_reps": args.host_reps, "image": "kodak_mosaic", "shape": [H, W],
           "unfilter_geometry": {"band_rows": ops.png_unfilter_band_rows(), "tile_steps": ops.png_unfilter_tile(), "granule_units": ops.png_unfilter_granule()},
           "inputs": "the file and its chunk table resident; output buffers and workspaces are allocated inside the calls",
           "rows": []}
    tmp = tempfile.mkdtemp()
    for name, data in files.items():
        info, table = ops.png_parse(data)
        assert info.status == 0
        file_dev = rh.dev(np.frombuffer(data, np.uint8).copy())
        n = len(data)
        r = {"form": name, "file_bytes": n, "colour_type": info.colour_type, "depth": info.depth, "bpp": info.bpp, "chunks": info.n_chunks,
             "idat_chunks": info.n_idat, "idat_bytes": info.idat_bytes, "scan_bytes": info.scan_bytes}

        def timed(fn):
            fn()                                                             # warm-up of this shape
            return row([window_ms(fn, args.inner) for _ in range(args.reps)])
        whole = rh.png_decode(file_dev, info, table)
        assert [int(v) for v in whole["status"].cpu()] == [0, 0]
        scan = whole["scan"].clone()
        types = scan[::info.rowbytes + 1].cpu().numpy()
        r["filter_rows"] = [int(v) for v in np.bincount(types, minlength=5)]
        r["rows_that_need_the_row_above"] = int((types >= 2).sum())
        segs = table[:, :2].copy()
        r["crcs"] = timed(lambda: rh.crc32_segments(file_dev, segs, extra=4))
        idat = rh.dev(table[info.first_idat:info.first_idat + info.n_idat].reshape(-1))
        stream = torch.empty((info.idat_bytes + 16,), dtype=torch.uint8, device=dev)
        r["join"] = timed(lambda: rh._check(rh.lib.rhccq_png_join(rh.ctx, rh._p(file_dev), n, rh._p(idat), info.n_idat, info.idat_bytes, rh._p(stream)), "png_join"))
        r["inflate"] = timed(lambda: rh.zlib_decompress_async(stream[:info.idat_bytes], info.scan_bytes))
        r["unfilter"] = timed(lambda: rh.png_unfilter(scan, info.height, info.rowbytes, info.bpp))
        r["unfilter_floor"] = floor_us(info.scan_bytes + info.rowbytes * info.height)
        r["unfilter_steps"] = {"units_a_row": info.rowbytes // info.bpp, "bands": -(-info.height // ops.png_unfilter_band_rows())}
        raw, _ = rh.png_unfilter(scan, info.height, info.rowbytes, info.bpp)
        pal = file_dev[info.plte_offset:info.plte_offset + 3 * info.palette_rows].reshape(-1, 3).clone() if info.colour_type == 3 else None
        r["expand"] = timed(lambda: rh.png_expand(raw, info.height, info.width, info.colour_type, info.depth, pal))
        r["png_decode"] = timed(lambda: rh.png_decode(file_dev, info, table))
        r["png_decode_no_crc"] = timed(lambda: rh.png_decode(file_dev, info, table, check_crc=False))
        path = os.path.join(tmp, name + ".png")
        with open(path, "wb") as f:
            f.write(data)
        want = np.asarray(Image.open(path).convert("RGB"))
        assert np.array_equal(container.read_png(path, rh)["image"].cpu().numpy(), want)
        r["read_png_wall"] = wall_ms(lambda: container.read_png(path, rh), args.host_reps)
        r["pillow_open_asarray_upload_wall"] = wall_ms(lambda: (rh.dev(np.asarray(Image.open(path).convert("RGB"))), torch.cuda.synchronize()), args.host_reps)
        out["rows"].append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
