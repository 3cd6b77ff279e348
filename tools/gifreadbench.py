"""Reading a GIF file on the device (csrc/gif_read.hip) under the other file tools' conditions: ONE process, the file and its tables
resident, HIP events around --inner calls, medians of --reps windows after a warm-up of every shape.  The files:
  mosaic4k_own_16 / _256       the 4K Kodak mosaic of tools/imagebench.py as the project writes it (a Clear every 16 384 pixels);
  mosaic4k_pillow_16 / _256    the same index maps written by Pillow (interlaced, a Clear where the table fills);
  noise4k_own_256              uniform noise of the same size over 256 colours, the project's writer (a Clear wherever the table fills);
  mosaic4k_one_segment_256     the same pixels as ONE segment: no Clear behind the first, 12-bit codes behind the full table (slow Python
                               writes it once);
  clip1080p_own / _pillow      64 1080p frames cut from the mosaic (a window that slides 8 pixels a frame), 256 colours, both writers;
  small_256x256 / _480x640     crops, the project's writer.
Per file: its segments, Rhccq.gif_decode (join, scan, plan, lengths, offsets, emit, compose on one stream), by the wall clock
container.read_gif beside Image.open + seek + convert("RGB") + upload on one host core, and beside rhccq_gif_decode_host (the serial
form), medians of --host-reps calls each; and Rhccq.gif_decode with a segment's chains resolved by pointer doubling and in order
(RHCCQ_OPT_GIF_READ_CHAIN) on a flat frame, on the noise and on the photograph's files, alternating.  The split of gif_decode into
its launches comes from a kernel trace of this tool: `rocprofv3 --kernel-trace -d DIR -o gifread -- python tools/gifreadbench.py
--trace-only` runs every decode once after its warm-up, and `--trace DIR/gifread_results.db` folds the launches' durations into the
output as "kernel_trace" and, a row a file, "launches_us".

    python tools/gifreadbench.py [--reps 5] [--inner 3] [--frames 64] [--host-reps 5] [--out profiles/gif_read.json]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ditherbench import png, window_ms  # noqa: E402
from gifbench import pillow_save, row  # noqa: E402


def kernel_trace(db_path):
    """the reader's kernels of a rocprofv3 results database -> [{kernel, workgroups, launches, min_us, median_us, max_us}]"""
    import sqlite3
    db = sqlite3.connect(db_path)
    groups = {}
    for name, groups_x, ns in db.execute("select name, grid_x / workgroup_x, duration from kernels where name like '%rhccq::gifr::%'"):
        short = name.split("rhccq::gifr::")[1].split("(")[0]
        groups.setdefault((short, int(groups_x)), []).append(ns / 1e3)
    return [{"kernel": k, "workgroups": g, "launches": len(v), "min_us": round(min(v), 1), "median_us": round(statistics.median(v), 1),
             "max_us": round(max(v), 1)} for (k, g), v in sorted(groups.items())]


LAUNCHES = ("join_kernel", "scan_kernel", "plan_kernel", "segments_kernel<false>", "offsets_kernel", "segments_kernel<true>", "finish_kernel", "compose_kernel")


def launches_per_decode(db_path, names):
    """a --trace-only run decodes every file twice, in the order of `names`: the second decode's launches in microseconds, a row a file
    (None when the trace does not have that shape)"""
    import sqlite3
    db = sqlite3.connect(db_path)
    try:
        rows = db.execute("select name, duration from kernels where name like '%rhccq::gifr::%' order by start").fetchall()
    except sqlite3.Error:
        return None
    short = [n.split("rhccq::gifr::")[1].split("(")[0] for n, _ in rows]
    k = len(LAUNCHES)
    if len(rows) != 2 * k * len(names) or any(tuple(short[i:i + k]) != LAUNCHES for i in range(0, len(rows), k)):
        return None
    return [dict({"file": name}, **{LAUNCHES[j]: round(rows[(2 * i + 1) * k + j][1] / 1e3, 1) for j in range(k)}) for i, name in enumerate(names)]


def one_segment_file(idx, pal):
    """idx uint8[H, W], pal uint8[256, 3] -> a GIF whose only Clear opens the stream"""
    import gifread_cases as R
    H, W = idx.shape
    tokens = R.lzw_tokens(idx.reshape(-1).tolist(), 8, clear="never")
    return R.build(W, H, [R.image((0, 0, W, H), R.stream_of(tokens, 8), 8)], gtable=pal)


def pillow_read(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    return np.stack([np.asarray((im.seek(f), im.convert("RGB"))[1]) for f in range(getattr(im, "n_frames", 1))])


def wall(fn, reps):
    t, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return row(t), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--trace", default=None, help="a rocprofv3 results database of a --trace-only run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gif_read.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import _lib, container, ops, synth
    from roibasedimagecompression_amd.image import ImageEncoder
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh, dev = enc.rh, enc.rh.device
    rgb = rh.dev(img)
    files = {}
    for colours in (16, 256):
        res = enc.quantize(rgb, colours=colours)
        pal = np.asarray(res["palette"], np.uint8).reshape(-1, 3)
        idx = res["indices"].reshape(-1).contiguous()
        files[f"mosaic4k_own_{colours}"] = rh.gif_encode(idx, 1, H, W, rh.dev(pal))
        host = idx.cpu().numpy().reshape(1, H, W)
        files[f"mosaic4k_pillow_{colours}"] = pillow_save(host, pal)
        if colours == 256:
            full = np.zeros((256, 3), np.uint8)
            full[:len(pal)] = pal
            t0 = time.perf_counter()
            files["mosaic4k_one_segment_256"] = one_segment_file(host[0], full)
            print(f"one-segment file written in {time.perf_counter() - t0:.1f} s", flush=True)
            noise = torch.randint(0, 256, (H * W,), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
            files["noise4k_own_256"] = rh.gif_encode(noise, 1, H, W, rh.dev(full))
            for sh, sw in ((256, 256), (480, 640)):
                small = res["indices"].reshape(H, W)[700:700 + sh, 900:900 + sw].contiguous().reshape(-1)
                files[f"small_{sh}x{sw}"] = rh.gif_encode(small, 1, sh, sw, rh.dev(pal))
    B, h, w = args.frames, 1080, 1920
    clip = torch.stack([rgb[4 * f:4 * f + h, 8 * f:8 * f + w] for f in range(B)]).contiguous()
    shared = enc.shared_palette(list(clip), 255)
    K = int(shared.shape[0])
    off = (np.arange(B + 1) * (h * w)).astype(np.int64)
    cidx, _ = rh.palette_remap_batch(clip.reshape(-1, 3), off, shared.unsqueeze(0).expand(B, K, 3).contiguous(), torch.full((B,), K, dtype=torch.int32, device=dev))
    files["clip1080p_own"] = rh.gif_encode(cidx, B, h, w, shared)
    files["clip1080p_pillow"] = pillow_save(cidx.cpu().numpy().reshape(B, h, w), shared.cpu().numpy())
    del clip, cidx
    out = {"tool": "tools/gifreadbench.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "reps": args.reps, "inner_calls": args.inner,
           "host_reps": args.host_reps, "image": "kodak_mosaic", "shape": [H, W], "clip": [B, h, w],
           "geometry": {"tile_codes": ops.gif_read_tile(), "threads": ops.gif_read_threads()},
           "inputs": "the file, its frame table and its sub-block table are parsed once; gif_decode uploads the tables and allocates outputs and workspace inside the call",
           "rows": []}
    lib = _lib.load()
    for name, data in files.items():
        parsed = ops.gif_parse(data)
        info, frames, blocks = parsed
        assert info.status == 0, (name, info.status)
        file_dev = rh.dev(np.frombuffer(data, np.uint8).copy())
        ws = C.c_int64()
        lib.rhccq_gif_read_sizes(C.byref(info), len(data), C.byref(ws))
        whole = rh.gif_decode(file_dev, parsed)
        status, head = rh.to_host(whole["status"], whole["head"])
        assert status.tolist() == [0, 0], (name, status)
        r = {"file": name, "file_bytes": len(data), "frames": info.n_frames, "screen": [info.height, info.width], "pixels": info.pixels,
             "stream_bytes": sum(frames[f].stream_bytes for f in range(info.n_frames)), "sub_blocks": info.n_blocks, "segments": int(head[2]),
             "interlaced": bool(frames[0].interlace), "segment_table_rows": info.seg_rows, "workspace_bytes": ws.value}
        del whole
        if args.trace_only:
            rh.gif_decode(file_dev, parsed)
            torch.cuda.synchronize()
            out["rows"].append(r)
            continue
        r["gif_decode"] = row([window_ms(lambda: rh.gif_decode(file_dev, parsed), args.inner) for _ in range(args.reps)])
        r["decode_ns_per_pixel"] = round(r["gif_decode"]["median_ms"] * 1e6 / info.pixels, 4)
        r["read_gif_wall"], got = wall(lambda: container.read_gif(data, rh), args.host_reps)
        r["pillow_open_seek_convert_upload_wall"], want = wall(lambda: rh.dev(pillow_read(data)), args.host_reps)
        r["equals_pillow"] = bool(torch.equal(got["images"], want))
        del got, want
        F, HH, WW = info.n_frames, info.height, info.width
        host_rgb, st = np.empty(F * HH * WW * 3, np.uint8), np.zeros(2, np.int32)
        a = np.frombuffer(data, np.uint8)

        def host_form():
            assert lib.rhccq_gif_decode_host(C.c_void_p(a.ctypes.data), len(a), C.c_void_p(host_rgb.ctypes.data), None, None, C.c_void_p(st.ctypes.data)) == 0
        r["decode_host_wall"], _ = wall(host_form, args.host_reps)
        out["rows"].append(r)
        print(json.dumps(r), flush=True)
    if not args.trace_only:
        # a segment's len / first chains: pointer doubling (the default) against one lane's pass in order (RHCCQ_OPT_GIF_READ_CHAIN), on
        # a flat frame (ONE segment, a chain 4 091 entries deep) and on the photograph's files (many segments, shallow chains)
        import gifread_cases as R
        out["chain_ab"] = []
        for name, data in (("flat_2900x2900", R.case("flat_deep")), ("noise4k_own_256", files["noise4k_own_256"]), ("mosaic4k_own_256", files["mosaic4k_own_256"]),
                           ("mosaic4k_pillow_16", files["mosaic4k_pillow_16"]), ("clip1080p_own", files["clip1080p_own"])):
            parsed = ops.gif_parse(data)
            file_dev = rh.dev(np.frombuffer(data, np.uint8).copy())
            r = {"file": name}
            for key, value in (("doubling", 0), ("in_order", 1), ("doubling_again", 0)):
                rh.set_option(rh.OPT_GIF_READ_CHAIN, value)
                assert rh.to_host(rh.gif_decode(file_dev, parsed)["status"]).tolist() == [0, 0]
                r[key] = row([window_ms(lambda: rh.gif_decode(file_dev, parsed), args.inner) for _ in range(args.reps)])
            rh.set_option(rh.OPT_GIF_READ_CHAIN, 0)
            out["chain_ab"].append(r)
            print(json.dumps(r), flush=True)
    if args.trace:
        out["kernel_trace"] = kernel_trace(args.trace)
        per_file = launches_per_decode(args.trace, list(files))
        if per_file:
            out["launches_us"] = per_file
    if args.out and not args.trace_only:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
