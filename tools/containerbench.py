"""The .rhccq container on the device (container.py, csrc/zlib_deflate.hip) against the host path, in ONE process.

  python tools/containerbench.py [--reps N] [--out profiles/r05_container.json]

Inputs: the configs[1] frame (synth.photo(2160, 3840, 1234), classes synth.frame_classes(H, W, (2, 1)), q = 20 / 20, through
FrameEncoder.encode_native: a uint16 index map of 16.6 MB) and the index maps of the 36 reference artefacts in tests/golden.
Device time is taken with HIP events on the context stream around the zlib calls (median of --reps after one warm-up):
  index stream, palette, outer layer (the pickle of the finished package), and their sum;
plus the wall time of container.write_frame (narrowing, all three layers, the read-backs, the pickle and the file write) and of the
host path lossless_compress_optimized + save_compressed on the same frame.  Sizes are compared with zlib levels 9 and 1."""
import argparse
import glob
import json
import os
import pickle
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dev_ms(rh, t, reps):
    """median device time (ms) of one zlib stream of tensor t, HIP events on the current stream; -> (ms, stream bytes)"""
    s = torch.cuda.current_stream(rh.device)
    out, n = rh.zlib_compress_async(t)                     # warm-up (code objects, allocator)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        out, n = rh.zlib_compress_async(t)
        b.record(s)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), int(n.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_container.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import synth
    from roibasedimagecompression_amd.api.compression import lossless_compress_optimized, save_compressed
    from roibasedimagecompression_amd.api.uncompression import load_compressed
    from roibasedimagecompression_amd.container import lossless_compress_device, narrow_indices, write_frame
    from roibasedimagecompression_amd.frame import ClassSpec, FrameEncoder
    from roibasedimagecompression_amd.ops import Rhccq
    rh = Rhccq(0)
    rep = {"device": torch.cuda.get_device_name(0), "reps": args.reps}

    H, W = 2160, 3840
    img = synth.photo(H, W, 1234)
    (lr, nr, br), (ln, nn, bn) = synth.frame_classes(H, W, (2, 1))
    specs = [ClassSpec(torch.from_numpy(lr).to(rh.device), np.zeros(nr, np.int64), [br], 20),
             ClassSpec(torch.from_numpy(ln).to(rh.device), np.zeros(nn, np.int64), [bn], 20)]
    res = FrameEncoder(rh).encode_native(torch.from_numpy(img).to(rh.device), specs)
    idx_dev, name = narrow_indices(res["indices"], rh)
    pal_dev = rh.dev(np.asarray(res["palette"], np.uint8).reshape(-1))
    pkg = lossless_compress_device(res["palette"], res["indices"], res["shape"], rh)
    body_raw = pickle.dumps(pkg, protocol=5)
    body_dev = rh.dev(np.frombuffer(body_raw, np.uint8).copy())
    t_i, n_i = dev_ms(rh, idx_dev, args.reps)
    t_p, n_p = dev_ms(rh, pal_dev, args.reps)
    t_o, n_o = dev_ms(rh, body_dev, args.reps)
    tmp = tempfile.mkdtemp()
    fn_dev, fn_host = os.path.join(tmp, "dev.rhccq"), os.path.join(tmp, "host.rhccq")
    write_frame(res, fn_dev, rh)                           # warm-up
    wall = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        size_dev = write_frame(res, fn_dev, rh)
        wall.append((time.perf_counter() - t0) * 1e3)
    idx_host = res["indices"].cpu().numpy().view(np.uint16).reshape(-1)
    t0 = time.perf_counter()
    hpkg = lossless_compress_optimized(res["palette"], idx_host, res["shape"])
    t1 = time.perf_counter()
    size_host = save_compressed(hpkg, fn_host)
    t2 = time.perf_counter()
    back = load_compressed(fn_dev)
    assert zlib.decompress(back["i"]) == zlib.decompress(hpkg["i"]) and zlib.decompress(back["p"]) == zlib.decompress(hpkg["p"])
    raw = zlib.decompress(hpkg["i"])
    l1 = len(zlib.compress(raw, 1))
    rep["configs1_frame"] = {
        "index_map": f"{H}x{W} {name}, {idx_dev.numel()} bytes, {len(res['palette'])} colours",
        "device_ms": {"index_stream": round(t_i, 3), "palette": round(t_p, 3), "outer_layer": round(t_o, 3), "sum": round(t_i + t_p + t_o, 3)},
        "index_stream_GBps": round(idx_dev.numel() / t_i / 1e6, 3),
        "write_frame_wall_ms_median": round(statistics.median(wall), 2),
        "host_ms": {"lossless_compress_optimized": round((t1 - t0) * 1e3, 1), "save_compressed": round((t2 - t1) * 1e3, 1),
                    "sum": round((t2 - t0) * 1e3, 1)},
        "bytes": {"index_stream_device": n_i, "index_stream_level9": len(hpkg["i"]), "index_stream_level1": l1,
                  "device_vs_level9": round(n_i / len(hpkg["i"]), 4), "device_vs_level1": round(n_i / l1, 4),
                  "file_device": size_dev + 1, "file_host": size_host + 1},
    }
    print(json.dumps(rep["configs1_frame"]), flush=True)

    maps, tot_dev, tot_9, tot_1, tot_ms, tot_in = [], 0, 0, 0, 0.0, 0
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.rhccq"))):
        p = load_compressed(f)
        raw = zlib.decompress(p["i"])
        ms, n = dev_ms(rh, rh.dev(np.frombuffer(raw, np.uint8).copy()), args.reps)
        l1 = len(zlib.compress(raw, 1))
        maps.append({"file": os.path.basename(f), "bytes_in": len(raw), "device": n, "level9": len(p["i"]), "level1": l1,
                     "device_vs_level9": round(n / len(p["i"]), 4), "device_ms": round(ms, 3), "GBps": round(len(raw) / ms / 1e6, 3)})
        tot_dev, tot_9, tot_1, tot_ms, tot_in = tot_dev + n, tot_9 + len(p["i"]), tot_1 + l1, tot_ms + ms, tot_in + len(raw)
    rep["reference_maps"] = {"n": len(maps), "device_vs_level9": round(tot_dev / tot_9, 4), "device_vs_level1": round(tot_dev / tot_1, 4),
                             "worst_vs_level9": max(m["device_vs_level9"] for m in maps), "device_ms_sum": round(tot_ms, 2),
                             "GBps_overall": round(tot_in / tot_ms / 1e6, 3), "maps": maps}
    print(json.dumps({k: v for k, v in rep["reference_maps"].items() if k != "maps"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rep, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
