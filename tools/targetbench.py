"""The palette ladder and the targets on it (csrc/palette_ladder.hip, ImageEncoder.ladder, encode_with_palette(target_bytes= /
target_psnr=)) on the 4K Kodak mosaic of tools/remapbench.py, in ONE process, the frame resident on the device:
  (a) the three kernels alone (HIP events around the launches, buffers allocated before) at K = the palette of encode (230 rows on this
      image), 1 024 and the device cap: rhccq_palette_moments with one table and with three, rhccq_palette_curve over a log to one row,
      rhccq_palette_rung to K / 2 and to 16; beside them ONE iteration of rhccq_palette_refine and one rhccq_palette_remap at the same
      K: the nearest existing kernels (the same search with one accumulator field fewer and one table, and with none).
  (b) ImageEncoder.ladder(image, palette): wall time.
  (c) encode_with_palette(target_bytes=B) at two targets (fractions of the full palette's file), and as a yardstick the same bisection
      written with what the parent commit has: encode_with_palette(colours=k, out_path=...) per probe, the same probe sequence.
  (d) encode_with_palette(target_psnr=P) at two targets, beside one encode_with_palette(colours=k) of the rung it picks.
Medians of --reps runs after a warm-up of every shape; compared variants alternate.  The times are reported, not gated.  Exits
non-zero (the JSON is written all the same) when the search and the per-probe loop disagree on k or on the file size.

    python tools/targetbench.py [--reps 5] [--out profiles/palette_target.json]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
BYTE_FRACTIONS = (0.8, 0.5)
PSNR_DROPS = (1.0, 4.0)                    # dB below the full palette's PSNR


def png(name):
    return np.asarray(Image.open(os.path.join(G, name + ".png")).convert("RGB"), dtype=np.uint8)


def wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def runs(ts, unit="s", digits=5):
    return {f"median_{unit}": round(statistics.median(ts), digits), f"runs_{unit}": [round(v, digits) for v in ts]}


def kernels(rh, rgb, pal, reps):
    """(a): every launch sequence alone, on buffers allocated before"""
    K, n = int(pal.shape[0]), rgb.numel() // 3
    cls = (torch.arange(n, device=rh.device) % 3 == 0).to(torch.uint8)                   # a third of the pixels in class 1
    idx = rh.empty((n,), torch.uint8 if K <= 256 else torch.int16)
    mom1, mom3 = rh.empty((1, K, 5), torch.int64), rh.empty((3, K, 5), torch.int64)
    sums = rh.empty((1, 2), torch.int64)
    rpal, hist, nit = pal.clone(), rh.empty((1, 2), torch.int64), rh.empty((1,), torch.int32)
    rwork = rh.empty((int(rh._raw.rhccq_palette_refine_bytes(K)) // 8,), torch.int64)
    rh.palette_moments(rgb, pal, cls, 2)
    _, m3 = rh.palette_moments(rgb, pal, cls, 2)
    counts = (m3[2, :, 0] + 1).contiguous()                                              # + 1: every row lives, K - 1 steps
    _, _, _, merges = rh.palette_reduce(pal, counts, 1)
    log = torch.full((max(K - 1, 1), 2), -1, dtype=torch.int32, device=rh.device)
    log[:merges.shape[0]] = merges
    cbytes = int(rh._raw.rhccq_palette_curve_bytes(K, 3))
    cwork, curve = rh.empty((cbytes // 8,), torch.int64), rh.empty((3, K), torch.int64)
    pal_out, cnt_out, map_, k_out = rh.empty((K, 3), torch.uint8), rh.empty((K,), torch.int64), rh.empty((K,), torch.int32), rh.empty((1,), torch.int32)
    lib, ctx, p = rh.lib, rh.ctx, rh._p
    calls = {
        "remap": lambda: lib.rhccq_palette_remap(ctx, p(rgb), n, p(pal), K, p(None), 0, p(idx), idx.element_size(), p(sums)),
        "refine_1_iteration": lambda: lib.rhccq_palette_refine(ctx, p(rgb), n, p(rpal), K, p(None), 0, None, 1, p(rwork), rwork.numel() * 8, p(hist), p(nit)),
        "moments_1_table": lambda: lib.rhccq_palette_moments(ctx, p(rgb), n, p(pal), K, p(None), 0, p(idx), idx.element_size(), p(mom1)),
        "moments_3_tables": lambda: lib.rhccq_palette_moments(ctx, p(rgb), n, p(pal), K, p(cls), 2, p(idx), idx.element_size(), p(mom3)),
        "curve_3_tables": lambda: lib.rhccq_palette_curve(ctx, p(pal), p(counts), K, p(log), p(m3), 3, p(cwork), cbytes, p(curve)),
        "rung_half": lambda: lib.rhccq_palette_rung(ctx, p(pal), p(counts), K, p(log), max(K // 2, 1), p(pal_out), p(cnt_out), p(map_), p(k_out)),
        "rung_16": lambda: lib.rhccq_palette_rung(ctx, p(pal), p(counts), K, p(log), min(16, K), p(pal_out), p(cnt_out), p(map_), p(k_out)),
    }
    ms = {name: [] for name in calls}
    for rep in range(reps + 1):                                                          # (rep 0: the warm-up of this shape)
        for name, call in calls.items():
            def checked():
                rh._check(call(), name)
            if name == "refine_1_iteration":
                rpal.copy_(pal)
            dt = events(checked)
            if rep:
                ms[name].append(dt)
    from roibasedimagecompression_amd import ops
    row = {"K": K, "steps": int(merges.shape[0]), "moments_in_lds": {"1_table": K <= ops.palette_moments_lds_rows(0), "3_tables": K <= ops.palette_moments_lds_rows(2)}}
    row.update({name: runs(v, "ms", 4) for name, v in ms.items()})
    row["curve_us_per_step"] = round(statistics.median(ms["curve_3_tables"]) * 1000.0 / max(int(merges.shape[0]), 1), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "palette_target.json"))
    args = ap.parse_args()
    from roibasedimagecompression_amd import ops, synth
    from roibasedimagecompression_amd.image import ImageEncoder
    img = synth.kodak_mosaic([png(f"kodak_{i}") for i in range(1, 21)])
    H, W = img.shape[:2]
    enc = ImageEncoder()
    rh, dev = enc.rh, enc.rh.device
    cap = ops.palette_reduce_max_rows()
    rgb = rh.dev(img)                                                                    # resident: everything below reads this tensor
    pal = np.asarray(enc.encode(img, 20, 10)["palette"], np.uint8).reshape(-1, 3)
    d_pal = rh.dev(pal)
    out = {"tool": "tools/targetbench.py", "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "reps": args.reps, "image": "kodak_mosaic",
           "shape": [H, W], "qualities": [20, 10], "palette_size": len(pal), "max_rows": cap,
           "inputs": "resident device tensors (the frame is uploaded once before the timed loops)", "kernels": []}

    rng = np.random.default_rng(1)
    flat = img.reshape(-1, 3)
    for K in (len(pal), 1024, cap):
        p = d_pal if K == len(pal) else rh.dev(flat[rng.integers(0, len(flat), K)])
        out["kernels"].append(kernels(rh, rgb.reshape(-1, 3), p, args.reps))

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "x.rhccq")
        full = enc.encode_with_palette(rgb, d_pal, out_path=path)
        full_bytes, full_psnr = os.path.getsize(path), full["stats"]["remap"]["all"]["psnr"]
        out["full_palette"] = {"rhccq_bytes": full_bytes, "psnr": full_psnr}
        enc.ladder(rgb, d_pal)
        out["ladder"] = runs([wall(lambda: enc.ladder(rgb, d_pal), dev)[0] for _ in range(args.reps)])
        L = enc.ladder(rgb, d_pal)
        out["ladder"].update(rungs=len(L["colours"]), psnr_bound_top=L["psnr_bound"]["all"][0], psnr_bound_16=L["psnr_bound"]["all"][-16] if len(L["colours"]) >= 16 else None)

        def loop(B, ks):
            """the same bisection with colours=k and a file per probe; ks: the probe sequence the search took"""
            sizes = []
            for k in ks:
                enc.encode_with_palette(rgb, d_pal, colours=k, out_path=path)
                sizes.append((k, os.path.getsize(path)))
            return sizes
        failures = []
        out["target_bytes"] = []
        for frac in BYTE_FRACTIONS:
            B = int(full_bytes * frac)
            res = enc.encode_with_palette(rgb, d_pal, target_bytes=B, out_path=path)     # warm-up; the probe sequence
            tg = res["stats"]["target"]
            ks = [k for k, _ in tg["probes"]]
            loop(B, ks)
            ts, tl = [], []
            for _ in range(args.reps):
                dt, res = wall(lambda: enc.encode_with_palette(rgb, d_pal, target_bytes=B, out_path=path), dev)
                ts.append(dt)
                dt, sizes = wall(lambda: loop(B, ks), dev)
                tl.append(dt)
            tg = res["stats"]["target"]
            if [tuple(x) for x in tg["probes"]] != sizes:
                failures.append(f"target_bytes={B}: the search probed {tg['probes']}, the loop {sizes}")
            out["target_bytes"].append({"fraction": frac, "target": B, "met": tg["met"], "colours": tg["colours"], "probes": tg["probes"],
                                        "psnr": res["stats"]["remap"]["all"]["psnr"], "bound_psnr": tg["bound_psnr"]["all"],
                                        "search": runs(ts), "loop_of_colours_k": runs(tl), "seconds": res["stats"]["seconds"]})
        out["target_psnr"] = []
        for drop in PSNR_DROPS:
            P = full_psnr - drop
            res = enc.encode_with_palette(rgb, d_pal, target_psnr=P)
            k = res["stats"]["target"]["colours"]
            enc.encode_with_palette(rgb, d_pal, colours=k)
            ts, tc = [], []
            for _ in range(args.reps):
                dt, res = wall(lambda: enc.encode_with_palette(rgb, d_pal, target_psnr=P), dev)
                ts.append(dt)
                dt, same = wall(lambda: enc.encode_with_palette(rgb, d_pal, colours=k), dev)
                tc.append(dt)
            tg = res["stats"]["target"]
            if not np.array_equal(res["palette"], same["palette"]):
                failures.append(f"target_psnr={P}: the palette is not that of colours={k}")
            out["target_psnr"].append({"drop_db": drop, "target": P, "met": tg["met"], "colours": k, "psnr": res["stats"]["remap"]["all"]["psnr"],
                                       "bound_psnr": tg["bound_psnr"]["all"], "call": runs(ts), "one_colours_k_call": runs(tc),
                                       "seconds": res["stats"]["seconds"]})
    out["failures"] = failures
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if failures:
        sys.exit("; ".join(failures))


if __name__ == "__main__":
    main()
