#!/usr/bin/env python3
"""G16: the whole image -> .rhccq script flow (encoder/compression/test.py:77-151) through the CPU oracle's own statement of it,
oracle.rhccq_oracle.script_flow: ROI stage, region lists, segments per region, find_contours' drop rule, levels 1-3, container.

    python tests/golden/make_golden_flow.py            (all cases, a few minutes on one host core)
    python tests/golden/make_golden_flow.py NAME ...   (selected cases)

One file per case, g16_flow_<name>.npz.  Synthetic inputs are stored with the case (no dependence on numpy's generators); PNG
cases store the file name and crop.  The set is chosen to reach every branch of the glue between the stages; `CHECKLIST` states
each branch from the oracle's own intermediates and the run fails if one is not hit.  Written with np.savez_compressed, whose
zip members carry a fixed time stamp: a second run writes identical bytes.

Stored per case (indices as sha256 of their int64 little-endian bytes; palettes in full):
  image / source, qualities      the input
  region_map                     packed bits of get_regions' 0 / 1 region map
  regions                        int64 [R, 8]: call (0 ROI list, 1 non-ROI list), source mask (0 ROI, 1 non-ROI), bbox (4), area,
                                 segment count; norm = normalize_result value; masks = packed bits of every bbox_mask;
                                 labels = uint16 label maps after drops, every region's box flattened and concatenated;
                                 kept / dropped = SLIC ids per region (offsets in kept_off / dropped_off)
  l1_*                           per region: present flag, top_left, shape, palette (offsets), index digest
  l2_*                           per class: present flag (region_quantization did not raise), top_left, shape, palette, digest
  final_*                        top_left, shape, palette, digest, indices dtype; file_bytes = the container bytes
  error                          the exception type name when the flow raises (then nothing else is stored)"""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle import rhccq_oracle as O  # noqa: E402

PREFIX = "g16_flow_"


def _png(name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(HERE, name + ".png")).convert("RGB"), dtype=np.uint8)


def _photo(H, W, seed, sigma=2.0):
    from roibasedimagecompression_amd import synth
    return synth.photo(H, W, seed, sigma=sigma)


def _bands(H, W, top, band, seed):
    """synth.photo with a flat band on top (a full-width rectangle of one SLIC segment: dropped) and a poster band below it"""
    from roibasedimagecompression_amd import synth
    img = synth.photo(H, W, seed)
    img[:top] = (90, 120, 150)
    img[top:top + band] = synth.poster(band, W, 3, cell=4)
    return img


def _patch(H, W, seed, ph, pw, py, px):
    """synth.poster of 16-px cells with a small fine poster patch: a small ROI component moved to the non-ROI list"""
    from roibasedimagecompression_amd import synth
    img = synth.poster(H, W, seed, cell=16)
    img[py:py + ph, px:px + pw] = synth.poster(ph, pw, seed + 100, cell=2)
    return img


# name -> (qualities, how the input is made); "png" inputs are read (and cropped) from this directory, the others are stored
CASES = {
    "lenna": ((20, 10), ("png", "Lenna", None)),
    "kodak1_crop": ((20, 10), ("png", "kodak_1", (0, 384, 0, 600))),            # a 600-px wide region: SLIC's downscale
    "kodak5_crop": ((20, 10), ("png", "kodak_5", (200, 248, 300, 364))),        # no non-ROI region: that call raises
    "bands": ((20, 10), ("synth", lambda: _bands(181, 182, 100, 30, 0))),       # dropped segment, single smaller final component
    "patch": ((20, 10), ("synth", lambda: _patch(162, 246, 476, 5, 15, 2, 98))),  # moved ROI component, two non-ROI layers, < 100 px
    # an ROI component of 486 px: under roi_min_region_size (604, from H * W * 3) but not under the same rule counted on H * W (202)
    "patch_mid": ((20, 10), ("synth", lambda: _patch(125, 161, 85, 17, 15, 2, 126))),
    "line": ((20, 10), ("synth", lambda: _photo(1, 67, 5))),                    # 1-pixel high boxes
    "near_lossless": ((100, 100), ("synth", lambda: _photo(121, 130, 7, sigma=40.0))),   # MiniBatchKMeans, uint16 indices
    "flat": ((20, 10), ("synth", lambda: np.full((96, 128, 3), 120, np.uint8))),
    # one 2 x 49 region of 98 pixels: one segment filling a box of exactly 2 px height, dropped; no component at all, so quantize_image
    # raises IndexError (a drop rule that wanted 3 px would keep it)
    "strip2": ((20, 10), ("synth", lambda: _photo(2, 49, 5))),
}
CHEAP = ("kodak5_crop", "bands", "patch", "patch_mid", "line", "near_lossless", "flat", "strip2")      # re-run by tests/test_flow_oracle_cpu.py


def case_image(name, fixture=None):
    """the input of a case: from the fixture (synthetic cases) or from the PNG in this directory"""
    kind, src = CASES[name][1][0], CASES[name][1][1]
    if kind == "png":
        img = _png(src)
        crop = CASES[name][1][2]
        if crop:
            img = img[crop[0]:crop[1], crop[2]:crop[3]]
        return np.ascontiguousarray(img)
    if fixture is not None:
        return np.ascontiguousarray(fixture["image"])
    return np.ascontiguousarray(src())


def digest(indices):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype="<i8").tobytes()).digest(), np.uint8)


def mbk_native(points, k):
    return O.minibatch_kmeans_native(points, k)[0]


def normalize_margin(nr):
    """distance of a normalize_result value to the nearest integer its ceil can change at (>= 1: ceil(x) <= 0 becomes 1 too)"""
    return abs(nr - max(1, round(nr)))


def run_flow(image, qualities):
    """oracle script_flow with the MiniBatchKMeans restatement in C; also counts the clustering calls of >= 10 000 colours"""
    big = []
    orig = O.cluster_palette

    def counting(quality, palette, indices, *a, **k):
        pal = np.asarray(palette).reshape(-1, 3)
        if int(np.any(pal != 0, axis=1).sum()) >= O.MINIBATCH_THRESHOLD:
            big.append(len(pal))
        return orig(quality, palette, indices, *a, **k)
    O.cluster_palette = counting
    try:
        return O.script_flow(image, qualities[0], qualities[1], minibatch=mbk_native), len(big)
    finally:
        O.cluster_palette = orig


def _comp_arrays(comps):
    present = np.array([c is not None for c in comps], np.uint8)
    tl = np.array([c["top_left"] if c is not None else (0, 0) for c in comps], np.int64).reshape(-1, 2)
    sh = np.array([c["shape"] if c is not None else (0, 0) for c in comps], np.int64).reshape(-1, 2)
    pals = [np.asarray(c["palette"], np.uint8).reshape(-1, 3) if c is not None else np.zeros((0, 3), np.uint8) for c in comps]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pals])]).astype(np.int64)
    dig = np.stack([digest(c["indices"]) if c is not None else np.zeros(32, np.uint8) for c in comps]) if comps else np.zeros((0, 32), np.uint8)
    pal = np.concatenate(pals) if pals else np.zeros((0, 3), np.uint8)
    return present, tl, sh, pal, off, dig


def fixture_arrays(name, image, qualities):
    """run the oracle flow on one case -> (dict of arrays to store, branch facts)"""
    out = {"name": np.array(name), "qualities": np.array(qualities, np.int64)}
    if CASES[name][1][0] == "synth":
        out["image"] = image
    out["image_shape"] = np.array(image.shape, np.int64)
    try:
        r, n_big = run_flow(image, qualities)
    except Exception as e:                                                # noqa: BLE001
        out["error"] = np.array(type(e).__name__)
        return out, {"error": type(e).__name__}
    H, W = image.shape[:2]
    regs = [(0, r) for r in r["roi_regions"]] + [(1, r) for r in r["nonroi_regions"]]
    infos = r["regions"][0] + r["regions"][1]
    tab = np.array([(call, 0 if (call == 0 or reg.get("type") == "nonroi") else 1) + tuple(reg["bbox"]) + (reg["area"], inf["n_segments"])
                    for (call, reg), inf in zip(regs, infos)], np.int64).reshape(-1, 8)
    out["region_map"] = np.packbits(np.asarray(r["region_map"]).astype(bool).reshape(-1))
    out["regions"] = tab
    out["norm"] = np.array([inf["normalize_result"] for inf in infos], np.float64)
    out["masks"] = np.packbits(np.concatenate([np.asarray(reg["bbox_mask"], bool).reshape(-1) for _, reg in regs]) if regs else np.zeros(0, bool))
    out["labels"] = np.concatenate([inf["labels"].reshape(-1) for inf in infos]).astype(np.uint16) if infos else np.zeros(0, np.uint16)
    for key in ("kept", "dropped"):
        out[key] = np.array([s for inf in infos for s in inf[key]], np.int64)
        out[key + "_off"] = np.concatenate([[0], np.cumsum([len(inf[key]) for inf in infos])]).astype(np.int64)
    l1 = [(comps[0] if comps else None) for cls in r["level1"] for comps in cls]
    for pre, comps in (("l1_", l1), ("l2_", r["level2"])):
        present, tl, sh, pal, off, dig = _comp_arrays(comps)
        out.update({pre + "present": present, pre + "top_left": tl, pre + "shape": sh, pre + "palette": pal, pre + "palette_off": off,
                    pre + "digest": dig})
    out["l2_error"] = np.array([e or "" for e in r["level2_error"]])
    fin = r["final"]
    out["final_top_left"] = np.array(fin["top_left"], np.int64)
    out["final_shape"] = np.array(fin["shape"], np.int64)
    out["final_palette"] = np.asarray(fin["palette"], np.uint8).reshape(-1, 3)
    out["final_digest"] = digest(fin["indices"])
    out["final_dtype"] = np.array(fin["indices_dtype"])
    out["file_bytes"] = np.frombuffer(r["file_bytes"], np.uint8)
    # branch facts, from the oracle's intermediates
    facts = {"moved_overlapping": 0, "under_100": 0, "dropped": 0, "thin": 0, "downscale": 0, "caught": 0, "palette_u16": 0,
             "palette_u8": 0, "final_smaller": 0, "minibatch": n_big, "odd_h": H % 2, "w_not_4": int(W % 4 != 0)}
    for call in (0, 1):
        painted = []
        for (c, reg), inf in zip(regs, infos):
            if c != call:
                continue
            minr, minc, maxr, maxc = reg["bbox"]
            m = np.zeros((H, W), bool)
            m[minr:maxr, minc:maxc] = reg["bbox_mask"]
            if call == 1 and reg.get("type") == "nonroi" and any((p & m).any() for p in painted):
                facts["moved_overlapping"] += 1
            p = np.zeros((H, W), bool)
            p[minr:maxr, minc:maxc] = inf["labels"] > 0
            painted.append(p)
            facts["under_100"] += int(np.sum(reg["bbox_mask"]) < 100)
            facts["dropped"] += len(inf["dropped"])
            facts["thin"] += int(min(maxr - minr, maxc - minc) == 1)
            facts["downscale"] += int(round(500 / max(maxr - minr, maxc - minc, 3), 1) < 1)
    facts["caught"] = sum(e is not None for e in r["level2_error"])
    facts["palette_u16"] = int(len(fin["palette"]) > 256)
    facts["palette_u8"] = int(len(fin["palette"]) <= 256)
    facts["final_smaller"] = int(tuple(fin["shape"]) != (H, W))
    facts["min_margin"] = min((normalize_margin(v) for v in out["norm"]), default=1.0)
    return out, facts


CHECKLIST = [
    ("small ROI component moved to the non-ROI list, overlapping a painted non-ROI region (two non-ROI layers)", "moved_overlapping"),
    ("region with fewer than 100 masked pixels", "under_100"),
    ("dropped segment (fills its box of at least 2 x 2)", "dropped"),
    ("region box 1 pixel high or wide", "thin"),
    ("region whose longest side forces the SLIC downscale", "downscale"),
    ("call without segments: region_quantization raised and was caught", "caught"),
    ("final palette above 256 entries (uint16 indices)", "palette_u16"),
    ("final palette of at most 256 entries (uint8 indices)", "palette_u8"),
    ("final result one component smaller than the image", "final_smaller"),
    ("MiniBatchKMeans branch (>= 10 000 colours)", "minibatch"),
    ("odd image height", "odd_h"),
    ("image width not a multiple of 4", "w_not_4"),
    ("flat image: the flow raises", "error"),
]


def main(names):
    facts = {}
    for name in names:
        t0 = time.perf_counter()
        q = CASES[name][0]
        img = case_image(name)
        arrays, f = fixture_arrays(name, img, q)
        facts[name] = f
        path = os.path.join(HERE, PREFIX + name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"{name}: {img.shape[0]}x{img.shape[1]} q={q} {os.path.getsize(path)} bytes in {time.perf_counter() - t0:.1f} s "
              f"{json.dumps(f, default=float)}", flush=True)
    if set(names) != set(CASES):
        return
    missing = []
    print("branch checklist:")
    for text, key in CHECKLIST:
        who = [n for n, f in facts.items() if f.get(key)]
        print(f"  [{'x' if who else ' '}] {text}: {', '.join(who) or '-'}")
        if not who:
            missing.append(text)
    margin = min(f.get("min_margin", 1.0) for f in facts.values())
    print(f"smallest normalize_result margin to an integer: {margin:.6g}")
    assert not missing, missing
    assert margin > 1e-6, margin


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
