"""kmeansbench.py -- the one-workgroup and the wide Lloyd path of rhccq_kmeans on lone problems (RHCCQ_OPT_KMEANS_WIDE_PAIRS,
RHCCQ_OPT_KMEANS_CHUNK; csrc/k7_kmeans.hip, csrc/km_wide_host.h).

Sizes: n different colours of the full cube, n in 500 ... 10 240, k = n / 10, and the large node of the first split round of the 4K bench
frame (caught from the Python host's Rhccq.kmeans_split call on that frame; --no-frame leaves it out).  Each problem runs alone through
Rhccq.kmeans_split with the pair count at 0 (one workgroup) and at 1 (wide) at every --chunks length: --reps timed calls behind --warmup,
wall clock around the call (its uploads, the launches, the host's reads of the state records, the download of the labels), interleaved
path by path; labels and (n_iter, strict, relocated) of every wide run must equal the one-workgroup run's.  Reported per size: the median
and max - min of each setting, and whether the wide path at its best chunk length wins by more than the larger of the two spreads.

    python tools/kmeansbench.py [--reps 15] [--warmup 3] [--chunks 4,8,16,32] [--no-frame] [--out profiles/kmeans_wide.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from roibasedimagecompression_amd.ops import Rhccq

SIZES = (500, 1000, 2000, 3883, 7000, 10240)


def colours(n, seed):
    rng = np.random.default_rng(seed)
    pick = rng.choice(1 << 24, n, replace=False)
    return pick.astype(np.uint32)


def frame_node(rh):
    """the largest problem of the first KMeans split round of the bench frame"""
    import bench
    from roibasedimagecompression_amd.frame import FrameEncoder
    _, rgb, specs, _, _ = bench.build_inputs(rh, 2160, 3840, 1234, (2, 1), 20, 20, 2.0)
    caught = []
    plain = rh.kmeans_split

    def spy(key_list, k_list, return_info=False):
        caught.append(max(zip(key_list, k_list), key=lambda kv: len(kv[0])))
        return plain(key_list, k_list, return_info)
    rh.kmeans_split = spy
    try:
        FrameEncoder(rh).encode(rgb, specs)
    finally:
        del rh.kmeans_split
    keys, k = max(caught, key=lambda kv: len(kv[0]))
    return np.ascontiguousarray(keys).astype(np.uint32), int(k)


def timed(rh, keys, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    labs, info = rh.kmeans_split([keys], [k], return_info=True)
    return (time.perf_counter() - t0) * 1e3, labs[0], tuple(int(v) for v in info[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunks", default="4,8,16,32")
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    chunks = [int(c) for c in args.chunks.split(",")]
    rh = Rhccq(0)
    problems = [(f"n{n}", colours(n, n), n // 10) for n in SIZES]
    if not args.no_frame:
        keys, k = frame_node(rh)
        problems.append((f"frame_node_n{len(keys)}_k{k}", keys, k))
    settings = [("one_workgroup", 0, chunks[0])] + [(f"wide_chunk{c}", 1, c) for c in chunks]
    rows = []
    for name, keys, k in problems:
        ms = {s[0]: [] for s in settings}
        ref = None
        for rep in range(args.warmup + args.reps):
            for label, pairs, chunk in settings:
                rh.set_option(Rhccq.OPT_KMEANS_WIDE_PAIRS, pairs)
                rh.set_option(Rhccq.OPT_KMEANS_CHUNK, chunk)
                t, lab, info = timed(rh, keys, k)
                assert info[3] == pairs, (name, label, info)
                if ref is None:
                    ref = (lab.copy(), info[:3])
                assert np.array_equal(lab, ref[0]) and info[:3] == ref[1], (name, label, info, ref[1])
                if rep >= args.warmup:
                    ms[label].append(t)
        stat = {l: {"median_ms": float(np.median(v)), "max_minus_min_ms": float(max(v) - min(v)), "min_ms": float(min(v))} for l, v in ms.items()}
        best = min((l for l in stat if l != "one_workgroup"), key=lambda l: stat[l]["median_ms"])
        gain = stat["one_workgroup"]["median_ms"] - stat[best]["median_ms"]
        spread = max(stat["one_workgroup"]["max_minus_min_ms"], stat[best]["max_minus_min_ms"])
        row = {"problem": name, "n": int(len(keys)), "k": int(k), "pairs": int(len(keys)) * int(k), "n_iter": ref[1][0], "strict": ref[1][1],
               "settings": stat, "best_wide": best, "gain_ms": gain, "spread_ms": spread, "wide_wins": bool(gain > spread)}
        rows.append(row)
        print(f"{name:28s} n_iter {ref[1][0]:3d}  one workgroup {stat['one_workgroup']['median_ms']:7.3f} ms (+-{stat['one_workgroup']['max_minus_min_ms']:.3f})  " +
              "  ".join(f"C={c}: {stat[f'wide_chunk{c}']['median_ms']:7.3f} (+-{stat[f'wide_chunk{c}']['max_minus_min_ms']:.3f})" for c in chunks) +
              f"  -> {'wide wins' if row['wide_wins'] else 'no win'} by {gain:.3f} ms", flush=True)
    rh.set_option(Rhccq.OPT_KMEANS_WIDE_PAIRS, 0)
    result = {"cmd": "python tools/kmeansbench.py " + " ".join(sys.argv[1:]), "reps": args.reps, "warmup": args.warmup,
              "what": "wall clock of one Rhccq.kmeans_split call on a lone problem, ms; wide_wins = the median gain exceeds the larger max - min", "rows": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"wide_wins": {r["problem"]: r["wide_wins"] for r in rows}}))


if __name__ == "__main__":
    main()
