#!/bin/bash
# profiles of round 4 (run on the GPU box from the repository root, results under OUTDIR): kernel stats of the bench command with
# --full, PMC traffic of the per-pixel passes (separate FETCH_SIZE / WRITE_SIZE passes on a three-frame run), the --full bench line itself
#   tools/pmc4.sh OUTDIR
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${1:?usage: tools/pmc4.sh OUTDIR}
export OUT
mkdir -p "$OUT"
python3 bench.py --steps 10 --warmup 2 --full > "$OUT/bench4k.json" 2> "$OUT/bench4k.err" &&
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/stats" -o s -- python3 bench.py --full > "$OUT/stats.log" 2>&1 &&
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_FETCH_SIZE" -o p -- python3 tools/oneframe.py > "$OUT/pmc_f.log" 2>&1 &&
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_WRITE_SIZE" -o p -- python3 tools/oneframe.py > "$OUT/pmc_w.log" 2>&1
python3 - <<'PY'
import csv, glob, json, collections, os
OUT = os.environ["OUT"]
out = {}
for name in ("FETCH_SIZE", "WRITE_SIZE"):
    for f in glob.glob(f"{OUT}/pmc_{name}/**/*counter_collection.csv", recursive=True):
        acc = collections.defaultdict(list)
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == name:
                acc[r["Kernel_Name"].split("(")[0]].append(float(r["Counter_Value"]))
        for k, v in acc.items():
            out.setdefault(k, {})[name] = {"launches": len(v), "mean": sum(v) / len(v)}
sel = {k: v for k, v in out.items() if any(s in k for s in ("job_scan", "bytemap_pack", "job_index", "frame_remap", "mbk_assign", "cluster_sums", "mbk_init3"))}
json.dump(sel, open(f"{OUT}/pmc_fetch_write_kb.json", "w"), indent=1)
print(json.dumps(sel, indent=1))
PY
